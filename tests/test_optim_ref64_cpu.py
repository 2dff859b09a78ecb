"""The test of tests/test_optim_float64_gpu.py's instruments (no GPU): tests/optim_ref64.py is held to torch (float64 Adam to 1e-12,
the fp32 yardstick to torch's fp32 Adam through the gate, the weight norm to torch._weight_norm and its autograd), and the operand classes
of tests/optim_cases.py are shown to be sharp: with an fp32 restatement standing in for the kernel, the honest alternative order (the
camera kernel's) passes the gate on every class, and each of fourteen mutants is caught.  The mutant / class table is printed
(pytest -s) and kept in DESIGN.md section 7."""
import math
import types
import warnings

import numpy as np
import pytest
import torch

import optim_cases as C
import optim_ref64 as R
from gate64 import gate

F32, F64 = torch.float32, torch.float64
SCHEDULES = ((0, 1.0), (3, 0.5), (50, 0.95))


def _torch_adam(case, t, hyper, lr_step, gamma, dtype):
    """one step of torch.optim.Adam from the case's state, loaded with step = t - 1; StepLR moved to epoch t - 1 in closed form"""
    b1, b2, eps, lr = (R.f32(x) for x in hyper)
    p = case["p0"].to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    sd = opt.state_dict()
    sd["state"] = {0: dict(step=torch.tensor(float(t - 1)), exp_avg=case["m0"].to(dtype).clone(), exp_avg_sq=case["v0"].to(dtype).clone())}
    opt.load_state_dict(sd)
    if lr_step:
        sched = torch.optim.lr_scheduler.StepLR(opt, lr_step, R.f32(gamma))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched.step(t - 1)
    p.grad = case["g"].to(dtype).clone()
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == t
    return st["exp_avg"].detach(), st["exp_avg_sq"].detach(), p.detach()


@pytest.mark.parametrize("name", list(C.HYPER))
def test_float64_mode_is_torch_adam_and_the_fp32_yardstick_is_torch_fp32_adam(name, capsys):
    hyper = C.HYPER[name]
    b1, b2, eps, lr = hyper
    failures = []
    for t in C.STEPS:
        for lr_step, gamma in SCHEDULES:
            case = C.adam_case(2048, 11 * t + lr_step, eps, b1=b1)
            r64 = R.adam_step(case["p0"], case["g"], case["m0"], case["v0"], t, lr, b1, b2, eps, lr_step, gamma)
            norms = C.adam_norms(case, r64)
            for q, a, b, n in zip("mvp", _torch_adam(case, t, hyper, lr_step, gamma, F64), r64, norms):
                err = float(((a - b).abs() / n).max())
                assert err <= 1e-12, f"{name} t={t} StepLR({lr_step},{gamma}): {q} differs from torch float64 Adam by {err:.2e}"
            y32 = R.adam_step(case["p0"], case["g"], case["m0"], case["v0"], t, lr, b1, b2, eps, lr_step, gamma, dtype=F32)
            t32 = _torch_adam(case, t, hyper, lr_step, gamma, F32)
            keep = case["cls"] != ord("E")         # (class E's moments are rounding noise on both sides; its p is judged)
            for q, a, b, r, n in zip("mvp", y32, t32, r64, norms):
                k = None if q == "p" else keep
                what = f"{name} t={t} StepLR({lr_step},{gamma}) {q}"
                if b1 == 0 and q in "mp":          # torch's lerp takes its weight >= 0.5 branch, g - (g - m0) 0: m = g EXACTLY, which
                    if q == "m":                   # the documented order m0 + 1 (g - m0) is not -- one direction only
                        assert torch.equal(b, case["g"])
                else:
                    gate(what + ": yardstick vs torch fp32", a[:, None], r[:, None], b[:, None], n, k, failures)
                gate(what + ": torch fp32 vs yardstick", b[:, None], r[:, None], a[:, None], n, k, failures)
    assert not failures, [f["what"] for f in failures]


def test_weight_norm_reference_is_torch_weight_norm_and_its_autograd():
    for n_layers, seed in ((1, 0), (3, 1), (8, 2)):
        layers = C.wn_layers(n_layers, seed)
        g_flat, _c = C.wn_cotangent(layers, seed)
        leaves, parts = [], []
        for v, g, b in layers:
            v, g, b = (x.double().requires_grad_(True) for x in (v, g, b))
            leaves.append((v, g, b))
            parts += [torch._weight_norm(v, g[:, None], 0).reshape(-1), b]
        flat = torch.cat(parts + [torch.zeros(1, dtype=F64)])
        mine, norms = R.weight_norm_flat(layers)
        assert float(((flat.detach() - mine).abs() / mine.abs().clamp_min(1e-300)).max()) <= 1e-12
        grads = torch.autograd.grad((flat * g_flat.double()).sum(), [x for l in leaves for x in l])
        want = torch.cat([x.reshape(-1) for x in grads])
        got = R.weight_norm_flat_backward(layers, g_flat)
        # per row: relative to |g| ||gW|| / ||v|| (g_v) -- as a whole vector here, with the row scale spread over its elements
        off, fo, r0 = 0, 0, 0
        for v, g, _b in layers:
            rows, cols = v.shape
            gw = g_flat[fo:fo + rows * cols].double().reshape(rows, cols)
            fo += rows * cols + rows
            scale = (g.double().abs() * gw.norm(dim=1) / norms[r0:r0 + rows]).clamp_min(1e-300)
            e = (got[off:off + rows * cols] - want[off:off + rows * cols]).reshape(rows, cols).norm(dim=1) / scale
            assert float(e.max()) <= 1e-12, float(e.max())
            e_g = (got[off + rows * cols:off + rows * cols + rows] - want[off + rows * cols:off + rows * cols + rows]).abs()
            assert float((e_g / gw.norm(dim=1).clamp_min(1e-300)).max()) <= 1e-12
            assert torch.equal(got[off + rows * cols + rows:off + rows * cols + 2 * rows], want[off + rows * cols + rows:off + rows * cols + 2 * rows])
            off += rows * cols + 2 * rows
            r0 += rows


# ------------------------------------------------------------------------------------------------------------------ mutants
ADAM_MUTANTS = ("eps / sqrt(bc2)", "eps omitted", "bias corrections from t - 1", "old v in the denominator", "old m in the numerator",
                "m updated with b2", "g g formed first", "last n % 4 elements not stepped", "zero-gradient step leaves v undecayed",
                "StepLR exponent floor(t / lr_step)")


def adam_mutant(mutant, case, t, hyper, lr_step, gamma):
    """the table-order fp32 yardstick with one fault"""
    b1, b2, eps, lr = (R.f32(x) for x in hyper)
    gamma = R.f32(gamma)
    tb = t - 1 if mutant == "bias corrections from t - 1" else t
    bc1, bc2 = 1.0 - b1 ** tb, 1.0 - b2 ** tb
    k = (t // lr_step if mutant == "StepLR exponent floor(t / lr_step)" else (t - 1) // lr_step) if lr_step else 0
    lr_t = R.f32(lr * R.f32(gamma ** k)) if lr_step else lr
    step_size, bc2_sqrt = R.f32(lr_t / bc1), R.f32(math.sqrt(bc2))
    w1, w2 = R.f32(1 - b1), R.f32(1 - b2)
    p0, g, m0, v0 = (case[k_] for k_ in ("p0", "g", "m0", "v0"))
    m = m0 + (R.f32(1 - b2) if mutant == "m updated with b2" else w1) * (g - m0)
    v = v0 * b2 + (w2 * (g * g) if mutant == "g g formed first" else (w2 * g) * g)
    if mutant == "zero-gradient step leaves v undecayed":
        v = torch.where(g == 0, v0, v)
    root = (v0 if mutant == "old v in the denominator" else v).sqrt() / bc2_sqrt
    if mutant == "eps / sqrt(bc2)":
        denom = (root * bc2_sqrt + eps) / bc2_sqrt
    elif mutant == "eps omitted":
        denom = root
    else:
        denom = root + eps
    p = p0 - step_size * ((m0 if mutant == "old m in the numerator" else m) / denom)
    if mutant == "last n % 4 elements not stepped":
        cut = case["n"] // 4 * 4
        m, v, p = (torch.cat([a[:cut], b[cut:]]) for a, b in ((m, m0), (v, v0), (p, p0)))
    return m, v, p


def _adam_settings():
    for name, hyper in C.HYPER.items():
        for t in C.STEPS:
            for lr_step, gamma in ((0, 1.0), (3, 0.5) if t <= 7 else (50, 0.95)):      # (t = 1000, 100000 are multiples of 50, not of 3)
                yield name, hyper, t, lr_step, gamma


def test_camera_order_passes_on_every_class_and_every_adam_mutant_is_caught(capsys):
    failures, caught, caught_project = [], {m: set() for m in ADAM_MUTANTS}, {m: set() for m in ADAM_MUTANTS}
    for name, hyper, t, lr_step, gamma in _adam_settings():
        b1, b2, eps, lr = hyper
        case = C.adam_case(8195, 3 * t + lr_step, eps, b1=b1)
        args = (case["p0"], case["g"], case["m0"], case["v0"], t, lr, b1, b2, eps, lr_step, gamma)
        r64, y_t, y_c = R.adam_step(*args), R.adam_step(*args, dtype=F32), R.adam_step(*args, dtype=F32, order="camera")
        tag = f"{name} t={t} StepLR({lr_step},{gamma})"
        honest = C.AdamJudge(failures, table_order_only=True)
        honest.add(tag + " camera order", case, y_c, r64, y_t, y_t)
        honest.finish(tag + " camera order")
        for mutant in ADAM_MUTANTS:
            if mutant == "bias corrections from t - 1" and t == 1:
                continue                           # (1 - b^0 = 0: not a number, nothing to judge)
            got = adam_mutant(mutant, case, t, hyper, lr_step, gamma)
            before = set(caught[mutant])
            j = C.AdamJudge([], caught[mutant])
            j.add(tag + " " + mutant, case, got, r64, y_t, y_c)
            j.finish(tag + " " + mutant)
            if name == "project":
                caught_project[mutant] |= caught[mutant] - before
    capsys.readouterr()                            # (the gate's lines: thousands; the table below is what this test reports)
    with capsys.disabled():
        print("\n  mutant                                      caught in (quantity class, over all hyper-parameter sets, t and schedules)")
        for mutant in ADAM_MUTANTS:
            by_class, project = (sorted({c for _q, c in d[mutant]} - {"pooled"}) for d in (caught, caught_project))
            print(f"  {mutant:<42s}  {' '.join(sorted(q + c for q, c in caught[mutant] if c != 'pooled'))}   [classes {''.join(by_class)}; "
                  f"with the project's eps = 1e-15 alone: {''.join(project)}]")
    assert not failures, [f["what"] for f in failures]
    for mutant in ADAM_MUTANTS:
        assert {c for _q, c in caught[mutant]} - {"pooled"}, f"no class catches the mutant: {mutant}"
    # with the project's eps = 1e-15 the classes today's tests resemble (A and B) see neither where eps sits nor the order of (w2 g) g:
    # that is what D and F are for (with the tracker's 1e-8 class A reaches down to sqrt(v) ~ 4e-7 and does see eps at t = 1)
    for mutant in ("eps / sqrt(bc2)", "eps omitted", "g g formed first"):
        assert not ({c for _q, c in caught_project[mutant]} & {"A", "B"}), (mutant, caught_project[mutant])


LOSSES = (5.0, 3.0, 3.0, float("nan"), 4.0, 2.0, 2.0)


def test_keep_best_rule_and_its_two_mutants():
    cams = [np.full(7, float(i), dtype=np.float32) for i in range(1, len(LOSSES) + 1)]       # the camera after step i
    before = [np.full(7, float(i), dtype=np.float32) for i in range(0, len(LOSSES))]
    got = R.keep_best(LOSSES, cams)
    assert [float(b) for b, _c in got] == [5.0, 3.0, 3.0, 3.0, 3.0, 2.0, 2.0]
    assert [int(c[0]) for _b, c in got] == [1, 2, 2, 2, 2, 6, 6]
    assert R.keep_best([float("nan")], cams[:1]) == [(np.float32(1e10), None)]

    def mutant_le(losses, cams):
        best, cam, out = np.float32(1e10), None, []
        for l, c in zip(losses, cams):
            if np.float32(l) <= best:
                best, cam = np.float32(l), c
            out.append((best, cam))
        return out
    differs = lambda a, b: any(x[0] != y[0] or (x[1] is not y[1] and not np.array_equal(x[1], y[1])) for x, y in zip(a, b))
    assert differs(mutant_le(LOSSES, cams), got), "the sequence does not tell <= from <"
    assert differs(R.keep_best(LOSSES, before), got), "the sequence does not tell the camera before the step from the one after"


def _wn_rows(layers, g_flat, got, ref, y_a, y_b, norms64):
    """g_v per row -> (got, ref, y_a, y_b [rows, max cols], norm [rows] = |g| ||gW|| / ||v||)"""
    out, off, fo, r0 = [], 0, 0, 0
    width = max(v.shape[1] for v, _g, _b in layers)
    for v, g, _b in layers:
        rows, cols = v.shape
        gw = g_flat[fo:fo + rows * cols].double().reshape(rows, cols)
        fo += rows * cols + rows
        norm = g.double().abs() * gw.norm(dim=1) / norms64[r0:r0 + rows]
        pad = lambda t: torch.nn.functional.pad(t[off:off + rows * cols].double().reshape(rows, cols), (0, width - cols))
        out.append((pad(got), pad(ref), pad(y_a), pad(y_b), norm))
        off += rows * cols + 2 * rows
        r0 += rows
    return [torch.cat([o[i] for o in out]) for i in range(5)]


def test_weight_norm_backward_mutant_without_the_projection_is_caught(capsys):
    layers = C.wn_layers(8, 2)
    g_flat, _c = C.wn_cotangent(layers, 2)
    _flat, norms = R.weight_norm_flat(layers)
    ref = R.weight_norm_flat_backward(layers, g_flat)
    y_a = R.weight_norm_flat_backward(layers, g_flat, dtype=F32)
    y_b = R.weight_norm_flat_backward(layers, g_flat, dtype=F32, kernel_order=True)
    keep = torch.ones(norms.shape[0], dtype=torch.bool)
    fails = []
    two = lambda what, got, r, ya, yb, norm, failures: gate(what, got, r, ya, norm, keep, failures, kernel_order=yb)
    assert two("weight norm backward, kernel order for the kernel", *_wn_rows(layers, g_flat, y_b, ref, y_a, y_a, norms), fails), fails
    bad = R.weight_norm_flat_backward(layers, g_flat, dtype=F32, drop_projection=True)
    assert not two("weight norm backward without v s / |v|^3", *_wn_rows(layers, g_flat, bad, ref, y_a, y_b, norms), [])


def test_track_tail_reference_and_the_mutant_with_slot_7_unscaled(capsys):
    import objective_cases as OC
    case = OC.rays_case(1, 65, 3)
    uv, K, cam = case["uv"][0], case["K"][0], case["cam"][0]
    args = (uv, K, cam, case["g_o"], case["g_d"])
    plain = R.track_tail_g_cam(*args, weight=0.0, slot7=0.25)
    per_ray = R.per_ray_cam_terms(*args)
    assert float(((per_ray.sum(0) - plain[:7]).abs() / per_ray.abs().sum(0)).max()) <= 1e-12       # the per-ray terms add up
    assert float(plain[7]) == 0.25
    ref = R.track_tail_g_cam(*args, weight=3.0, slot7=0.25)
    assert ref.shape == (9,) and float(ref[8]) == 3.0 and float(ref[7]) == 0.75
    assert float(((ref[:7] - 3.0 * plain[:7]).abs() / per_ray.abs().sum(0)).max()) <= 1e-12
    y32 = R.track_tail_g_cam(*args, weight=3.0, slot7=0.25, dtype=F32)
    bad = R.track_tail_g_cam(*args, weight=3.0, slot7=0.25, dtype=F32, scale_slot7=False)
    norm = torch.cat([3.0 * per_ray.abs().sum(0), torch.tensor([0.75, 3.0], dtype=F64)])
    assert not gate("track_tail, slot 7 unscaled", bad[:, None], ref[:, None], y32[:, None], norm), "slot 7 is not judged"
    # nsa_track_finish's message on the same rays: the loss slot and the composition with rays_backward
    rb = OC.rays_backward_case(65, 7, 4)
    red = R.track_finish_red(uv, K, cam, rb["z"], rb["g_x"], rb["g_dir"], torch.full((65,), 0.5), weight=0.0)
    assert red.shape == (8,) and abs(float(red[7]) - 0.5 / 3) < 1e-15


# ------------------------------------------------------------------------------------------------------------------ voxels, keys, cases
def test_voxel_index_is_update_voxels_on_the_crafted_points():
    from nicer_slam_amd.model.network import SLAMNetwork
    for res in C.VOXEL_RES:
        for P in C.VOXEL_P:
            x = np.concatenate([C.crafted_points(P, 7 * P + res), C.run_points("straddle")])
            idx = R.voxel_index(x, res)
            xt = torch.from_numpy(x)
            keep = ~(xt.abs() > 0.99).any(dim=1)
            q = ((xt[keep] + 1) / 2 * res).long()
            want = q[:, 0] * res * res + q[:, 1] * res + q[:, 2]
            assert np.array_equal(idx[keep.numpy()], want.numpy()) and bool((idx[~keep.numpy()] == -1).all())
            assert int(keep.sum()) >= P // 2 and (P < 64 or int((~keep).sum()) > 0)
            if res <= 64:                          # the module's own method, unbound, on a stand-in that holds the counter
                net = types.SimpleNamespace(voxel_res=res, voxels=torch.zeros(res, res, res))
                SLAMNetwork.update_voxels(net, xt)
                assert np.array_equal(net.voxels.reshape(-1).numpy(), R.voxel_counts(x, res))
    # both fp32 neighbours of a cell boundary fall on different sides of it somewhere
    c = C.crafted_coordinates()
    one = lambda v: R.voxel_index(np.array([[v, 0.0, 0.0]], dtype=np.float32), 64)[0] // (64 * 64)
    b = np.float32(-0.5)
    assert one(np.nextafter(b, np.float32(-1))) + 1 == one(b) == one(np.nextafter(b, np.float32(1)))
    assert one(np.float32(0.99)) == 63 and one(np.nextafter(np.float32(0.99), np.float32(1))) == -1 // (64 * 64)
    assert np.float32(0.99) in c and np.float32(-0.0) in c


def test_morton_key_statement():
    x = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [np.nan, -1.0, -1.0], [-3.0, 3.0, 0.0], [-1.0 + 1 / 512, -1.0, -1.0],
                  [-1.0, -1.0 + 1 / 512, -1.0], [-1.0, -1.0, -1.0 + 1 / 512]], dtype=np.float32)
    k = R.morton_key(x)
    assert list(k[:3]) == [0, (1 << 30) - 1, 0]
    assert list(k[4:]) == [1, 2, 4]
    assert k[3] == sum(1 << (3 * b + 1) for b in range(10)) | 4 << 27        # x clamped to 0, y to 1023, z = 512


def test_left_out_conditions_hold_for_the_cases_alone():
    for name, (b1, b2, eps, lr) in C.HYPER.items():
        for t in C.STEPS:
            case = C.adam_case(2051, t, eps, b1=b1)
            cls = case["cls"]
            assert float((cls == ord("E")).double().mean()) <= 1 / 8 + 1e-3          # the only class with ungated quantities
            assert {chr(c) for c in cls.tolist()} == set(C.CLASSES)
            if name == "project":
                for k in ("g", "m0", "v0"):                                          # class D stays normal for eps = 1e-15
                    a = case[k][cls == ord("D")].abs()
                    assert bool((a >= 2.0 ** -126).all())
            r64 = R.adam_step(case["p0"], case["g"], case["m0"], case["v0"], t, lr, b1, b2, eps)
            other = (cls != ord("E")) & (cls != ord("F"))
            for q, a in zip("mvp", r64):
                assert bool(torch.isfinite(a).all()), (name, t, q)
                a = a[other].abs()
                assert bool(((a == 0) | (a >= 2.0 ** -126)).all()), f"{name} t={t}: a subnormal float64 {q} outside classes E and F"
            sub = case["v0"][cls == ord("E")]
            assert bool(((sub > 0) & (sub < 2.0 ** -126)).all())
            g = case["g"][cls == ord("F")].double()
            assert bool((g * g > 3.4028234663852886e38).all()) and bool(((1 - R.f32(b2)) * g * g < 3.4e38).all())
