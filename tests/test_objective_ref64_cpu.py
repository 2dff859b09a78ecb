"""tests/objective_ref64.py (the float64 reference of tests/test_objective_float64_gpu.py) evaluated in fp32 must be the oracle:
compositing against oracle/render_ref.py::volume_weights and the composite sums on the func_rows golden, ray lifting against
camera_rays / camera_from_tensor on the a1 / a17 rows, the loss terms against the four loss goldens.  Then, on the very inputs the GPU
test uses (tests/objective_cases.py), the two facts its gate relies on: the last interval's alpha is exactly 0 or 1 on every ray, and
the yardstick (fp32 mode against float64 mode) is small -- a gate against a yardstick that is itself O(1) wrong cannot pass by accident --
and the shares of rays the GPU test leaves out (ill-conditioned depth quotient, kinks) stay under their caps for the reference alone.
Run with -s for the per-group table."""
import math

import pytest
import torch

import objective_cases as C
import objective_ref64 as O
from helpers import load, tt, assert_close
from oracle import render_ref as R

F32 = torch.float32


# ------------------------------------------------------------------------------------------------------------------ fp32 mode = oracle
def test_composite_in_fp32_is_the_oracle_bit_for_bit():
    """Same operations in the same order as volume_weights / density / beta_from_voxels (which tests/test_func_rows_cpu.py pins to the
    reference's own outputs at the golden's points) and the sums of render_ref.render, so the fp32 mode has to reproduce them exactly:
    the forward, and the gradients to sdf, rgb and grad sdf as well -- autograd walks the same graph, and the one difference, the
    oracle's derivative of the last alpha where the restatement has a constant, is exactly 0 (alpha is exactly 0 or 1 there: expm1's
    backward, result + 1, or exp(-1e10 sigma) is 0), and adding an exact zero changes no sum."""
    fx = load("func_rows")
    vox, z = tt(fx["a11_voxels"]), tt(fx["a13_z"])
    Rn, S = z.shape
    g = torch.Generator().manual_seed(2)
    o = (torch.rand(Rn, 3, generator=g) - 0.5) * 0.4
    d = torch.nn.functional.normalize(torch.rand(Rn, 3, generator=g) - 0.5, dim=-1) * 0.45
    rgb, grad = torch.rand(Rn, S, 3, generator=g), torch.randn(Rn, S, 3, generator=g)
    for last in (None, 0.0005, 0.5):                    # the golden's rays, then every ray ending near / far from the surface
        sdf = tt(fx["a13_sdf"]).reshape(Rn, S).clone()
        if last is not None:
            sdf[:, -1] = last
        out = O.composite(z, sdf, rgb, grad, o, d, vox, 64, dtype=F32)
        x = O.sample_points(z, o, d).reshape(-1, 3)
        assert torch.equal(x, (o[:, None] + z[..., None] * d[:, None]).reshape(-1, 3))
        s_, c_, g_ = (t.clone().requires_grad_(True) for t in (sdf, rgb, grad))
        w = R.volume_weights(z, s_.reshape(-1, 1), x, vox, 64)
        ref = dict(weights=w, rgb_values=torch.sum(w.unsqueeze(-1) * c_, 1),
                   depth=(torch.sum(w * z, 1, keepdims=True) / (w.sum(dim=1, keepdims=True) + 1e-8))[:, 0],
                   nmap=torch.sum(w.unsqueeze(-1) * (g_ / (g_.norm(2, -1, keepdim=True) + 1e-6)), 1),
                   entropy=(-w * torch.log(w + 1e-4)).sum(dim=-1))
        for k in O.COMPOSITE_OUT:
            assert torch.equal(getattr(out, k).detach(), ref[k].detach()), k
        cot = {"g_" + k: torch.randn(ref[k].shape, generator=g) for k in O.COMPOSITE_OUT}
        for keep in [(k,) for k in O.COMPOSITE_OUT] + [O.COMPOSITE_OUT]:
            obj = sum((cot["g_" + k] * ref[k]).sum() for k in keep)
            gs_o = torch.autograd.grad(obj, (s_, c_, g_), retain_graph=True, allow_unused=True)
            gs = O.composite_backward(out, **{"g_" + k: cot["g_" + k] for k in keep})
            for name, a, b in zip(("sdf", "rgb", "grad"), gs, gs_o):
                b = torch.zeros_like(a) if b is None else b
                assert torch.equal(a, b), f"d/d {name} of {keep}"
        assert bool((O.composite_backward(out, **cot)[0][:, -1] == 0).all())          # the last sample's sdf gradient: exactly 0


def test_rays_in_fp32_are_the_oracle_on_the_golden_rows():
    fx = load("func_rows")
    uv, K, pose, cam = tt(fx["a1_uv"]), tt(fx["a1_K"]), tt(fx["a1_pose"]), tt(fx["a17_cam"])
    r = O.rays(uv, pose, K, dtype=F32)
    d_o, loc = R.camera_rays(uv, pose, K)
    assert torch.equal(r.rays_d.detach(), d_o) and torch.equal(r.rays_o[:, 0].detach(), loc)
    assert_close(r.rays_d.detach(), fx["a1_ray_dirs"], 1e-6, 1e-5, "ray_dirs vs the reference golden")
    assert_close(r.rays_o[:, 0].detach(), fx["a1_cam_loc"], 0, 0, "cam_loc")
    eye = torch.eye(4)[None].repeat(3, 1, 1)
    assert torch.equal(r.depth_scale.detach(), R.camera_rays(uv, eye, K)[0][:, :, 2])
    rc = O.rays(uv, cam, K, dtype=F32)
    assert torch.equal(rc.pose.detach(), R.camera_from_tensor(cam))
    assert_close(rc.pose.detach(), fx["a17_pose"], 1e-6, 1e-6, "pose vs the reference golden")
    # the backward to the 7-vector: autograd through the oracle's own functions
    g = torch.Generator().manual_seed(0)
    g_o, g_d = torch.randn(3, 11, 3, generator=g), torch.randn(3, 11, 3, generator=g)
    cam_o = cam.clone().requires_grad_(True)
    d_o, loc = R.camera_rays(uv, R.camera_from_tensor(cam_o), K)
    ((g_d * d_o).sum() + (g_o * loc[:, None]).sum()).backward()
    assert_close(O.rays_pose_backward(rc, g_o, g_d), cam_o.grad, 1e-6, 1e-5, "d/d cam")
    r64 = O.rays(uv, cam, K)
    assert_close(O.rays_pose_backward(r64, g_o, g_d), cam_o.grad, 1e-4, 1e-3, "d/d cam, float64 vs the fp32 oracle")


class _DS:
    data_dir = "../Datasets/processed/Replica"


def _golden_loss_inputs(name):
    """a loss golden as the arguments of slam_terms, with the weights SLAMLoss.forward would use (tests/test_loss_cpu.py)"""
    from nicer_slam_amd.model.loss import SLAMLoss
    fx = load(name)
    if "meta_data_dir" in fx:
        from nicer_slam_amd.utils.conf import run_conf
        rc = next(c for c in map(run_conf, ("replica", "7scenes", "azure")) if c["data_dir"] == str(fx["meta_data_dir"]))
        crit = SLAMLoss(scan_id=1, **rc["loss"])
    else:
        crit = SLAMLoss(rgb_loss="torch.nn.L1Loss", eikonal_weight=0.1, train_dataset=_DS(), scan_id=1, assign_scale_shift_init=True,
                        smooth_weight=0.005, warp_loss_type="l1", depth_weight=0.1, normal_l1_weight=0.05, normal_cos_weight=0.05,
                        flow_weight=0.001, warp_loss_weight=0.5)
    bs, n = fx["in_depth_values"].shape[:2]
    out = {k: tt(fx["in_" + k]) for k in ("rgb_values", "depth_values", "grad_theta", "grad_theta_nei", "sdf")}
    out["normal_map"] = tt(fx["in_normal_map"]).reshape(bs, n, 3)
    gt = dict(rgb=tt(fx["gt_rgb"]), depth=tt(fx["gt_depth"]), normal=tt(fx["gt_normal"]).reshape(bs, n, 3), mask=tt(fx["gt_mask"]),
              gt_depth=tt(fx["gt_gt_depth"]), gt_depth_mask=tt(fx["gt_gt_depth"]))
    w_gt = crit.gt_depth_weight
    if crit.assign_scale_shift_init:
        w_gt = 10.0 if int(fx["meta_frame_idx"]) == 0 else 0.0
        if int(fx["meta_frame_idx"]) == 0:
            gt["gt_depth"] = gt["depth"] * crit.assign_scale
    w = (crit.rgb_loss_weight, crit.eikonal_weight, crit.smooth_weight, crit.depth_weight, w_gt, crit.normal_l1_weight,
         crit.normal_cos_weight)
    return fx, out, gt, w


@pytest.mark.parametrize("name", ["loss_mapping_first_frame", "loss_mapping_fine", "loss_mapping_7scenes", "loss_mapping_azure_first_frame"])
def test_slam_terms_in_fp32_reproduce_the_loss_goldens(name):
    fx, out, gt, w = _golden_loss_inputs(name)
    for dtype, atol, gtol in ((F32, 1e-6, 1e-7), (torch.float64, 2e-6, 2e-7)):
        res = O.slam_terms(out, gt, w, whole_image=False, dtype=dtype)
        t = dict(zip(O.TERMS, res.terms))
        wd = dict(zip(O.TERMS, w))
        for key, val in (("rgb_loss", wd["rgb"] * t["rgb"]), ("eikonal_loss", wd["eikonal"] * t["eikonal"]),
                         ("smooth_loss", wd["smooth"] * t["smooth"]), ("depth_loss", t["depth"]), ("normal_l1", t["normal_l1"]),
                         ("normal_cos", t["normal_cos"]), ("gt_depth_loss", t["gt_depth"])):
            assert_close(torch.as_tensor(float(val)), fx["out_" + key], atol, 1e-5, key)
        rest = float(fx["out_loss"]) - float(fx["out_flow_loss"]) - float(fx["out_warp_loss"])
        assert_close(torch.as_tensor(float(res.total)), torch.as_tensor(rest), 2 * atol, 1e-5, "total without flow / warp")
        for k in O.LOSS_LEAVES:
            if "grad_" + k in fx:
                assert_close(res.grads[k].reshape(fx["grad_" + k].shape), fx["grad_" + k], gtol, 1e-4, "d/d " + k)


# ------------------------------------------------------------------------------------------------------------------ the GPU test's inputs
# Caps on the yardstick's own error (fp32 mode against float64 mode), from the arithmetic and not from a run:
#   forward, per ray, divided by max(|ref|, 1): a weight is alpha exp(-sum of <= S energies); where it is not negligible (> 2^-24) the
#   exponent is below 17, and an fp32 prefix sum of S terms carries at most S 2^-24 of it: S 2^-24 17 = 2.6e-4 at S = 256.  The ray sums
#   add S rounded products of weights that sum to <= 1: below that.
#   backward, per ray, relative to the ray's own float64 gradient or, where that is smaller, to the median ray gradient of the case
#   times the ray's cotangent scale.  Two terms, added: (i) the forward's exponent error FWD_CAP enters a sample's gradient once
#   through each of T, alpha and the suffix sum: 3 FWD_CAP = 7.8e-4; (ii) d sigma / d sdf carries expm1(-|s| / beta) + 1, which fp32
#   holds to an ABSOLUTE 2^-25 (it is a multiple of 2^-24 next to -1), i.e. to a relative 2^-25 e^(|s| / beta): 6.6e-4 at
#   |s| / beta = 10.  BWD_CAP = 3 FWD_CAP + 2^-25 e^10 = 1.44e-3 therefore bounds every ray that has a sample with a gradient (any but
#   the last) at |s| / beta <= 10.  A ray whose nearest such sample is at rho = |s| / beta > 10 has a gradient of e^-rho of those, all
#   of it quantised, and is held to BWD_CAP of the median ray or, failing that, to the same formula at its own rho of its own gradient: 3 FWD_CAP + 2^-25 e^rho (4.1e-3 at rho = 11.8; above 1 from rho = 17.3,
#   where fp32 returns exactly 0 -- 100 % of that gradient, and fp32's honest answer).  Such rays are counted in the printed table.
#   Without the last-interval rule the figure is 1 on every ray that ends in empty space, whatever its rho.
FWD_CAP = 256 * 2.0 ** -24 * 17
QUANTISED = 10.0
BWD_CAP = 3 * FWD_CAP + 2.0 ** -25 * math.exp(QUANTISED)


def _rel_rows(a, b):
    a, b = a.detach().double().reshape(a.shape[0], -1), b.detach().double().reshape(b.shape[0], -1)
    return (a - b).norm(dim=1), b.norm(dim=1)


@pytest.mark.parametrize("R_,S", [(5, 1), (5, 2), (5, 65), (5, 193), (C.COMPOSITE_R_BIG, 98), (C.COMPOSITE_R_BIG, 128),
                                  (C.COMPOSITE_R_BIG, 160), (C.COMPOSITE_R_BIG, 256)])
def test_composite_yardstick_is_small_and_last_alpha_is_0_or_1(R_, S, capsys):
    case = C.composite_case(R_, S, seed=100 + S)
    args = C.composite_args(case)
    a = O.last_alpha(case["z"], case["sdf"], case["rays_o"], case["rays_d"], case["voxels"], C.RES)       # asserts 0 / 1
    o64, o32 = O.composite(*args), O.composite(*args, dtype=F32)
    c, cot = C.composite_cotangents(case, seed=200 + S)
    left = o64.weights.detach().sum(1) < C.SUM_W_MIN
    grp = case["group"]
    beta32 = O.beta_of(O.visit_counts(O.sample_points(case["z"], case["rays_o"], case["rays_d"]), case["voxels"], C.RES), F32)
    rho = (case["sdf"].reshape(R_, S).abs() / beta32)[:, :-1].double()
    rho = rho.amin(1) if S > 1 else torch.zeros(R_, dtype=torch.float64)       # (S = 1: no sample has a gradient)
    bwd_cap = 3 * FWD_CAP + 2.0 ** -25 * torch.exp(rho.clamp_min(QUANTISED))   # [R]; BWD_CAP wherever rho <= 10
    with capsys.disabled():
        print(f"\n  composite R = {R_} S = {S}: last alpha 0 on {int((a == 0).sum())}, 1 on {int((a == 1).sum())} rays (no other value); "
              f"left out of depth (sum w < {C.SUM_W_MIN}): {float(left.double().mean()):.3f} of the rays, group 4 is "
              f"{float((grp == 3).double().mean()):.3f}; rays whose nearest sample with a gradient is beyond |s| / beta = {QUANTISED:g}: "
              f"{int((rho > QUANTISED).sum())}")
        assert not bool((left & (grp != 3)).any()), "a ray of groups 1-3 has no weight"
        assert float(left.double().mean()) <= float((grp == 3).double().mean())
        for gi, gname in enumerate(C.GROUPS):
            sel = grp == gi
            if not bool(sel.any()):
                continue
            line = []
            for k in O.COMPOSITE_OUT:
                keep = sel & ~left if k == "depth" else sel
                if not bool(keep.any()):
                    continue
                e, n = _rel_rows(getattr(o32, k)[keep], getattr(o64, k)[keep])
                e = e / n.clamp_min(1.0)
                line.append(f"{k} {float(e.max()):.1e}")
                assert float(e.max()) <= FWD_CAP * max(S, 64) / 256, (gname, k, float(e.max()))
            print(f"    {gname:<26s} forward max: " + "  ".join(line))
            for name in C.COTANGENTS + ("all",):
                kw = dict(cot) if name == "all" else {name: cot[name]}
                if "g_depth" in kw:
                    kw["g_depth"] = torch.where(left, torch.zeros_like(kw["g_depth"]), kw["g_depth"])
                g64, g32 = O.composite_backward(o64, **kw), O.composite_backward(o32, **kw)
                live = sel & (c > 0)
                line = []
                for what, x64, x32 in zip(("sdf", "rgb", "grad"), g64, g32):
                    every = c > 0
                    per_ray = _rel_rows(x32[every], x64[every])[1] / c[every]
                    med = float(per_ray.median())                                                # the median ray gradient of the case
                    e, n = _rel_rows(x32[live], x64[live])
                    if med > 0 and bool(live.any()):
                        rel = e / torch.maximum(n, c[live] * med)
                        rms = float((rel ** 2).mean().sqrt())
                        line.append(f"d/d{what} rms {rms:.1e} max {float(rel.max()):.1e}")
                        own = e <= bwd_cap[live] * n if what == "sdf" else torch.zeros_like(rel, dtype=torch.bool)
                        assert bool(((rel <= BWD_CAP) | own).all()), (gname, name, what, float(rel.max()))
                    assert bool((x32[sel & (c == 0)] == 0).all()) and bool((x64[sel & (c == 0)] == 0).all())
                assert bool((g64[0][:, -1] == 0).all()) and bool((g32[0][:, -1] == 0).all())
                print(f"      {name:<14s} " + "  ".join(line))


def test_composite_last_alpha_is_0_or_1_on_every_shape_of_the_gpu_test():
    for R_, S in C.composite_shapes():
        case = C.composite_case(R_, S, seed=100 + S)
        a = O.last_alpha(case["z"], case["sdf"], case["rays_o"], case["rays_d"], case["voxels"], C.RES)
        assert bool(((a == 0) | (a == 1)).all())
        if R_ >= 32:
            assert int((a == 0).sum()) > R_ // 8 and int((a == 1).sum()) > R_ // 4        # both kinds of ray are there


@pytest.mark.parametrize("S", C.COMPOSITE_S_BIG)
def test_tracking_kinks_of_the_reference_stay_under_one_percent(S, capsys):
    case = C.composite_case(C.COMPOSITE_R_BIG, S, seed=100 + S)
    a = C.composite_args(case)
    gt = C.track_gt(case, seed=300 + S)
    _rgb, _l, _g, margin = O.composite_track(a[0], a[1], a[2], *a[4:], gt, 2 * case["R"] + 3)
    share = float((margin < C.KINK).double().mean())
    with capsys.disabled():
        print(f"\n  composite_track S = {S}: rays within {C.KINK} of an L1 kink: {share:.4f}")
    assert share < 0.01


def test_rays_yardstick_is_small(capsys):
    with capsys.disabled():
        print()
        for b, n in ((1, 1), (3, 1025), (8, 8192 + 7)):
            cs = C.rays_case(b, n, seed=b + n)
            r64, r32 = O.rays(cs["uv"], cs["cam"], cs["K"]), O.rays(cs["uv"], cs["cam"], cs["K"], dtype=F32)
            assert torch.equal(r32.rays_o.detach().double(), r64.rays_o.detach())
            # |t| <= 100 enters v = (R c + t) - t: 100 2^-24 per component against |v| >= 1, then d = v / |v|^2
            e = (r32.rays_d.detach().double() - r64.rays_d.detach()).norm(dim=-1) / r64.rays_d.detach().norm(dim=-1)
            assert float(e.max()) <= 128 * 2.0 ** -24 * 4, float(e.max())
            g64 = O.rays_pose_backward(r64, cs["g_o"], cs["g_d"])
            g32 = O.rays_pose_backward(r32, cs["g_o"], cs["g_d"])
            cmax = cs["c"].reshape(b, n).amax(1)
            live = cmax > 0
            assert bool((g64[~live] == 0).all()) and bool((g32[~live] == 0).all())
            eg = (g32.double() - g64)[live].norm(dim=1) / g64[live].norm(dim=1)
            print(f"  rays b = {b} n = {n}: rays_d rel err max {float(e.max()):.1e}; d/d cam rel err per image max {float(eg.max()):.1e}")
            assert float(eg.max()) <= 1e-2          # a sum of n fp32 terms at most 128 2^-24 each off, some cancelling: far below O(1)


def test_loss_kinks_of_the_reference_stay_under_one_percent(capsys):
    with capsys.disabled():
        print()
        for shape, variant in C.loss_cases():
            out, gt, w, whole = C.loss_case(shape, variant, seed=7)
            r64 = O.slam_terms(out, gt, w, whole)
            r32 = O.slam_terms(out, gt, w, whole, dtype=F32)
            dk, nk = C.loss_kinks(r64.aux, shape)
            near = variant == "near_singular"
            print(f"  loss {shape} {variant:<22s} depth kinks {float(dk.double().mean()):.4f}  normal kinks {float(nk.double().mean()):.4f}  "
                  f"terms fp32 - float64 max {float((r32.terms.double() - r64.terms).abs().max()):.1e}")
            assert float(nk.double().mean()) < 0.01
            if not near:                             # (image 0 of that variant is rank-deficient in fp32: reported by the GPU test)
                assert float(dk.double().mean()) < 0.01
                assert float((r32.terms.double() - r64.terms).abs().max()) <= 1e-4
