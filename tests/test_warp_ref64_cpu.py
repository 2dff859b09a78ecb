"""What keeps tests/warp_ref64.py honest (no GPU): the restatement the re-projection kernels are held to by
tests/test_warp_float64_gpu.py.

  * its fp32 mode reproduces the torch twin model/warp.py on the inputs of the golden ``reproj_blocks`` to the tolerances of
    tests/test_warp_cpu.py, and meets that file's check_forward / check_backward against the golden itself (the reference's recorded
    output, code/model/network.py:153-279), with w2c = inv(pose) as a node of the graph;
  * its float64 mode agrees with the float64 evaluation of the twin (F.grid_sample, torch.linalg.inv) on cases of tests/warp_cases.py
    with a different K per frame, skew, a frame index and fractional pixels: values, masks, and the gradients of random cotangents;
  * on EVERY case of warp_cases.py: the fp32 yardstick's own error is printed (rms and max per quantity, per row and relative to the
    row's norm as the GPU test forms them) and bounded -- a yardstick that is itself far off makes the gate vacuous --, and the caps
    on what the gates leave out are asserted on the restatement alone (warp_cases.check_caps)."""
from types import SimpleNamespace

import pytest
import torch

import warp_cases as C
import warp_ref64 as R
from helpers import assert_close, load, tt
from test_warp_cpu import check_backward, check_forward, reproj_inputs

F32, F64 = torch.float32, torch.float64


def _blocks(d, model, dtype, cast=lambda t: t):
    """the restatement on reproj-shaped inputs, its leaves the graph nodes depth, pose and inv(pose)"""
    bs = d["uv"].shape[0]
    pose = cast(d["pose"])
    leaves = (cast(d["depth"]).reshape(bs, -1), pose, torch.linalg.inv(pose))
    out = {}
    for ps in model.patchsizes:
        o = R.patch_warp(d["uv"], None, None, d["K"], None, d["full_rgb"].reshape(bs, -1, 3), d["full_depth"].reshape(bs, -1, 1), None,
                         model.H, model.W, ps, dtype=dtype, leaves=leaves)
        out[ps] = (o.gt_rgb, o.sampled, o.mask, None if o.flat is None else o.flat.reshape(-1))
    fl = R.flow(d["uv"], None, None, d["K"], None, d["edges"][0], d["edges"][1], dtype=dtype, leaves=leaves).flow
    return out, fl


def test_fp32_mode_reproduces_the_twin_and_meets_the_golden():
    from nicer_slam_amd.model.warp import flow_reproject, patch_warp
    fx = load("reproj_blocks")
    d, model = reproj_inputs(fx)
    bs = d["uv"].shape[0]
    ours, flow = _blocks(d, model, F32)
    check_forward(fx, ours, flow)
    terms = {f"warp{ps}": (s[m] - g[m]).abs().mean() for ps, (g, s, m, _) in ours.items()}
    terms["flow"] = (flow[d["flow_mask"]] - d["gt_flow"][d["flow_mask"]]).abs().mean()
    for (tag, t), ref in zip(terms.items(), list(fx["out_warp_terms"]) + [fx["out_flow_term"]]):
        assert abs(float(t) - float(ref)) < 1e-5 * max(1.0, abs(float(ref))), tag
    check_backward(fx, terms, d["depth"], d["pose"])
    with torch.no_grad():
        twin = patch_warp(model, d["uv"], d["pose"], d["K"], d["depth"].reshape(-1, 1).unsqueeze(2),
                          {"full_rgb": d["full_rgb"], "full_depth": d["full_depth"]}, bs)
        twin_flow = flow_reproject(d["uv"], d["pose"], d["K"], d["depth"], d["edges"])
    assert_close(flow, twin_flow, 2e-4, 1e-5, "flow vs twin")
    for ps, (g, s, m, ray) in ours.items():
        g_t, s_t, m_t, ray_t = twin[ps]
        assert torch.equal(g, g_t), ps
        assert float((m == m_t).float().mean()) > 0.995, ps
        assert_close(s, s_t, 2e-5, 1e-5, f"warp{ps} sampled vs twin")
        if ps > 1:
            assert torch.equal(ray, ray_t)


def _twin64(c, depth, pose):
    """model/warp.py in float64 on a case (it forms w2c = inv(pose) itself and takes the frames stacked)"""
    from nicer_slam_amd.model.warp import patch_warp
    b = c["b"]
    model = SimpleNamespace(H=c["H"], W=c["W"], patchsizes=[c["patch"]])
    gt = {"full_rgb": R.frames_of(c["images"], c["frame_index"], b).double(), "full_depth": R.frames_of(c["depths"], c["frame_index"], b).double()}
    return patch_warp(model, c["uv"].double(), pose, c["K"].double(), depth.reshape(-1, 1).unsqueeze(2), gt, b)[c["patch"]]


@pytest.mark.parametrize("name", ["b3 n65 48x33 p5", "b8 n255 48x33 p1", "b2 n63 24x40 p11", "b3 n63 24x40 p3 frac"])
def test_float64_mode_agrees_with_the_twin_in_float64(name):
    c = C.patch_case(name)
    b, n = c["b"], c["n"]
    ex = C.exclusions(c, C.evaluate(c, F64), C.evaluate(c, F32))
    g_sampled = C.g_sampled_of(c, torch.where(ex["rows"], torch.zeros_like(c["scale"]), c["scale"]).clamp(max=1.0)).double()
    grads = []
    for which in ("ours", "twin"):
        depth, pose = c["depth"].double().requires_grad_(True), c["pose"].double().requires_grad_(True)
        if which == "ours":
            o = R.patch_warp(c["uv"], None, None, c["K"], None, c["images"], c["depths"], c["frame_index"], c["H"], c["W"], c["patch"],
                             leaves=(depth, pose, torch.linalg.inv(pose)))
            gt_rgb, sampled, mask, ray = o.gt_rgb, o.sampled, o.mask, (None if o.flat is None else o.flat.reshape(-1))
        else:
            gt_rgb, sampled, mask, ray = _twin64(c, depth, pose)
        grads.append((gt_rgb, sampled, mask, ray) + torch.autograd.grad((g_sampled * sampled).sum(), (depth, pose)))
    (g_o, s_o, m_o, r_o, gd_o, gp_o), (g_t, s_t, m_t, r_t, gd_t, gp_t) = grads
    assert torch.equal(g_o.double(), g_t)
    assert_close(s_o, s_t, 1e-11, 1e-11, "sampled")
    # (two float64 evaluations may still disagree where a comparison is decided by the last bit: a frame's own border pixels)
    assert bool(((m_o != m_t) <= ex["mask"]).all()), "the twin's mask differs from the restatement's outside the exclusions"
    if r_o is not None:
        assert torch.equal(r_o, r_t)
    assert_close(gd_o, gd_t, 1e-9 * float(gd_t.abs().max()), 1e-9, "d / d depth")
    assert_close(gp_o, gp_t, 1e-9 * float(gp_t.abs().max()), 1e-9, "d / d pose, through the inverse")


@pytest.mark.parametrize("name", ["b3 n255 special 5", "b8 n257 shipped 36"])
def test_float64_flow_agrees_with_the_twin_in_float64(name):
    from nicer_slam_amd.model.warp import flow_reproject
    c = C.flow_case(name)
    g_flow = C.g_flow_of(c, c["edges"], c["scale"].clamp(max=1.0)).double()
    res = []
    for which in ("ours", "twin"):
        depth, pose = c["depth"].double().requires_grad_(True), c["pose"].double().requires_grad_(True)
        if which == "ours":
            fl = R.flow(c["uv"], None, None, c["K"], None, c["idii"], c["idjj"], leaves=(depth, pose, torch.linalg.inv(pose))).flow
        else:
            fl = flow_reproject(c["uv"].double(), pose, c["K"].double(), depth, (c["idii"], c["idjj"]))
        res.append((fl,) + torch.autograd.grad((g_flow * fl).sum(), (depth, pose)))
    assert_close(res[0][0], res[1][0], 1e-10, 1e-11, "flow")
    for k, what in ((1, "d / d depth"), (2, "d / d pose, through the inverse")):
        assert_close(res[0][k], res[1][k], 1e-9 * float(res[1][k].abs().max()), 1e-9, what)


def _row_err(a, ref, norm):
    e = (a.detach().double() - ref.detach()).reshape(norm.numel(), -1).norm(dim=1) / norm.reshape(-1)
    return float((e ** 2).mean().sqrt()), float(e.max())


# The yardstick's own error, bounded from what fp32 can do (u = 2^-24 = 6e-8):
#   * sampled: the image values lie in [0, 1.02], so the bilinear sample has a slope of at most 1.02 per pixel in each axis (the
#     zero padding included); the coordinates are off by at most delta / 8 (the measured fp32 coordinate error), and the blend of four
#     texels adds a few u: per entry at most 1.02 (delta_ix + delta_iy) / 8 + 1e-6;
#   * flow: a pixel coordinate of size <= 64 after ~25 fp32 operations: 64 * 25 u = 1e-4 per row of norm >= 1 (the rows behind the
#     camera carry larger coordinates and the same RELATIVE error), rms a tenth of it;
#   * gradients: every term is a texel difference times a bilinear weight (absolute error delta / 8 on a range of 1) times a
#     projection derivative (relative error of a few hundred u where tz is small): a yardstick with three correct digits relative to
#     the rms size of the float64 rows, 1e-3, is what the gate needs to mean anything.
#     With ONE frame (b = 1, w2c perturbed by 1e-3) every derivative with respect to the depth is the difference of two terms a
#     thousand times its size -- against the exact inverse it would vanish --, three of those digits are lost, and g_depth is held
#     to one digit there, 1e-1; the pose gradients are not affected.
FLOW_MAX, FLOW_RMS, GRAD_REL, GRAD_REL_B1 = 1e-4, 1e-5, 1e-3, 1e-1


@pytest.mark.parametrize("name", list(C.PATCH_CASES))
def test_patch_cases_yardstick_error_and_exclusion_caps(name, capsys):
    c = C.patch_case(name)
    b, n, p2 = c["b"], c["n"], c["patch"] ** 2
    o64, o32 = C.evaluate(c, F64), C.evaluate(c, F32)
    ex = C.exclusions(c, o64, o32)
    line = C.check_caps(c, ex)
    assert bool(torch.isfinite(o64.sampled).all()) and bool(torch.isfinite(o32.sampled).all())
    assert torch.equal(o64.gt_rgb, o32.gt_rgb) and torch.equal(o64.inside, o32.inside)
    want = C.expected_mask(o64, ex, o32.flat)              # (on a row within the rounding bound of 0.01: with the fp32 mode's own flat bit)
    assert bool((o32.mask == want)[~ex["mask"]].all()), "the two modes disagree on a mask entry outside the exclusions"
    assert bool((o32.mask == want)[C.known_mask_entries(c, ex)].all()), "the two modes disagree on a mask entry of a known-edge row"
    assert torch.equal(C.expected_mask(o64, ex, o64.flat), o64.mask)
    if o64.flat is not None:
        assert bool((o64.flat == o32.flat)[~ex["flat"]].all()), "the two modes disagree on a flat row outside the exclusions"
        well = (o64.var < 0.5 * R.FLAT_LIMIT).sum(), (o64.var > 2 * R.FLAT_LIMIT).sum()
        assert min(int(w) for w in well) >= 1 or n < 16, "no patch variance well below / well above 0.01"
    if "near_plane" in c["known"]:
        r = c["known"]["near_plane"]
        for o in (o64, o32):
            big = torch.maximum(o.ix[b - 1, 0, r, 0].abs(), o.iy[b - 1, 0, r, 0].abs())
            assert not bool(o.ok[b - 1, 0, r, 0]) and float(big) >= 1e8 and bool(torch.isfinite(big)) and abs(float(o.tz[b - 1, 0, r, 0])) < 1e-6
            assert bool((o.sampled[b - 1, 0, r] == 0).all())
    if "behind" in c["known"]:
        assert int((o64.tz[:, 0, c["known"]["behind"]] < 0).sum()) >= b - 1          # (all but the frame that stands 0.6 behind)
    scale = torch.where(ex["rows"], torch.zeros_like(c["scale"]), c["scale"])
    g = C.g_sampled_of(c, scale)
    g64, g32 = R.backward(o64.sampled, o64.leaves, g), R.backward(o32.sampled, o32.leaves, g)
    fwd_norm = o64.sampled.detach().reshape(b * b * n, -1).norm(dim=1).clamp_min(1.0)
    nz = torch.where(scale == 0, torch.ones_like(scale), scale)
    ps, pt = C.pose_norms(scale, torch.ones(b, b, dtype=torch.bool))
    safe = lambda v: torch.where(v == 0, torch.ones_like(v), v)
    rows = {"sampled": _row_err(o32.sampled, o64.sampled, fwd_norm), "g_depth": _row_err(g32[0], g64[0], nz),
            "g_pose": _row_err(g32[1], g64[1], safe(ps)), "g_w2c": _row_err(g32[2], g64[2], safe(pt))}
    size = {"g_depth": _row_err(torch.zeros_like(g64[0]), g64[0], nz)[0], "g_pose": _row_err(torch.zeros_like(g64[1]), g64[1], safe(ps))[1],
            "g_w2c": _row_err(torch.zeros_like(g64[2]), g64[2], safe(pt))[1]}
    with capsys.disabled():
        print(f"\n  {name}: {line}")
        print("    fp32 yardstick against float64 (rms, max per row): " + ";  ".join(f"{k} {v[0]:.2e} {v[1]:.2e}" for k, v in rows.items())
              + ";  size of the float64 rows: " + "  ".join(f"{k} {v:.2e}" for k, v in size.items()))
    per_entry = 1.02 * (ex["delta"]["ix"] + ex["delta"]["iy"]) / 8 + 1e-6
    assert rows["sampled"][1] <= per_entry * (3 * p2) ** 0.5, (rows["sampled"], per_entry)
    assert rows["g_depth"][0] <= (GRAD_REL_B1 if b == 1 else GRAD_REL) * size["g_depth"], (rows["g_depth"], size["g_depth"])
    for k in ("g_pose", "g_w2c"):
        assert rows[k][1] <= GRAD_REL * size[k] or size[k] == 0, (k, rows[k], size[k])


@pytest.mark.parametrize("name", list(C.FLOW_CASES))
def test_flow_cases_yardstick_error(name, capsys):
    c = C.flow_case(name)
    b, n = c["b"], c["n"]
    o64, o32 = C.evaluate_flow(c, F64), C.evaluate_flow(c, F32)
    assert bool(torch.isfinite(o64.flow).all()) and bool(torch.isfinite(o32.flow).all())
    g = C.g_flow_of(c, c["edges"])
    g64, g32 = R.backward(o64.flow, o64.leaves, g), R.backward(o32.flow, o32.leaves, g)
    feeds = torch.zeros(b, b, dtype=torch.bool)
    feeds[c["idjj"], c["idii"]] = True
    ps, pt = C.pose_norms(c["scale"], feeds)
    has_edge = torch.zeros(b, dtype=torch.bool)
    has_edge[c["idii"]] = True
    assert bool((g64[0][~has_edge] == 0).all()) and bool((g64[1][~has_edge] == 0).all()), "a source without an edge has a gradient"
    assert bool((g64[2][~feeds.any(dim=1)] == 0).all()), "a target without an incoming edge has a gradient"
    nz = torch.where(c["scale"] == 0, torch.ones_like(c["scale"]), c["scale"])
    safe = lambda v: torch.where(v == 0, torch.ones_like(v), v)
    fwd_norm = o64.flow.detach().reshape(-1, 2).norm(dim=1).clamp_min(1.0)
    rows = {"flow": _row_err(o32.flow, o64.flow, fwd_norm), "g_depth": _row_err(g32[0], g64[0], nz),
            "g_pose": _row_err(g32[1], g64[1], safe(ps)), "g_w2c": _row_err(g32[2], g64[2], safe(pt))}
    size = {"g_depth": _row_err(torch.zeros_like(g64[0]), g64[0], nz)[0], "g_pose": _row_err(torch.zeros_like(g64[1]), g64[1], safe(ps))[1],
            "g_w2c": _row_err(torch.zeros_like(g64[2]), g64[2], safe(pt))[1]}
    with capsys.disabled():
        print(f"\n  flow {name}: fp32 yardstick against float64 (rms, max per row): "
              + ";  ".join(f"{k} {v[0]:.2e} {v[1]:.2e}" for k, v in rows.items())
              + ";  size of the float64 rows: " + "  ".join(f"{k} {v:.2e}" for k, v in size.items()))
    assert rows["flow"][0] <= FLOW_RMS and rows["flow"][1] <= FLOW_MAX, rows["flow"]
    assert rows["g_depth"][0] <= (GRAD_REL_B1 if b == 1 else GRAD_REL) * size["g_depth"], (rows["g_depth"], size["g_depth"])
    for k in ("g_pose", "g_w2c"):
        assert rows[k][1] <= GRAD_REL * size[k] or size[k] == 0, (k, rows[k], size[k])


def test_the_cases_cover_what_they_are_for():
    seen, kinds, index = set(), set(), set()
    for name, spec in C.PATCH_CASES.items():
        c = C.patch_case(name)
        seen |= set(c["known"]) | ({"var_rows"} if c["var_rows"] else set())
        kinds.add(spec[4])
        index.add(spec[5])
        K = c["K"]
        assert int((K[:, 0, 1] != 0).sum()) * 2 >= c["b"] and (c["b"] == 1 or bool((K[:, 0, 1] == 0).any()))
        assert c["b"] == 1 or float((K[:, 0, 0].max() / K[:, 0, 0].min())) > 1.02
        if spec[4] == "perturbed":
            off = (c["w2c"].double() @ c["pose"].double() - torch.eye(4, dtype=F64)).abs().max()
            assert 1e-5 < float(off) < 1e-2, float(off)
    want = {"corner_00", "corner_WH", "behind", "near_plane", "strip_left", "strip_right", "strip_top", "strip_bottom", "leaves_left",
            "leaves_right", "leaves_top", "leaves_bottom", "var_rows"}
    assert want <= seen, want - seen
    assert kinds == {"inv64", "inv_ex32", "perturbed"} and index == {"none", "perm", "shared"}
    assert {s[0] for s in C.PATCH_CASES.values()} == {1, 2, 3, 8} and {s[3] for s in C.PATCH_CASES.values()} == {1, 3, 5, 11}
    ns = {s[1] for s in C.PATCH_CASES.values()} | {s[1] for s in C.FLOW_CASES.values()}
    assert {1, 63, 64, 65, 255, 256, 257} <= ns
    assert len(C.SHIPPED_36) == 36
    frac = [C.patch_case(k)["uv"] for k, s in C.PATCH_CASES.items() if s[3] > 1 and s[2] != (2, 2) and s[6]]
    assert frac and all(int((uv != uv.floor()).any(-1).sum()) >= 100 for uv in frac), "no patch > 1 on a real image with fractional uv"
    waves = lambda per: -(-per // 256) * 4
    assert any(waves(s[1] * s[3] ** 2) > 21 for s in C.PATCH_CASES.values())
    assert any(s[0] * waves(s[1]) > 21 and len(s[2]) > s[0] for s in C.FLOW_CASES.values())
    g = C.g_sampled_of(C.patch_case("b3 n256 48x33 p3"))
    assert bool((g[:, 0, 5] == 0).all()) and float(g.abs().max()) > 2.0 ** 28


def test_masked_l1_restatement_against_torch():
    for items, ch, mask in ((257, 3, "random"), (65537, 2, "none"), (255, 1, "all")):
        pred, target, m = C.l1_case(items, ch, mask, 5)
        loss, g = R.masked_l1(pred, target, m, ch)
        a = pred.double().requires_grad_(True)
        sel = torch.ones(items, dtype=torch.bool) if m is None else m
        ref = (a[sel] - target.double()[sel]).abs().mean()
        ref.backward()
        assert abs(float(loss) - float(ref)) <= 1e-7 * float(ref)                # (the fp32 difference, rounded once, against the exact one)
        assert_close(g, a.grad, 0, 1e-6, "masked L1 gradient")
        assert bool((g.reshape(-1)[::17] == 0).all())                            # ties
        l64, g64 = R.masked_l1_float64(pred, target, m, ch)
        assert abs(float(l64) - float(ref)) <= 1e-12
    loss, g = R.masked_l1(*C.l1_case(300, 3, "empty", 1), 3)
    assert torch.isnan(loss) and bool((g == 0).all())
