"""The streaming kernels of the objective against float64 (tests/objective_ref64.py), ray by ray and image by image, through the C ABI:
compositing (nsa_composite_forward / _backward / _track), ray lifting and the camera chain (nsa_rays_forward, nsa_rays_pose_backward,
nsa_rays_backward, nsa_cam_to_pose, nsa_pose_grad_to_cam, nsa_track_head, nsa_l1_loss) and the loss terms (nsa_slam_loss).

The method is tests/test_gemm_float64_gpu.py's, and the gate is tests/gate64.py:
  * e_k = |kernel - float64|, e_32 = |fp32 mode of the same restatement - float64| (the yardstick; tests/test_objective_ref64_cpu.py
    holds that mode to oracle/render_ref.py and to the loss goldens, and bounds it on these very inputs),
  * PER RAY (or per image / per eikonal point): forward outputs divided by max(|float64 output|, 1), backward outputs by the ray's
    cotangent scale c_r; a row whose cotangents are all zero must come out exactly 0,
  * gate: rms(e_k) <= 1.5 rms(e_32) and max(e_k) <= 3 max(e_32), every output finite.
A gate over one or three rows is a coin toss between two correctly rounded results, so the small cases (R = 1, 3, 5 at every S; the
per-image quantities of the ray kernels; the loss scalars) are POOLED: their rows are gathered over the cases and judged once.

Inputs: tests/objective_cases.py -- four ray groups interleaved ray by ray (crossing; crossing in voxels visited up to 30 000 times,
1 / (2 beta^2) ~ 9e4; grazing with the last sample in empty space; miss), edges on known rays (sdf exactly 0, two equal z, a zero
grad row, points beyond 0.99 and exactly on +-0.99 -- voxel indices 0 and res - 1, the ends of the range: the kernel's clamp itself
is unreachable for |x| <= 0.99 --, the last sample at sdf / beta = 1, 10, 100), S on both sides of every change of lane ownership
(per = ceil(S / 64)), cotangent scales 2^U(-30, 30) with neighbours alternating 2^30 / 2^-30 and every 97th ray zero.

Left out, counted and capped: from `depth` and the g_depth pull-back the rays whose float64 sum of weights is below 1e-3 (the quotient
sum w z / (sum w + 1e-8) is ill-conditioned there; no ray of groups 1-3, at most the share of group 4); rays within 2e-6 of a kink of
the tracking L1; in the loss, rays whose depth-residual difference or unit-normal difference is below its fp32 rounding bound (< 1 %).

nsa_colour_forward_composite and nsa_colour_forward_track are tied bit for bit to nsa_composite_forward / nsa_composite_track by
tests/test_tiling_gpu.py and tests/test_track_fold_gpu.py and are not tested again here.

Measured on MI355X: DESIGN.md section 7 holds the printed table."""
import ctypes

import pytest
import torch

import objective_cases as C
import objective_ref64 as O
from devcall import dev, nan, ptr, st
from gate64 import Pool, fwd_norm, gate, report

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN = float("nan")


# Quantities that missed the gate against the reference-order yardstick on MI355X, traced, and found to be a different but equally
# valid fp32 order (DESIGN.md section 7 has the figures); each has a second fp32 evaluation in the kernel's order
# (objective_ref64.loss_grads_kernel_order, composite_g_grad_kernel_order):
#   * nsa_slam_loss, d/d normal_map and d/d grad_theta(_nei) on rows whose input is ZERO (derivative u / 1e-12 resp. q / 1e-5: nothing
#     else contributes, so one rounding shows): the kernel multiplies by invR = fl(1 / R), invE = fl(1 / E) where torch divides the
#     cotangent by the count -- a systematic extra rounding, 5.9e-8 for R = 255 and 4.5e-8 for E = 7 on EVERY row of the batch;
#   * nsa_composite_backward, g_grad on rays with a zero grad row (derivative w g_nmap / 1e-6): inv = 1 / (|g| + 1e-6) and two
#     products, three roundings, where autograd divides once, two roundings -- 1.57 x rms on the two such rays of S = 160.


# ------------------------------------------------------------------------------------------------------------------ compositing
class DevCase:
    def __init__(self, case):
        self.R, self.S = case["R"], case["S"]
        self.t = {k: dev(case[k]) for k in ("rays_o", "rays_d", "z", "sdf", "rgb", "grad", "voxels")}

    def head(self, with_grad=True):
        t = self.t
        return [ptr(t["rays_o"]), ptr(t["rays_d"]), ptr(t["z"]), ptr(t["sdf"]), ptr(t["rgb"])] + ([ptr(t["grad"])] if with_grad else []) + \
               [ptr(t["voxels"]), C.RES, self.R, self.S]


def k_forward(dc):
    from nicer_slam_amd._native import lib, check
    R, S = dc.R, dc.S
    out = dict(weights=nan(R, S), rgb_values=nan(R, 3), depth=nan(R), nmap=nan(R, 3), entropy=nan(R))
    check(lib.nsa_composite_forward(*dc.head(), *[ptr(out[k]) for k in O.COMPOSITE_OUT], st()))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def k_backward(dc, cot):
    """cot: {name: fp32 CPU tensor}; absent = NULL"""
    from nicer_slam_amd._native import lib, check
    R, S = dc.R, dc.S
    d = {k: dev(cot.get(k)) for k in C.COTANGENTS}
    g = [nan(R, S), nan(R, S, 3), nan(R, S, 3)]
    check(lib.nsa_composite_backward(*dc.head(), *[ptr(d[k]) for k in C.COTANGENTS], *[ptr(t) for t in g], st()))
    torch.cuda.synchronize()
    return [t.cpu() for t in g]


def k_track(dc, gt, n_total):
    from nicer_slam_amd._native import lib, check
    R, S = dc.R, dc.S
    gtd = dev(gt)
    rgbv, loss, g = nan(R, 3), nan(R), [nan(R, S), nan(R, S, 3), nan(R, S, 3)]
    check(lib.nsa_composite_track(*dc.head(with_grad=False), ptr(gtd), n_total, ptr(rgbv), ptr(loss), *[ptr(t) for t in g], st()))
    torch.cuda.synchronize()
    return rgbv.cpu(), loss.cpu(), [t.cpu() for t in g]


def _composite_rows(case, pool, tag=""):
    """one case against float64: the five forward outputs, the three gradients for each cotangent alone and all together, and the
    tracking chain; rows go to ``pool``.  -> share of rays left out of depth"""
    R, S = case["R"], case["S"]
    args = C.composite_args(case)
    dc = DevCase(case)
    o64, o32 = O.composite(*args), O.composite(*args, dtype=F32)
    left = o64.weights.detach().sum(1) < C.SUM_W_MIN
    grp = case["group"]
    assert not bool((left & (grp != 3)).any()), "a ray of groups 1-3 is left out of depth"
    share, cap = float(left.double().mean()), float((grp == 3).double().mean())
    assert share <= cap, f"R = {R} S = {S}: {share:.3f} of the rays left out of depth, group 4 is {cap:.3f}"
    out = k_forward(dc)
    for k in O.COMPOSITE_OUT:
        assert bool(torch.isfinite(out[k]).all()), k
        pool.add(f"{tag}forward: {k}", out[k], getattr(o64, k), getattr(o32, k), fwd_norm(getattr(o64, k)), ~left if k == "depth" else None)
    c, cot = C.composite_cotangents(case, seed=200 + S)
    zero_grad = torch.zeros(R, dtype=torch.bool)
    zero_grad[case["zero_grad_rays"]] = True
    for name in C.COTANGENTS + ("all",):
        kw = dict(cot) if name == "all" else {name: cot[name]}
        keep = None
        if name == "g_depth":
            keep = ~left
        elif name == "all":                       # (all together: the ill-conditioned quotient is pulled back on the kept rays only)
            kw["g_depth"] = torch.where(left, torch.zeros_like(kw["g_depth"]), kw["g_depth"])
        got = k_backward(dc, kw)
        g64, g32 = O.composite_backward(o64, **kw), O.composite_backward(o32, **kw)
        assert bool((g64[0][:, -1] == 0).all())
        assert bool((got[0][:, -1] == 0).all()), f"R = {R} S = {S} {name}: the last sample's g_sdf is not exactly 0"
        for what, a, b, y in zip(("g_sdf", "g_rgb", "g_grad"), got, g64, g32):
            assert bool(torch.isfinite(a).all()), (name, what)
            k_ = torch.ones(R, dtype=torch.bool) if keep is None else keep
            if what == "g_grad" and "g_nmap" in kw:  # (a zero grad row has the derivative w g_nmap / 1e-6: its ray in a line of its own,
                ko = O.composite_g_grad_kernel_order(o32.weights, case["grad"], kw["g_nmap"])                          # not over the others)
                pool.add(f"{tag}backward of {name}: {what}, rays with a zero grad row", a, b, y, c, k_ & zero_grad, kernel_order=ko)
                k_ = k_ & ~zero_grad
            pool.add(f"{tag}backward of {name}: {what}", a, b, y, c, k_)
    # the tracking chain: forward -> L1 over 3 n_total scalars -> backward of that cotangent
    n_total = 2 * R + 3
    gt = C.track_gt(case, seed=300 + S)
    rgbv, ray_loss, g = k_track(dc, gt, n_total)
    a = args
    r64 = O.composite_track(a[0], a[1], a[2], *a[4:], gt, n_total)
    r32 = O.composite_track(a[0], a[1], a[2], *a[4:], gt, n_total, dtype=F32)
    keep = r64[3] >= C.KINK
    pool.add(f"{tag}track: rgb_values", rgbv, r64[0], r32[0], fwd_norm(r64[0]))
    pool.add(f"{tag}track: ray_loss", ray_loss, r64[1], r32[1], fwd_norm(r64[1]))
    inv = torch.full((R,), 1.0 / (3 * n_total), dtype=torch.float64)
    for what, x, b, y in zip(("g_sdf", "g_rgb", "g_grad"), g, r64[2], r32[2]):
        assert bool(torch.isfinite(x).all())
        pool.add(f"{tag}track: {what}", x, b, y, inv, keep)
    assert bool((g[2] == 0).all()) and bool((g[0][:, -1] == 0).all())
    return share, int((~keep).sum())


def test_composite_small_ray_counts_at_every_lane_ownership_vs_float64(capsys):
    """R = 1, 3, 5 at S = 1 ... 256 (both sides of 64 / 65, 128 / 129, 192 / 193), every ray carrying an edge; rows pooled"""
    fails, pool, kinks, rays = [], Pool(), 0, 0
    for S in C.COMPOSITE_S:
        for R in C.COMPOSITE_R_SMALL:
            _share, k = _composite_rows(C.composite_case(R, S, seed=100 + S), pool)
            kinks, rays = kinks + k, rays + R
    with capsys.disabled():
        print(f"\n  composite, R = 1, 3, 5 x S = {C.COMPOSITE_S} pooled ({rays} rays); tracking-L1 kink rays left out: {kinks}")
        pool.judge("small R: ", fails)
    assert kinks <= rays // 100 + 1
    assert not fails, [f["what"] for f in fails]


@pytest.mark.parametrize("S", C.COMPOSITE_S_BIG)
def test_composite_1027_rays_vs_float64(S, capsys):
    fails, pool = [], Pool()
    share, kinks = _composite_rows(C.composite_case(C.COMPOSITE_R_BIG, S, seed=100 + S), pool)
    with capsys.disabled():
        print(f"\n  composite, R = {C.COMPOSITE_R_BIG} S = {S}: left out of depth {share:.3f} of the rays (group 4: 0.25), "
              f"tracking-L1 kink rays left out: {kinks}")
        pool.judge(f"S {S}: ", fails)
    assert kinks < C.COMPOSITE_R_BIG // 100
    assert not fails, [f["what"] for f in fails]


def _all_outputs(case, cot, gt, n_total):
    dc = DevCase(case)
    out = k_forward(dc)
    res = [out[k] for k in O.COMPOSITE_OUT] + k_backward(dc, cot)
    rgbv, loss, g = k_track(dc, gt, n_total)
    return res + [rgbv, loss] + g


def _take(case, idx):
    out = dict(case)
    for k in ("rays_o", "rays_d", "z", "sdf", "rgb", "grad"):
        out[k] = case[k][idx].contiguous()
    out["R"] = len(idx)
    return out


def test_composite_rays_are_independent_bit_for_bit():
    """needs no reference: a permutation of the rays permutes every output; changing the other rays, or R, changes no bit of a ray"""
    S, R = 129, 203
    case = C.composite_case(R, S, seed=5)
    _c, cot = C.composite_cotangents(case, seed=6)
    gt = C.track_gt(case, seed=7)
    base = _all_outputs(case, cot, gt, 1000)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(8))
    moved = _all_outputs(_take(case, perm), {k: v[perm].contiguous() for k, v in cot.items()}, gt[perm].contiguous(), 1000)
    for a, b in zip(base, moved):
        assert torch.equal(a[perm], b)
    # the first 37 rays alone (R changes, the waves of a workgroup are filled differently), then among OTHER rays
    head = torch.arange(37)
    alone = _all_outputs(_take(case, head), {k: v[:37].contiguous() for k, v in cot.items()}, gt[:37].contiguous(), 1000)
    other = C.composite_case(R, S, seed=9)
    _c2, cot2 = C.composite_cotangents(other, seed=10)
    mixed, cotm, gtm = dict(other, voxels=case["voxels"]), {k: v.clone() for k, v in cot2.items()}, C.track_gt(other, seed=11)
    for k in ("rays_o", "rays_d", "z", "sdf", "rgb", "grad"):
        mixed[k] = other[k].clone()
        mixed[k][:37] = case[k][:37]
    for k in cotm:
        cotm[k][:37] = cot[k][:37]
    gtm[:37] = gt[:37]
    among = _all_outputs(mixed, cotm, gtm, 1000)
    for a, b, c_ in zip(base, alone, among):
        assert torch.equal(a[:37], b) and torch.equal(a[:37], c_[:37])


# ------------------------------------------------------------------------------------------------------------------ rays and pose
def k_cam_to_pose(cam):
    from nicer_slam_amd._native import lib, check
    b = cam.shape[0]
    camd, pose = dev(cam), nan(b, 4, 4)
    check(lib.nsa_cam_to_pose(ptr(camd), b, ptr(pose), st()))
    torch.cuda.synchronize()
    return pose.cpu()


def k_rays_forward(uv, pose, K):
    from nicer_slam_amd._native import lib, check
    b, n = uv.shape[:2]
    u, p, k = dev(uv), dev(pose), dev(K)
    o, d, ds = nan(b * n, 3), nan(b * n, 3), nan(b * n)
    check(lib.nsa_rays_forward(ptr(u), ptr(p), ptr(k), b, n, ptr(o), ptr(d), ptr(ds), st()))
    torch.cuda.synchronize()
    return o.cpu(), d.cpu(), ds.cpu()


def k_rays_pose_backward(uv, pose, K, g_o, g_d):
    from nicer_slam_amd._native import lib, check
    b, n = uv.shape[:2]
    u, p, k, go, gd = (dev(t) for t in (uv, pose, K, g_o, g_d))
    gp = nan(b, 4, 4)
    check(lib.nsa_rays_pose_backward(ptr(u), ptr(p), ptr(k), b, n, ptr(go), ptr(gd), ptr(gp), st()))
    torch.cuda.synchronize()
    return gp.cpu()


def k_pose_grad_to_cam(cam, g_pose):
    from nicer_slam_amd._native import lib, check
    b = cam.shape[0]
    c, g = dev(cam), dev(g_pose)
    out = nan(b, 7)
    check(lib.nsa_pose_grad_to_cam(ptr(c), ptr(g), b, ptr(out), st()))
    torch.cuda.synchronize()
    return out.cpu()


def k_track_head(uv1, K1, cam1):
    from nicer_slam_amd._native import lib, check
    n = uv1.shape[0]
    u, k, c = dev(uv1), dev(K1), dev(cam1)
    pose, o, d, ds = nan(4, 4), nan(n, 3), nan(n, 3), nan(n)
    check(lib.nsa_track_head(ptr(u), ptr(k), ptr(c), n, ptr(pose), ptr(o), ptr(d), ptr(ds), st()))
    torch.cuda.synchronize()
    return pose.cpu(), o.cpu(), d.cpu(), ds.cpu()


def test_rays_and_pose_chain_vs_float64(capsys):
    """Every kernel of the camera chain on the fp32 inputs it is given (cam -> pose -> rays; g_rays -> g_pose -> g_cam), and the whole
    chain's g_cam against float64 autograd from the 7-vector.  Per ray: rays_d, depth_scale (rays_o exact); per image, pooled over the
    cases: pose, g_pose, g_cam divided by the largest c_r of the image; an image whose rays all have zero cotangents gets an exactly
    zero g_pose block, bottom row included."""
    fails, per_ray, per_image = [], Pool(), Pool()
    for b in C.RAYS_B:
        for n in C.RAYS_N:
            cs = C.rays_case(b, n, seed=b + n)
            uv, cam, K, g_o, g_d = cs["uv"], cs["cam"], cs["K"], cs["g_o"], cs["g_d"]
            cmax = cs["c"].reshape(b, n).amax(1)
            # cam -> pose
            pose = k_cam_to_pose(cam)
            p64, p32 = O.camera_from_tensor(cam.double()), O.camera_from_tensor(cam)
            per_image.add("cam_to_pose: pose", pose, p64, p32, fwd_norm(p64))
            # pose (the kernel's, fp32) -> rays
            o, d, ds = k_rays_forward(uv, pose, K)
            r64, r32 = O.rays(uv, pose, K), O.rays(uv, pose, K, dtype=F32)
            assert torch.equal(o.reshape(b, n, 3), pose[:, None, :3, 3].expand(-1, n, -1)), "rays_o is not the pose's translation"
            d64, d32 = r64.rays_d.detach().reshape(-1, 3), r32.rays_d.detach().reshape(-1, 3)
            per_ray.add("rays_forward: rays_d", d, d64, d32, fwd_norm(d64))
            s64, s32 = r64.depth_scale.detach().reshape(-1), r32.depth_scale.detach().reshape(-1)
            per_ray.add("rays_forward: depth_scale", ds, s64, s32, fwd_norm(s64))
            # g_rays -> g_pose at that pose
            gp = k_rays_pose_backward(uv, pose, K, g_o, g_d)
            assert bool(torch.isfinite(gp).all())
            gp64, gp32 = O.rays_pose_backward(r64, g_o, g_d), O.rays_pose_backward(r32, g_o, g_d)
            assert bool((gp[:, 3] == 0).all()), "g_pose: bottom row"
            per_image.add("rays_pose_backward: g_pose", gp, gp64, gp32, cmax)
            # g_pose (the kernel's) -> g_cam
            gc = k_pose_grad_to_cam(cam, gp)
            gc64, gc32 = O.pose_grad_to_cam(cam, gp), O.pose_grad_to_cam(cam, gp, dtype=F32)
            per_image.add("pose_grad_to_cam: g_cam", gc, gc64, gc32, cmax)
            # the chain from the 7-vector
            c64, c32 = O.rays(uv, cam, K), O.rays(uv, cam, K, dtype=F32)
            per_image.add("chain: g_cam", gc, O.rays_pose_backward(c64, g_o, g_d), O.rays_pose_backward(c32, g_o, g_d), cmax)
            # the tracker's fused head, image by image (pose and rays from the 7-vector in one launch)
            for i in range(b):
                hp, ho, hd, hs = k_track_head(uv[i], K[i], cam[i])
                assert torch.equal(ho, cam[i, 4:].expand(n, 3)), "track_head: rays_o is not the camera's translation"
                per_image.add("track_head: pose", hp[None], p64[i:i + 1], p32[i:i + 1], fwd_norm(p64[i:i + 1]))
                per_ray.add("track_head: rays_d", hd, c64.rays_d.detach()[i], c32.rays_d.detach()[i], fwd_norm(c64.rays_d.detach()[i]))
                per_ray.add("track_head: depth_scale", hs, c64.depth_scale.detach()[i], c32.depth_scale.detach()[i],
                            fwd_norm(c64.depth_scale.detach()[i]))
    with capsys.disabled():
        print(f"\n  rays and pose, b = {C.RAYS_B} x n = {C.RAYS_N} pooled")
        per_ray.judge("", fails)
        per_image.judge("", fails)
    assert not fails, [f["what"] for f in fails]


@pytest.mark.parametrize("S", [1, 64, 65, 160, 256])
def test_rays_backward_vs_float64(S, capsys):
    from nicer_slam_amd._native import lib, check
    fails = []
    R = 1027
    cs = C.rays_backward_case(R, S, seed=S)
    with capsys.disabled():
        print()
        for with_dir in (True, False):
            z, gx, gdir = dev(cs["z"]), dev(cs["g_x"]), dev(cs["g_dir"]) if with_dir else None
            go, gd = nan(R, 3), nan(R, 3)
            check(lib.nsa_rays_backward(ptr(z), ptr(gx), ptr(gdir), R, S, ptr(go), ptr(gd), st()))
            torch.cuda.synchronize()
            a64 = O.rays_backward(cs["z"], cs["g_x"], cs["g_dir"] if with_dir else None)
            a32 = O.rays_backward(cs["z"], cs["g_x"], cs["g_dir"] if with_dir else None, dtype=F32)
            for what, got, b, y in zip(("g_rays_o", "g_rays_d"), (go.cpu(), gd.cpu()), a64, a32):
                gate(f"rays_backward S {S} g_dir {int(with_dir)}: {what}", got, b, y, cs["c"], failures=fails)
    assert not fails, [f["what"] for f in fails]


def test_l1_loss_vs_float64(capsys):
    from nicer_slam_amd._native import lib, check
    fails, loss_rows, grad_rows = [], Pool(), Pool()
    for n in C.L1_N:
        for seed in range(8):
            pred, target = C.l1_case(n, seed)
            p, t, loss, g = dev(pred), dev(target), nan(1), nan(n)
            check(lib.nsa_l1_loss(ptr(p), ptr(t), n, ptr(loss), ptr(g), st()))
            torch.cuda.synchronize()
            l64, g64 = O.l1(pred, target)
            l32, g32 = O.l1(pred, target, dtype=F32)
            assert bool((g.cpu()[::7] == 0).all()), "an exact tie has a non-zero gradient"
            loss_rows.add("l1_loss: loss", loss.cpu(), l64.reshape(1), l32.reshape(1), torch.ones(1, dtype=torch.float64))
            grad_rows.add("l1_loss: g_pred", g.cpu(), g64, g32, torch.full((n,), 1.0 / n, dtype=torch.float64))
    with capsys.disabled():
        print(f"\n  nsa_l1_loss, n = {C.L1_N} x 8 seeds pooled")
        loss_rows.judge("", fails)
        grad_rows.judge("", fails)
    assert not fails, [f["what"] for f in fails]


# ------------------------------------------------------------------------------------------------------------------ loss
def _guarded(t):
    """the tensor on the device with 16 NaNs behind it (and the workspace likewise): a neighbour read that runs past the last ray of
    the last image stays inside the allocation and poisons what it feeds"""
    buf = torch.full((t.numel() + 16,), NAN, device="cuda")
    buf[:t.numel()] = t.detach().reshape(-1).to("cuda", torch.float32)
    return buf[:t.numel()].view(t.shape)


def k_slam_loss(out, gt, weights, whole, shape):
    from nicer_slam_amd._native import lib, check, LossDesc
    bs, n, S, E = shape
    R = bs * n
    d = {k: _guarded(out[k]) for k in ("rgb_values", "depth_values", "normal_map", "sdf")}
    gth = dev(out["grad_theta"]) if E else None
    gnei = dev(out["grad_theta_nei"]) if (E and out["grad_theta_nei"] is not None) else None
    g = {k: _guarded(gt[k]) for k in ("rgb", "depth", "gt_depth", "gt_depth_mask", "mask", "normal")}
    res = dict(rgb_values=nan(R, 3), depth_values=nan(R), normal_map=nan(R, 3), grad_theta=nan(E, 3) if E else None,
               grad_theta_nei=nan(E, 3) if gnei is not None else None)
    terms = nan(8)
    ws = torch.full(((int(lib.nsa_slam_loss_workspace(bs, n, E)) + 1) // 2 + 8,), NAN, device="cuda", dtype=torch.float64)
    desc = LossDesc(bs, n, S, E, ptr(d["rgb_values"]), ptr(g["rgb"]), ptr(d["depth_values"]), ptr(g["depth"]), ptr(g["gt_depth"]),
                    ptr(g["gt_depth_mask"]), ptr(g["mask"]), ptr(d["sdf"]), ptr(d["normal_map"]), ptr(g["normal"]), ptr(gth), ptr(gnei),
                    *[float(w) for w in weights], int(bool(whole)),
                    *[ptr(res[k]) for k in O.LOSS_LEAVES], ptr(terms))
    check(lib.nsa_slam_loss(ctypes.byref(desc), ws.data_ptr(), st()))
    torch.cuda.synchronize()
    return terms.cpu(), {k: (None if v is None else v.cpu()) for k, v in res.items()}


def test_slam_loss_vs_float64(capsys):
    """The eight terms (each divided by max(|float64|, 1); pooled over the cases) and every gradient per ray / per eikonal point,
    divided by the natural size 1 / R resp. 1 / E of a mean's gradient so that shapes can share a pool.  Rays on a kink of the
    regulariser (sign of a residual difference) or of the normal L1 (sign of p - g) are left out on both sides, counted and capped at
    1 %.  The image of `near_singular` whose masked depths are constant to 1e-6 is NOT gated: its 2x2 system has a
    determinant five orders below fp32's rounding of a00 a11, so (scale, shift) and everything multiplied by them is rounding noise
    in ANY fp32 evaluation of the reference's formula, and a ratio of two such noises says nothing.  What is asserted of it: every
    output is finite, and the other images of the batch and the other terms stay in the gated pools; its depth terms and its
    d/d depth_values are printed without a verdict.  The kink cap is applied to the other rays of that case."""
    fails, terms_pool, pools = [], Pool(), {}
    with capsys.disabled():
        print()
        for shape, variant in C.loss_cases():
            bs, n, S, E = shape
            R = bs * n
            out, gt, w, whole = C.loss_case(shape, variant, seed=7)
            terms, g = k_slam_loss(out, gt, w, whole, shape)
            r64, r32 = O.slam_terms(out, gt, w, whole), O.slam_terms(out, gt, w, whole, dtype=F32)
            dk, nk = C.loss_kinks(r64.aux, shape)
            near = torch.zeros(R, dtype=torch.bool)
            if variant == "near_singular":
                near[:n] = True
            share_d, share_n = float((dk & ~near).double().mean()), float(nk.double().mean())
            print(f"  loss {shape} {variant}: depth-kink rays {share_d:.4f} (+ {int((dk & near).sum())} in the near-singular image), "
                  f"normal-kink rays {share_n:.4f}")
            assert share_d < 0.01 and share_n < 0.01, (shape, variant, share_d, share_n)
            t64, t32 = torch.cat([r64.terms, r64.total.reshape(1)]), torch.cat([r32.terms, r32.total.reshape(1)])
            depth_terms = torch.tensor([0, 0, 0, 1, 0, 0, 0, 1], dtype=torch.bool)
            assert bool(torch.isfinite(terms).all()), (shape, variant, terms)
            sel = ~depth_terms if variant == "near_singular" else torch.ones(8, dtype=torch.bool)
            terms_pool.add("terms", terms.reshape(8, 1), t64.reshape(8, 1), t32.reshape(8, 1), t64.abs().clamp_min(1.0), sel)
            if variant == "near_singular":
                report(f"slam_loss {shape}: depth terms of a near-singular fit", terms.reshape(8, 1), t64.reshape(8, 1), t32.reshape(8, 1),
                       t64.abs().clamp_min(1.0), depth_terms)
            pool = pools.setdefault("small" if R < 1000 else str(shape), Pool())
            ray_norm, pt_norm = torch.full((R,), 1.0 / R, dtype=torch.float64), torch.full((max(E, 1),), 1.0 / max(E, 1), dtype=torch.float64)
            zero_n = r64.aux["fg"].reshape(-1) & (out["normal_map"].reshape(R, 3).abs().amax(-1) == 0)
            for k, keep in (("rgb_values", None), ("depth_values", ~dk & ~near), ("normal_map", ~nk & ~zero_n)):
                assert bool(torch.isfinite(g[k]).all()), (shape, variant, k)
                pool.add("d/d " + k, g[k], r64.grads[k].reshape(R, -1), r32.grads[k].reshape(R, -1), ray_norm, keep)
            ko = O.loss_grads_kernel_order(out, gt, w)
            if bool(zero_n.any()):                    # (derivative u / 1e-12: a line of its own, not over the other rays)
                pool.add("d/d normal_map, zero rows under a set mask", g["normal_map"], r64.grads["normal_map"].reshape(R, -1),
                         r32.grads["normal_map"].reshape(R, -1), ray_norm, zero_n & ~nk, kernel_order=ko["normal_map"])
            if bool(near.any()):
                report(f"slam_loss {shape}: d/d depth_values of a near-singular fit", g["depth_values"],
                       r64.grads["depth_values"].reshape(R, -1), r32.grads["depth_values"].reshape(R, -1), ray_norm, near & ~dk)
            for k in ("grad_theta", "grad_theta_nei"):
                if g[k] is None:
                    assert k == "grad_theta_nei" or E == 0
                    continue
                assert bool(torch.isfinite(g[k]).all()), (shape, variant, k)
                zero_p = out["grad_theta"].abs().amax(-1) == 0     # (|g| = 0: derivative q / 1e-5, a line of its own)
                pool.add("d/d " + k, g[k], r64.grads[k], r32.grads[k], pt_norm[:E], ~zero_p)
                if bool(zero_p.any()):
                    pool.add("d/d " + k + ", zero grad_theta rows", g[k], r64.grads[k], r32.grads[k], pt_norm[:E], zero_p, kernel_order=ko[k])
            if variant == "no_foreground":
                assert float(terms[3]) == 0.0 and bool((g["depth_values"] == 0).all())
        terms_pool.judge("slam_loss: ", fails)
        for name, pool in pools.items():
            pool.judge(f"slam_loss {name}: ", fails)
    assert not fails, [f["what"] for f in fails]
