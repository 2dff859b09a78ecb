"""The SSIM form of the patch-warp term on the MI355X (C ABI section 5 nsa_patch_ssim, csrc/patch_ssim.hip, fused/warp.py::patch_ssim;
DESIGN 4e): the kernel against the float64 oracle (tests/patch_ssim_ref.py) and beside pytorch_msssim's conv2d form evaluated in
fp32 on the device, its reproducibility, SLAMLoss(warp_loss_type="ssim") on both engines behind one HIP patch warp, and a mapping
forward of SLAMNetwork with that loss on the fused engine."""
import math
from types import SimpleNamespace

import pytest
import torch

import patch_ssim_ref as R
from helpers import load, tt, draws_of
from test_model_cpu import build_model

pytestmark = pytest.mark.gpu

# csrc/patch_ssim.hip: 16 patches per workgroup, at most 1024 workgroups; one patch more and the workgroups stride
COVERED = 1024 * 16


def _inputs(n, p, seed, first=0):
    """fp32 [n, p^2, 3] pairs and a mask whose patches cycle through eight kinds (patch index + first, modulo 8):
    0 fully valid with values at exactly 0 and 1; 1 flat (constant) pair; 2 nearly flat pair (sigma^2 cancels); 3 identical pair;
    4 wholly masked; 5 about 80 % valid with values at 0 and 1; 6, 7 about 80 % valid."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, p * p, 3, generator=g)
    y = (x + 0.1 * torch.randn(n, p * p, 3, generator=g)).clamp(0, 1)
    m = torch.rand(n, p * p, generator=g) > 0.2
    kind = (torch.arange(n) + first) % 8
    lo, hi = torch.rand(n, p * p, 3, generator=g) < 0.1, torch.rand(n, p * p, 3, generator=g) > 0.9
    ends = ((kind == 0) | (kind == 5))[:, None, None]
    x = torch.where(ends & lo, torch.zeros_like(x), torch.where(ends & hi, torch.ones_like(x), x))
    y = torch.where(ends & hi, torch.zeros_like(y), torch.where(ends & lo, torch.ones_like(y), y))
    level = torch.rand(n, 1, 3, generator=g)
    flat, near = (kind == 1)[:, None, None], (kind == 2)[:, None, None]
    x = torch.where(flat, level.expand_as(x), torch.where(near, level + 1e-3 * x, x))
    y = torch.where(flat, (level - 0.01).expand_as(y), torch.where(near, level + 1e-3 * y, y))
    y = torch.where((kind == 3)[:, None, None], x, y)
    m = torch.where((kind <= 3)[:, None], torch.ones_like(m), m)
    m = torch.where((kind == 4)[:, None], torch.zeros_like(m), m)
    return x.contiguous(), y.contiguous(), m.contiguous()


def _kernel(x, y, m, p, grad=True):
    from nicer_slam_amd.fused.warp import patch_ssim
    xd = x.cuda().requires_grad_(grad)
    loss = patch_ssim(xd, y.cuda(), None if m is None else m.cuda(), p)
    if not grad:
        return loss.detach(), None
    loss.backward()
    return loss.detach(), xd.grad


def _check_against_float64(x, y, m, p, tag):
    loss, grad = _kernel(x, y, m, p)
    ref_loss, _, ref_grad = R.direct(x, y, m, p)
    got = grad.double().cpu()
    gmax = float(ref_grad.abs().max())
    assert abs(float(loss) - ref_loss) <= R.ulp32(ref_loss), (tag, float(loss), ref_loss)
    bound = 2.0 ** -23 * ref_grad.abs() + 1e-9 * gmax
    assert bool(((got - ref_grad).abs() <= bound).all()), (tag, float((got - ref_grad).abs().max()), gmax)
    if m is not None and not bool(m.all()):
        assert float(got[~m].abs().max()) == 0.0, tag
    # pytorch_msssim's shape in fp32 on the same device: context, and the bar the kernel has to clear
    loss32, grad32 = R.conv_form(x, y, m, p, dtype=torch.float32, device="cuda")
    e_k, e_32 = (got - ref_grad).abs(), (grad32.double().cpu() - ref_grad).abs()
    rms = lambda e: float(e.pow(2).mean().sqrt())
    print(f"{tag}: loss {ref_loss:.6e} |kernel - f64| {abs(float(loss) - ref_loss):.2e} |fp32 conv2d - f64| {abs(float(loss32) - ref_loss):.2e}; "
          f"gradient (max |g| {gmax:.2e}) kernel max {float(e_k.max()):.2e} rms {rms(e_k):.2e}, fp32 conv2d max {float(e_32.max()):.2e} "
          f"rms {rms(e_32):.2e}")
    assert float(e_k.max()) <= float(e_32.max()) and rms(e_k) <= rms(e_32), tag
    assert abs(float(loss) - ref_loss) <= abs(float(loss32) - ref_loss), tag


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, COVERED + 1])
@pytest.mark.parametrize("p", [3, 5, 11])
def test_kernel_against_float64(p, n):
    if n < 8:                          # too few patches to hold every kind at once: one run per kind
        for first in range(8):
            x, y, m = _inputs(n, p, 100 * p + first, first)
            if first in (3, 4):        # identical / wholly masked alone: exactly 0, gradient exactly 0 where masked
                loss, grad = _kernel(x, y, m, p)
                assert float(loss) == 0.0 and (first == 3 or float(grad.abs().max()) == 0.0)
                continue
            _check_against_float64(x, y, m, p, f"p {p} n {n} kind {first}")
        return
    x, y, m = _inputs(n, p, 7 * p + n)
    _check_against_float64(x, y, m, p, f"p {p} n {n}")


@pytest.mark.parametrize("p", [3, 5, 7, 9, 11])
def test_exact_cases_every_patch_size(p):
    from nicer_slam_amd.fused.warp import patch_ssim
    x, y, m = _inputs(40, p, p)
    loss, grad = _kernel(x, x.clone(), m, p)
    assert float(loss) == 0.0                                              # scored against itself: SSIM exactly 1 everywhere
    loss, grad = _kernel(x, y, torch.zeros_like(m), p)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0          # all masked
    loss, grad = _kernel(x, y, None, p)                                    # no mask = all valid
    ref_loss, _, ref_grad = R.direct(x, y, None, p)
    assert abs(float(loss) - ref_loss) <= R.ulp32(ref_loss)
    assert bool(((grad.double().cpu() - ref_grad).abs() <= 2.0 ** -23 * ref_grad.abs() + 1e-9 * float(ref_grad.abs().max())).all())
    empty = torch.empty(0, p * p, 3, device="cuda")
    assert math.isnan(float(patch_ssim(empty, empty, torch.empty(0, p * p, dtype=torch.bool, device="cuda"), p)))


def test_reproducible_and_independent_of_the_patch_order():
    from nicer_slam_amd.fused.warp import patch_ssim
    for p, n in ((3, 1000), (5, 257), (11, 130)):
        x, y, m = _inputs(n, p, 11 + p)
        loss, grad = _kernel(x, y, m, p)
        again, grad2 = _kernel(x, y, m, p)
        assert torch.equal(loss, again) and torch.equal(grad, grad2)
        assert torch.equal(_kernel(x, y, m, p, grad=False)[0], loss)       # g_pred = NULL: the same loss
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(p))
        _, grad_p = _kernel(x[perm], y[perm], m[perm], p)
        assert torch.equal(grad_p, grad[perm.cuda()])
        # leading dimensions, a non-contiguous view and a uint8 mask change nothing
        xv = x.cuda().reshape(n, p * p, 3).transpose(0, 1).contiguous().transpose(0, 1)
        assert not xv.is_contiguous() or n == 1
        lv = patch_ssim(xv.reshape(1, n, p * p, 3), y.cuda().reshape(1, n, p * p, 3), m.cuda().to(torch.uint8).reshape(1, n, p * p), p)
        assert torch.equal(lv, loss)
        # the inputs are left alone
        xd, yd = x.cuda(), y.cuda()
        patch_ssim(xd, yd, m.cuda(), p)
        assert torch.equal(xd.cpu(), x) and torch.equal(yd.cpu(), y)


def test_both_engines_behind_one_patch_warp():
    """One HIP patch warp at 680 x 1200 (patches 1 / 5 / 11, 4 keyframes x 300 pixels, bundle adjustment); the SSIM warp loss on
    the same warp_output by the torch restatement and by the kernel, both backpropagated through the same HIP warp backward."""
    from nicer_slam_amd.fused import warp as fw
    from nicer_slam_amd.model.loss import SLAMLoss
    from nicer_slam_amd.utils.general import get_camera_from_tensor
    from test_warp_gpu import _random_batch
    bs, n = 4, 300
    uv, K, cam, rgb, dep, depth0 = _random_batch(bs, n, 3)
    model = SimpleNamespace(H=680, W=1200, patchsizes=[1, 5, 11])
    cam_l = cam.clone().requires_grad_(True)
    depth = depth0.clone().requires_grad_(True)
    wo = fw.patch_warp(model, uv, get_camera_from_tensor(cam_l), K, depth, {"full_rgb": rgb, "full_depth": dep}, bs)
    crit = SLAMLoss("torch.nn.L1Loss", 0.0, warp_loss_type="ssim")
    res = {}
    for engine in ("torch", "auto"):
        crit.engine = engine
        total = crit._warp_loss(wo)
        parts = {ps: crit._warp_loss({ps: wo[ps]}).item() for ps in (5, 11)}
        depth.grad = cam_l.grad = None
        total.backward(retain_graph=True)
        res[engine] = (total.item(), parts, depth.grad.clone(), cam_l.grad.clone())
    for ps in (5, 11):
        gt, samp, mask, _ = wo[ps]
        want = R.term(samp.detach().cpu(), gt.cpu(), mask.cpu(), ps)
        t, a = res["torch"][1][ps], res["auto"][1][ps]
        print(f"patch {ps}: float64 term {want:.9e}  torch engine {t:.9e}  kernel {a:.9e}  valid {float(mask.float().mean()):.3f}")
        assert want > 1e-4                                                  # the term is live on these frames
        assert abs(t - want) <= 2 * R.ulp32(want) and abs(a - want) <= 2 * R.ulp32(want) and abs(a - t) <= 2 * R.ulp32(want)
    # the totals add the fp32 L1 mean of the one-pixel patches (torch: an fp32 sum of ~14 000 values) to the two terms
    assert abs(res["auto"][0] - res["torch"][0]) <= 1e-6 * res["torch"][0]
    for k, name in ((2, "depth"), (3, "camera")):
        g_t, g_a = res["torch"][k], res["auto"][k]
        gmax = float(g_t.abs().max())
        print(f"{name} gradient: max |kernel - torch engine| {float((g_a - g_t).abs().max()):.3e} of max {gmax:.3e}")
        assert gmax > 0 and bool(torch.isfinite(g_a).all())
        assert float((g_a - g_t).abs().max()) <= 1e-5 * gmax, name


def _mapping(fx, engine, gt):
    from nicer_slam_amd.utils.general import camera_from_tensor_torch as get_camera_from_tensor
    model = build_model(fx)
    # the geometric initialisation zeroes the first-layer columns that the grid features feed, so a freshly built SDF network sends
    # nothing to its tables; noise on weight_v, as in the reference goldens' "_rw" cases, makes that path live
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.startswith("implicit_network") and n.endswith("weight_v"):
                p.add_((0.05 if ".lin0." in n else 0.01) * torch.randn(p.shape, generator=g))
    model = model.cuda()
    model.freeze_fine_mlp()
    model.engine = engine
    model.mapping_patchsizes = [1, 5, 11]
    model.train(True)
    model.voxels = tt(fx["in_voxels"]).cuda()
    model.draws = draws_of(fx, "cuda")
    model.draws["z_vals_override"] = tt(fx["out_z_vals"]).cuda()
    cam = tt(fx["in_cam"]).cuda().requires_grad_(True)
    pose = get_camera_from_tensor(cam)
    out = model({"intrinsics": tt(fx["in_K"]).cuda(), "uv": tt(fx["in_uv"]).cuda(), "pose": pose},
                torch.arange(pose.shape[0], device="cuda"), gt, mode="mapping", stage=str(fx["meta_stage"]),
                color_stage=str(fx["meta_color_stage"]), frame_idx=1)
    return model, cam, out


def test_mapping_forward_with_the_ssim_warp_loss():
    """mode="mapping" with mapping_patchsizes = [1, 5, 11], SLAMLoss(warp_loss_type="ssim"), warp_loss_weight = 0.5 on the fused
    engine: finite loss, live gradients into the warp (the depth), the poses and the tables, and the loss of the composed engine on
    the same draws at the tolerance test_mapping_gpu.py::test_fused_mapping_with_warp_block applies (1e-5)."""
    from nicer_slam_amd.model.loss import SLAMLoss
    fx = load("full_mapping_warp")
    gt = {"full_rgb": tt(fx["in_full_rgb"]).cuda(), "full_depth": tt(fx["in_full_depth"]).cuda()}
    crit = SLAMLoss("torch.nn.L1Loss", 0.0, warp_loss_type="ssim", warp_loss_weight=0.5)
    tables = ("implicit_network.coarse.encoding.embeddings", "implicit_network.fine.encoding.embeddings",
              "rendering_network.encoding.embeddings")
    losses = {}
    for engine in ("fused", "composed"):
        model, cam, out = _mapping(fx, engine, gt)
        assert model.last_engine == engine and sorted(out["warp_output"]) == [1, 5, 11]
        warp = crit.warp_loss_weight * crit._warp_loss(out["warp_output"])
        loss = (out["rgb_values"].reshape(-1, 3) - tt(fx["gt_rgb"]).cuda()).abs().mean() + warp
        assert math.isfinite(loss.item()) and warp.item() > 0
        losses[engine] = loss.item()
        if engine != "fused":
            continue
        named = dict(model.named_parameters())
        seen = {}
        for ps in (5, 11):                                  # what the SSIM terms send back into the HIP warp backward (-> depth)
            out["warp_output"][ps][1].register_hook(lambda g, ps=ps: seen.__setitem__(ps, g))
        loss.backward()
        for ps in (5, 11):
            assert bool(torch.isfinite(seen[ps]).all()) and float(seen[ps].abs().max()) > 0, ps
        assert bool(torch.isfinite(cam.grad).all()) and float(cam.grad.abs().max()) > 0
        live = [float(named[k].grad.abs().max()) for k in tables if named[k].grad is not None]
        assert len(live) == len(tables) and min(live) > 0 and all(math.isfinite(v) for v in live)
    assert abs(losses["fused"] - losses["composed"]) < 1e-5, losses
