"""Rendering metrics on the MI355X: C ABI Section 9 held to the float64 oracle (tests/ssim_ref.py) per image, its exact cases,
the drop-ins, and the evaluation loop end to end (render -> score -> files -> command line)."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_ref as S

pytestmark = pytest.mark.gpu


def _metrics(pred, gt, ssim_map=True):
    from nicer_slam_amd.render_eval import image_metrics
    H, W = pred.shape[-3:-1]
    return image_metrics(torch.from_numpy(pred).cuda()[None], torch.from_numpy(gt).cuda()[None], (H, W), ssim_map=ssim_map)


def _ref_fp32_torch(pred, gt):
    """The reference's SSIM shape (utils/SSIM: five grouped fp32 conv2d with the fp32 2-D window) on the device."""
    g = torch.from_numpy(S.window_1d())[:, None]
    w = (g @ g.t()).float()[None, None].expand(3, 1, 11, 11).contiguous().cuda()
    x = torch.from_numpy(pred).cuda().permute(2, 0, 1)[None]
    y = torch.from_numpy(gt).cuda().permute(2, 0, 1)[None]
    mu1, mu2 = F.conv2d(x, w, padding=5, groups=3), F.conv2d(y, w, padding=5, groups=3)
    s11 = F.conv2d(x * x, w, padding=5, groups=3) - mu1 ** 2
    s22 = F.conv2d(y * y, w, padding=5, groups=3) - mu2 ** 2
    s12 = F.conv2d(x * y, w, padding=5, groups=3) - mu1 * mu2
    m = ((2 * mu1 * mu2 + S.C1) * (2 * s12 + S.C2)) / ((mu1 ** 2 + mu2 ** 2 + S.C1) * (s11 + s22 + S.C2))
    return float(m.mean())


def _cases():
    rng = np.random.default_rng(11)
    out = []

    def add(name, p, g):
        out.append((name, np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(g, dtype=np.float32)))
    for H, W in ((1, 1), (1, 17), (5, 3), (11, 11), (15, 31), (15, 33), (16, 32), (17, 31), (17, 33), (33, 65)):
        add(f"noise{H}x{W}", rng.random((H, W, 3)), rng.random((H, W, 3)))
    H, W = 120, 200
    r = np.linspace(0, 1, H * W).reshape(H, W, 1).repeat(3, -1)
    add("ramp", r, r ** 1.1)
    add("constants", np.full((H, W, 3), 0.37), np.full((H, W, 3), 0.61))
    add("near_constants", np.full((40, 50, 3), 0.5), np.full((40, 50, 3), 0.5) + np.float32(2 ** -20))
    add("out_of_range", rng.uniform(-0.5, 1.8, (37, 45, 3)), rng.uniform(-0.5, 1.8, (37, 45, 3)))
    t = rng.random((480, 640, 3))
    add("480x640", t, np.clip(t + rng.normal(0, 0.05, t.shape), 0, 1))
    t = np.sin(np.arange(680)[:, None, None] / 30.0) * np.cos(np.arange(1200)[None, :, None] / 50.0 + np.arange(3)) * 0.4 + 0.5
    add("680x1200", t, t + rng.normal(0, 0.02, t.shape))
    return out


@pytest.mark.parametrize("name,pred,gt", _cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_kernel_against_float64(name, pred, gt):
    psnr, ssim, mse, smap = _metrics(pred, gt)
    ref_map = S.ssim_map(pred, gt)
    ref_ssim = float(ref_map.mean())
    ref_sse = S.sq_err_sum(pred, gt)
    got_ssim, got_mse = float(ssim[0]), float(mse[0])
    assert abs(got_ssim - ref_ssim) <= 1e-9, (name, got_ssim, ref_ssim)
    ref_mse = ref_sse / pred.size
    assert abs(got_mse - ref_mse) <= 1e-11 * ref_mse, (name, got_mse, ref_mse)
    assert float(psnr[0]) == pytest.approx(-10 * math.log10(ref_mse), rel=0, abs=1e-9)
    m64 = ref_map.mean(-1)
    tol = np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64) + 1e-12
    err = np.abs(smap[0].cpu().numpy().astype(np.float64) - m64)
    assert (err <= tol).all(), (name, float(err.max()))
    fp32 = _ref_fp32_torch(pred, gt)
    print(f"{name}: |kernel - float64| {abs(got_ssim - ref_ssim):.2e}   |reference-shaped fp32 torch - float64| "
          f"{abs(fp32 - ref_ssim):.2e}")


def test_self_comparison_is_exact():
    rng = np.random.default_rng(2)
    for H, W in ((1, 1), (23, 31), (68, 120)):
        x = rng.random((H, W, 3)).astype(np.float32)
        psnr, ssim, mse, smap = _metrics(x, x)
        assert float(ssim[0]) == 1.0 and float(mse[0]) == 0.0 and float(psnr[0]) == math.inf
        assert bool((smap == 1.0).all())


def test_batches_are_bit_identical_to_single_images_and_repeatable():
    from nicer_slam_amd.render_eval import image_metrics
    rng = np.random.default_rng(3)
    H, W = 45, 70
    x = torch.from_numpy(rng.random((5, H, W, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.random((5, H, W, 3)).astype(np.float32)).cuda()
    batch = image_metrics(x, y, (H, W), ssim_map=True)
    again = image_metrics(x, y, (H, W), ssim_map=True)
    for a, b in zip(batch, again):
        assert torch.equal(a, b)
    for i in range(5):
        one = image_metrics(x[i:i + 1], y[i].reshape(H * W, 3), (H, W), ssim_map=True)
        for a, b in zip(batch, one):
            assert torch.equal(a[i:i + 1], b)


def test_non_finite_values_poison_their_image_only():
    from nicer_slam_amd.render_eval import image_metrics
    rng = np.random.default_rng(4)
    H, W = 30, 40
    x = torch.from_numpy(rng.random((4, H, W, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.random((4, H, W, 3)).astype(np.float32)).cuda()
    clean = image_metrics(x, y, (H, W))
    x[1, 7, 9, 2] = float("nan")
    y[2, 29, 39, 0] = float("inf")
    x[3, 0, 0, 1] = float("-inf")
    psnr, ssim, mse = image_metrics(x, y, (H, W))
    for i in (1, 2, 3):
        assert math.isnan(float(ssim[i])) and math.isnan(float(mse[i])) and math.isnan(float(psnr[i])), i
    assert torch.equal(ssim[0], clean[1][0]) and torch.equal(mse[0], clean[2][0])


def test_arguments_are_checked():
    from nicer_slam_amd.render_eval import image_metrics
    x = torch.rand(2, 12, 3, device="cuda")
    with pytest.raises(ValueError):
        image_metrics(x, x[:1], (3, 4))
    with pytest.raises(ValueError):
        image_metrics(x, x, (4, 4))
    with pytest.raises(ValueError):
        image_metrics(x.cpu(), x, (3, 4))


def test_dropins_agree_with_the_oracle():
    from nicer_slam_amd.render_eval import get_psnr, get_ssim
    rng = np.random.default_rng(6)
    H, W = 40, 64
    p, g = rng.random((H, W, 3)).astype(np.float32), rng.random((H, W, 3)).astype(np.float32)
    a, b = torch.from_numpy(p).cuda().reshape(-1, 3), torch.from_numpy(g).cuda().reshape(-1, 3)
    assert abs(get_ssim(a, b, (H, W), object()).item() - S.ssim(p, g)) <= 1e-9
    assert get_psnr(a, b).item() == pytest.approx(S.psnr(p, g), rel=0, abs=1e-9)
    assert get_psnr(a * 2 - 1, b * 2 - 1, normalize_rgb=True).item() == pytest.approx(S.psnr(p, g), rel=1e-6)


# ---- the evaluation loop -----------------------------------------------------------------------------------------------------

def _model():
    from nicer_slam_amd.utils.conf import replica_model_conf
    from nicer_slam_amd.model.network import SLAMNetwork
    torch.manual_seed(4)
    m = SLAMNetwork(replica_model_conf(use_warp_loss=False)).cuda()
    with torch.no_grad():
        for enc in (m.implicit_network.coarse.encoding, m.implicit_network.fine.encoding, m.rendering_network.encoding):
            enc.embeddings.uniform_(-0.05, 0.05)
    return m.eval()


def _views(H, W, n):
    K = torch.eye(4, device="cuda")[None].repeat(n, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = 30.0
    K[:, 0, 2], K[:, 1, 2] = W / 2 - 0.5, H / 2 - 0.5
    poses = torch.eye(4, device="cuda")[None].repeat(n, 1, 1)
    for i in range(n):
        poses[i, :3, 3] = torch.tensor([0.1 * i, 0.05, -0.2], device="cuda")
    return K, poses


def _render(m, K, poses, H, W):
    from nicer_slam_amd import inference
    from nicer_slam_amd.render_eval import _uv
    uv = _uv(H, W, "cuda")[None]
    out = []
    for i in range(poses.shape[0]):
        inp = {"intrinsics": K[i:i + 1], "uv": uv, "pose": poses[i:i + 1]}
        rgb = inference.render_image(m, inp, torch.tensor([i], device="cuda"), mode="mapping_vis")["rgb_values"]
        out.append(rgb.reshape(1, H * W, 3))
    return torch.cat(out, 0)


def test_evaluate_views_end_to_end(tmp_path, capsys):
    from nicer_slam_amd.render_eval import evaluate_views, image_metrics, load_png, main, read_csv
    m = _model()
    H, W, n = 24, 40, 3
    K, poses = _views(H, W, n)
    gt = _render(m, K, poses, H, W)
    assert m.last_engine == "fused" and float(gt.std()) > 0
    same = evaluate_views(m, K, poses, gt, (H, W), n_pixels=173)
    assert (same["ssim"] == 1.0).all() and (same["psnr"] == math.inf).all()

    moved = poses.clone()
    moved[:, :3, 3] += torch.tensor([0.03, -0.02, 0.01], device="cuda")
    r = evaluate_views(m, K, moved, gt, (H, W), indices=[0, 2], out_dir=str(tmp_path), method="extrapolate")
    assert r["indices"] == [0, 2]
    assert (r["ssim"] < 1.0).all() and np.isfinite(r["psnr"]).all()
    ev = _render(m, K, moved, H, W)
    p, s, _ = image_metrics(ev[[0, 2]], gt[[0, 2]], (H, W))
    assert np.array_equal(r["psnr"], p.cpu().numpy()) and np.array_equal(r["ssim"], s.cpu().numpy())

    d = tmp_path / "rendering_extrapolation"
    for i in (0, 2):
        for kind in ("gt", "eval", "residual"):
            assert (d / f"{kind}_{i:04d}.png").exists()
    assert not (d / "eval_0001.png").exists()
    np.testing.assert_array_equal(read_csv(d / "psnr.csv"), np.concatenate([p.cpu().numpy(), [r["psnr_mean"], r["psnr_std"]]]))
    np.testing.assert_array_equal(read_csv(d / "ssim.csv"), np.concatenate([s.cpu().numpy(), [r["ssim_mean"], r["ssim_std"]]]))
    log = (tmp_path / "extrapolate.log").read_text().splitlines()
    assert log[0] == "psnr mean = %.2f ; psnr std = %.2f" % (r["psnr_mean"], r["psnr_std"])
    assert log[1] == "ssim mean = %.3f ; ssim std = %.3f" % (r["ssim_mean"], r["ssim_std"])
    assert "lpips" in log[2]

    # the PNGs hold the clipped, 8-bit images; the command line scores exactly those
    q = lambda t: (np.clip(t.reshape(H, W, 3).cpu().numpy(), 0, 1) * 255).astype(np.uint8).astype(np.float32) / np.float32(255)
    for i in (0, 2):
        assert np.array_equal(load_png(d / f"eval_{i:04d}.png"), q(ev[i]))
        assert np.array_equal(load_png(d / f"gt_{i:04d}.png"), q(gt[i]))
    qe = torch.from_numpy(np.stack([q(ev[i]) for i in (0, 2)])).cuda()
    qg = torch.from_numpy(np.stack([q(gt[i]) for i in (0, 2)])).cuda()
    qp, qs, _ = image_metrics(qe, qg, (H, W))
    capsys.readouterr()
    assert main([str(d), "--json"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["indices"] == [0, 2] and "quantised" in out["note"]
    assert out["psnr"] == qp.cpu().tolist() and out["ssim"] == qs.cpu().tolist()
    assert main([str(d)]) == 0
    text = capsys.readouterr().out
    assert "psnr mean = " in text and "quantised" in text
