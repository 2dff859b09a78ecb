"""Rendering metrics without a GPU: the float64 oracle against the reference's own SSIM / PSNR values, pose alignment, the
reference's csv / log format, the PNG pairing rules of the command line and C ABI Section 9's argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import ssim_ref as S
from helpers import GOLDEN

FIXTURE = os.path.join(GOLDEN, "render_metrics.npz")


def _fx():
    return np.load(FIXTURE, allow_pickle=False)


def _decode(code):
    return code.astype(np.float32) / np.float32(255)


def _pairs(fx):
    k = 0
    while f"pair{k}_pred" in fx:
        yield k, _decode(fx[f"pair{k}_pred"]), _decode(fx[f"pair{k}_gt"])
        k += 1


def test_oracle_matches_the_reference_values():
    fx = _fx()
    seen = []
    for k, p, g in _pairs(fx):
        seen.append(p.shape[:2])
        assert abs(S.ssim(p, g) - float(fx[f"pair{k}_ssim"])) <= 1e-5, k
        assert abs(S.psnr(p, g) - float(fx[f"pair{k}_psnr"])) <= 1e-4, k
    assert len(seen) == 4 and (68, 120) in seen
    assert fx["pair3_pred"].min() < 0 and fx["pair3_gt"].max() > 255          # the out-of-range pair


def test_oracle_window_is_the_reference_window():
    g = S.window_1d()
    assert g.dtype == np.float32 and g.shape == (11,)
    assert np.array_equal(g, g[::-1]) and abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-6
    # the reference builds it as torch.Tensor of the float64 Gaussian divided by torch's fp32 sum
    raw = torch.tensor([math.exp(-((k - 5) ** 2) / float(2 * 1.5 ** 2)) for k in range(11)], dtype=torch.float32)
    assert np.array_equal((raw / raw.sum()).numpy(), g)
    w = S.window_2d()
    assert np.array_equal(w, np.outer(g.astype(np.float64), g.astype(np.float64)))
    # the reference's fp32-rounded 2-D weights differ from the exact products by at most half an fp32 ulp
    assert np.abs(w.astype(np.float32).astype(np.float64) - w).max() <= 2.0 ** -24 * w.max()


def test_oracle_exact_cases():
    rng = np.random.default_rng(0)
    x = rng.random((9, 14, 3)).astype(np.float32)
    assert S.ssim(x, x) == 1.0 and S.psnr(x, x) == math.inf
    c = np.full((12, 7, 3), 0.37, np.float32)
    assert abs(S.ssim(c, c) - 1.0) < 1e-15
    assert S.ssim(c, np.full_like(c, 0.61)) < 1.0


def _align_ref_free(est, gt, ev):
    from nicer_slam_amd.render_eval import align_eval_poses
    return align_eval_poses(torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(ev))


@pytest.mark.parametrize("k", [0, 1])
def test_align_eval_poses_matches_the_reference(k):
    fx = _fx()
    out, sim3 = _align_ref_free(fx[f"align{k}_est"], fx[f"align{k}_gt"], fx[f"align{k}_eval"])
    assert out.dtype == torch.float32 and tuple(out.shape) == fx[f"align{k}_out"].shape
    np.testing.assert_allclose(out.numpy(), fx[f"align{k}_out"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(sim3["R"].numpy(), fx[f"align{k}_R"], rtol=0, atol=1e-6)
    for key in ("t0", "t1", "s0", "s1"):
        np.testing.assert_allclose(np.asarray(sim3[key]), fx[f"align{k}_{key}"], rtol=1e-6, atol=1e-6)


def _rot(axis, th):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def _poses(rng, n):
    R = np.stack([_rot(rng.normal(size=3), rng.uniform(0, math.pi)) for _ in range(n)])
    return np.concatenate([R, rng.uniform(-2, 2, (n, 3, 1))], -1).astype(np.float32)


def _map(poses, s, R, t, M=np.eye(3)):
    c = (s * poses[:, :, 3].astype(np.float64) @ R.T + t) @ M.T
    return np.concatenate([M @ R @ poses[:, :, :3].astype(np.float64), c[..., None]], -1).astype(np.float32)


def test_align_eval_poses_recovers_a_known_sim3():
    rng = np.random.default_rng(3)
    gt, ev = _poses(rng, 20), _poses(rng, 6)
    R, s, t = _rot([0.3, -1.0, 0.4], 0.9), 1.7, np.array([0.5, -0.2, 1.1])
    est = _map(gt, s, R, t)
    out, sim3 = _align_ref_free(est, gt, ev)
    want = _map(ev, s, R, t)                             # the held-out poses in the estimate's frame
    np.testing.assert_allclose(out.numpy(), want, rtol=0, atol=1e-5)
    np.testing.assert_allclose(sim3["R"].numpy(), R, atol=1e-5)
    assert abs(float(sim3["s0"]) / float(sim3["s1"]) - s) < 1e-5


def test_align_eval_poses_reflection_branch():
    rng = np.random.default_rng(5)
    gt, ev = _poses(rng, 15), _poses(rng, 3)
    M = np.diag([-1.0, 1.0, 1.0])
    est = _map(gt, 1.0, np.eye(3), np.zeros(3), M)
    # the unconstrained Procrustes rotation is a reflection here ...
    from nicer_slam_amd.render_eval import _centres
    X0, X1 = _centres(torch.from_numpy(est)).double(), _centres(torch.from_numpy(gt)).double()
    X0c, X1c = X0 - X0.mean(0), X1 - X1.mean(0)
    U, _, V = (X0c.t() @ X1c).svd()
    assert float(torch.det(U @ V.t())) < 0
    # ... and align_eval_poses returns the reference's proper rotation (third row negated)
    out, sim3 = _align_ref_free(est, gt, ev)
    assert abs(float(torch.det(sim3["R"])) - 1.0) < 1e-5
    np.testing.assert_allclose(sim3["R"].numpy(), (U @ V.t()).float().numpy() * np.array([[1.0], [1.0], [-1.0]]), atol=1e-6)
    assert torch.isfinite(out).all()


def test_eval_indices():
    from nicer_slam_amd.render_eval import eval_indices
    assert list(eval_indices("interpolate", 2000)) == list(range(2, 2000, 100))
    assert list(eval_indices("extrapolate", 2000)) == list(range(100))
    with pytest.raises(ValueError):
        eval_indices("both", 10)


def test_csv_and_log_in_the_reference_format(tmp_path):
    from nicer_slam_amd.render_eval import write_csv, read_csv, summary_lines
    vals = np.array([30.125, 28.5, math.pi])
    write_csv(tmp_path / "psnr.csv", vals)
    text = (tmp_path / "psnr.csv").read_text()
    mean, std = vals.mean(), vals.std()
    assert text == f",0\n0,30.125\n1,28.5\n2,{math.pi!r}\n3,{float(mean)!r}\n4,{float(std)!r}\n"
    np.testing.assert_array_equal(read_csv(tmp_path / "psnr.csv"), np.concatenate([vals, [mean, std]]))
    try:                                                  # pandas, when present, reads and writes the same file
        import pandas as pd
        pd.DataFrame(np.concatenate([vals, [mean, std]])).to_csv(tmp_path / "pd.csv")
        assert (tmp_path / "pd.csv").read_text() == text
    except ImportError:
        pass
    lines = summary_lines(vals, [0.9, 0.8, 0.85])
    assert lines[0] == "psnr mean = %.2f ; psnr std = %.2f" % (mean, std)
    assert lines[1] == "ssim mean = 0.850 ; ssim std = 0.041"
    assert lines[2].startswith("lpips: not computed")
    bad = tmp_path / "bad.csv"
    bad.write_text("a,b\n0,1\n")
    with pytest.raises(ValueError):
        read_csv(bad)


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_png_pairing_rules(tmp_path):
    from nicer_slam_amd.render_eval import png_pairs, load_pairs, load_png, _to_uint8
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    for i in (2, 102):
        _png(tmp_path / f"eval_{i:04d}.png", a)
        _png(tmp_path / f"gt_{i:04d}.png", a[::-1].copy())
    _png(tmp_path / "residual_0002.png", a)
    assert [p[0] for p in png_pairs(tmp_path)] == [2, 102]
    got = load_pairs(tmp_path)
    assert np.array_equal(got[0][1], a.astype(np.float32) / np.float32(255))
    assert np.array_equal(load_png(tmp_path / "gt_0002.png"), a[::-1].astype(np.float32) / np.float32(255))
    # a missing partner is rejected
    _png(tmp_path / "eval_0202.png", a)
    with pytest.raises(ValueError, match="partner"):
        png_pairs(tmp_path)
    os.remove(tmp_path / "eval_0202.png")
    _png(tmp_path / "gt_0302.png", a)
    with pytest.raises(ValueError, match="partner"):
        png_pairs(tmp_path)
    os.remove(tmp_path / "gt_0302.png")
    # a size mismatch is rejected
    _png(tmp_path / "gt_0102.png", a[:5])
    with pytest.raises(ValueError, match="9x6"):
        load_pairs(tmp_path)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError):
        png_pairs(empty)
    # PNGs are written clipped, not wrapped as astype(np.uint8) would
    assert _to_uint8(np.array([[[-0.1, 0.5, 1.02]]])).tolist() == [[[0, 127, 255]]]


def test_image_metrics_rejects_cpu_tensors_and_bad_shapes():
    from nicer_slam_amd.render_eval import image_metrics
    x = torch.zeros(12, 3)
    with pytest.raises(ValueError, match="CUDA"):
        image_metrics(x, x, (3, 4))


def test_section9_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib, EXPORTS
    NSA_EBADARG = 4
    assert "nsa_image_metrics_workspace" in EXPORTS and "nsa_image_metrics" in EXPORTS
    ws = lib.nsa_image_metrics_workspace
    assert ws(0, 10, 10) == 0 and ws(1, 0, 10) == 0 and ws(1, 10, 0) == 0
    assert ws(1, 1, 1) == 16 and ws(2, 16, 32) == 32 and ws(1, 17, 33) == 64 and ws(3, 680, 1200) == 3 * 43 * 38 * 16
    lim = (1 << 31) // 3                                  # n * H * W * 3 < 2^31
    assert ws(1, 1, lim) > 0 and ws(1, 1, lim + 1) == 0 and ws(1 << 20, 1 << 10, 1 << 10) == 0
    fake = ctypes.c_void_p(4096)                          # never dereferenced: every call below is rejected before a launch
    args = dict(p=fake, g=fake, n=2, H=8, W=8, ws=fake, s=fake, e=fake, m=None)
    for key, val in (("p", None), ("g", None), ("ws", None), ("s", None), ("e", None), ("n", 0), ("H", 0), ("W", 0),
                     ("W", lim + 1), ("n", 1 << 30)):
        a = dict(args, **{key: val})
        assert lib.nsa_image_metrics(a["p"], a["g"], a["n"], a["H"], a["W"], a["ws"], a["s"], a["e"], a["m"], None) == \
            NSA_EBADARG, key
