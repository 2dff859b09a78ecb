"""Rendering metrics on the device: what code/evaluation/eval_rendering.py computes with rend_util.get_psnr, utils/SSIM and
its loop over held-out views.

* ``image_metrics``: PSNR, SSIM and MSE of a batch of image pairs in float64 (C ABI Section 9, csrc/image_metrics.hip).
* ``get_psnr`` / ``get_ssim``: drop-ins for rend_util.get_psnr / get_ssim.
* ``align_eval_poses``: prealign_cameras_apply_another (utils/cam_util.py) on the host, as datasets/scene_dataset.py calls it.
* ``eval_indices``: the held-out views of SLAMDataset_EVAL.
* ``evaluate_views``: render, score and write what eval_rendering.py writes (LPIPS is not computed).
* ``python -m nicer_slam_amd.render_eval DIR``: score the eval_NNNN.png / gt_NNNN.png pairs of a rendering_* directory.

SSIM is the reference's definition (11-tap Gaussian window, sigma 1.5, zero padding, C1 = 1e-4, C2 = 9e-4, mean over the
channels and pixels) evaluated in float64; the reference's fp32 moments cancel on smooth images by up to ~7e-4 per pixel.  A pair
with a non-finite value gets NaN for both metrics.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import json
import math
import os
import re

import numpy as np
import torch

from ._native import lib, check

LIMIT = 1 << 31                 # n_images * H * W * 3 per native call
LPIPS_NOTE = "lpips: not computed (needs the lpips package and AlexNet weights)"
QUANTISED_NOTE = ("metrics of 8-bit PNGs: these score the quantised images, not the float renders the reference scores "
                  "in eval_rendering.py")


def _images(x, name, img_res):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise ValueError(f"{name}: needs a CUDA tensor")
    H, W = int(img_res[0]), int(img_res[1])
    if H <= 0 or W <= 0:
        raise ValueError(f"{name}: bad img_res {tuple(img_res)}")
    if x.dim() == 2:
        x = x[None]
    if x.dim() == 4:
        if tuple(x.shape[1:]) != (H, W, 3):
            raise ValueError(f"{name}: expected [n, {H}, {W}, 3], got {tuple(x.shape)}")
        x = x.reshape(x.shape[0], H * W, 3)
    if x.dim() != 3 or x.shape[1] != H * W or x.shape[2] != 3:
        raise ValueError(f"{name}: expected [H*W, 3], [n, H*W, 3] or [n, H, W, 3] with H, W = {H}, {W}; got {tuple(x.shape)}")
    return x.detach().float().contiguous()


@torch.no_grad()
def image_metrics(pred, gt, img_res, ssim_map=False):
    """(psnr, ssim, mse) float64 [n] each, plus the fp32 SSIM map [n, H, W] (mean over the channels) when ``ssim_map``.
    pred, gt: CUDA tensors [H*W, 3], [n, H*W, 3] or [n, H, W, 3] with pixel (r, c) at r * W + c.  PSNR = -10 log10(mse), +inf
    for identical images; a pair with any non-finite value gives NaN everywhere.  Batches beyond 2^31 values are split."""
    x, y = _images(pred, "pred", img_res), _images(gt, "gt", img_res)
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f"image_metrics: pred {tuple(x.shape)} on {x.device} vs gt {tuple(y.shape)} on {y.device}")
    n, H, W = x.shape[0], int(img_res[0]), int(img_res[1])
    per = (LIMIT - 1) // (3 * H * W)
    if per == 0:
        raise ValueError(f"image_metrics: one {H}x{W} image exceeds 2^31 values")
    ssim = torch.empty(n, dtype=torch.float64, device=x.device)
    sse = torch.empty(n, dtype=torch.float64, device=x.device)
    smap = torch.empty(n, H, W, dtype=torch.float32, device=x.device) if ssim_map else None
    if n:
        ws = torch.empty(lib.nsa_image_metrics_workspace(min(n, per), H, W), dtype=torch.uint8, device=x.device)
        st = torch.cuda.current_stream(x.device).cuda_stream
        for lo in range(0, n, per):
            m = min(per, n - lo)
            check(lib.nsa_image_metrics(x[lo].data_ptr(), y[lo].data_ptr(), m, H, W, ws.data_ptr(), ssim[lo:].data_ptr(),
                                        sse[lo:].data_ptr(), smap[lo].data_ptr() if ssim_map else None, st))
    mse = sse / (3 * H * W)
    psnr = -10.0 * torch.log10(mse)
    return (psnr, ssim, mse, smap) if ssim_map else (psnr, ssim, mse)


def get_psnr(img1, img2, normalize_rgb=False):
    """rend_util.get_psnr: -10 log10(mean((img1 - img2)^2)) over all values of two CUDA tensors [..., 3] (a float64
    tensor [1]; the reference returns fp32 [1])."""
    if normalize_rgb:                                    # [-1, 1] -> [0, 1]
        img1, img2 = (img1 + 1.0) / 2.0, (img2 + 1.0) / 2.0
    a, b = img1.reshape(-1, 3), img2.reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"get_psnr: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    return image_metrics(a, b, (1, a.shape[0]))[0]


def get_ssim(img1, img2, res, ssim_computer=None):
    """rend_util.get_ssim: SSIM of two CUDA images [H*W, 3] at res = (H, W) (a float64 tensor [1]).  ``ssim_computer`` is
    accepted for the reference's call signature and ignored."""
    return image_metrics(img1.reshape(-1, 3), img2.reshape(-1, 3), res)[1]


# ---- held-out views -------------------------------------------------------------------------------------------------

def eval_indices(method, n_images):
    """SLAMDataset_EVAL's views (datasets/scene_dataset.py:308-311)."""
    if method == "interpolate":
        return range(2, n_images, 100)
    if method == "extrapolate":
        return range(100)
    raise ValueError(f"eval_indices: method must be 'interpolate' or 'extrapolate', got {method!r}")


def _invert(pose):
    """Pose().invert: [R|t] -> [R^T | -R^T t] (fp32)."""
    R, t = pose[..., :3], pose[..., 3:]
    Ri = R.transpose(-1, -2)
    return torch.cat([Ri.float(), (-Ri @ t).float()], -1)


def _centres(c2w):
    """cam2world(0, invert(c2w)): the camera centres [N, 3] as the reference computes them (fp32)."""
    w2c = _invert(c2w)
    hom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    return (hom @ _invert(w2c).transpose(-1, -2))[:, 0]


@torch.no_grad()
def align_eval_poses(est_c2w, gt_c2w, eval_c2w):
    """Map held-out ground-truth poses into the estimated trajectory's frame: datasets/scene_dataset.py calls
    prealign_cameras_apply_another(gt_c2w, est_c2w, eval_c2w) (utils/cam_util.py:94-115), restated here on the host in fp32.
    est_c2w, gt_c2w [N, 3|4, 4] (the first N frames of the run), eval_c2w [M, 3|4, 4].  Procrustes on the camera centres with
    X0 = the estimate's, X1 = ground truth's (in the function's own names: pose_GT is the estimate), the SVD in float64 and
    R[2] *= -1 on a reflection; an SVD that does not converge gives the identity, as in the reference.
    Returns (aligned eval poses [M, 3, 4] camera-to-world, sim3 dict t0, t1 [3], s0, s1 scalars, R [3, 3])."""
    est = torch.as_tensor(est_c2w).detach().cpu().float()[:, :3, :4]
    gt = torch.as_tensor(gt_c2w).detach().cpu().float()[:, :3, :4]
    ev = torch.as_tensor(eval_c2w).detach().cpu().float()[:, :3, :4]
    if est.shape != gt.shape or est.shape[0] < 1:
        raise ValueError(f"align_eval_poses: est {tuple(est.shape)} vs gt {tuple(gt.shape)}")
    X1, X0 = _centres(gt), _centres(est)              # cam2world(center, pose) / (center, pose_GT)
    ev_w2c = _invert(ev)
    ca = _centres(ev)
    try:
        t0, t1 = X0.mean(0, keepdim=True), X1.mean(0, keepdim=True)
        X0c, X1c = X0 - t0, X1 - t1
        s0, s1 = (X0c ** 2).sum(-1).mean().sqrt(), (X1c ** 2).sum(-1).mean().sqrt()
        U, _, V = ((X0c / s0).t() @ (X1c / s1)).double().svd(some=True)
        R = (U @ V.t()).float()
        if R.det() < 0:
            R[2] *= -1
        sim3 = dict(t0=t0[0], t1=t1[0], s0=s0, s1=s1, R=R)
    except RuntimeError:                                 # torch.linalg.LinAlgError
        sim3 = dict(t0=torch.zeros(3), t1=torch.zeros(3), s0=torch.tensor(1.0), s1=torch.tensor(1.0), R=torch.eye(3))
    c = (ca - sim3["t1"]) / sim3["s1"] @ sim3["R"].t() * sim3["s0"] + sim3["t0"]
    R_al = ev_w2c[..., :3] @ sim3["R"].t()
    t_al = (-R_al @ c[..., None])[..., 0]
    return _invert(torch.cat([R_al.float(), t_al.float()[..., None]], -1)), sim3


# ---- the evaluation loop ----------------------------------------------------------------------------------------------

def _uv(H, W, device):
    """SLAMDataset_EVAL's pixel list: (column, row) per pixel, row-major."""
    vv, uu = torch.meshgrid(torch.arange(H, device=device).float(), torch.arange(W, device=device).float(), indexing="ij")
    return torch.stack([uu.reshape(-1), vv.reshape(-1)], -1)


def _to_uint8(img):
    """[H, W, 3] float -> uint8 as eval_rendering.py writes PNGs, except that values are clipped to [0, 1] first: the
    reference's astype(np.uint8) wraps out-of-range values around (1.02 * 255 -> 4)."""
    return (np.clip(img, 0.0, 1.0) * 255).astype(np.uint8)


def _write_png(path, img):
    from PIL import Image
    Image.fromarray(_to_uint8(img)).save(path)


def _repr(v):
    return repr(float(v))


def write_csv(path, values):
    """pandas.DataFrame(values + [mean, std]).to_csv(path) as eval_rendering.py writes psnr.csv / ssim.csv: a header ',0', then
    'i,value' rows, the last two the mean and the (population) std.  Values are written in Python's shortest repr."""
    v = np.asarray(values, dtype=np.float64)
    rows = np.concatenate([v, [v.mean(), v.std()]])
    with open(path, "w") as f:
        f.write(",0\n" + "".join(f"{i},{_repr(x)}\n" for i, x in enumerate(rows)))


def read_csv(path):
    """The values of a psnr.csv / ssim.csv (the mean and std rows included)."""
    lines = open(path).read().splitlines()
    if not lines or lines[0] != ",0":
        raise ValueError(f"{path}: not a one-column DataFrame csv")
    out = []
    for k, ln in enumerate(lines[1:]):
        i, x = ln.split(",")
        if int(i) != k:
            raise ValueError(f"{path}: row {k} has index {i}")
        out.append(float(x))
    return np.array(out)


def summary_lines(psnrs, ssims):
    """eval_rendering.py's summary lines, plus one line saying that LPIPS is not computed."""
    p, s = np.asarray(psnrs, dtype=np.float64), np.asarray(ssims, dtype=np.float64)
    return ["psnr mean = %.2f ; psnr std = %.2f" % (p.mean(), p.std()),
            "ssim mean = %.3f ; ssim std = %.3f" % (s.mean(), s.std()), LPIPS_NOTE]


@torch.no_grad()
def evaluate_views(model, intrinsics, poses, gt_rgb, img_res, indices=None, out_dir=None, method="interpolate",
                   n_pixels=65536):
    """Render each held-out view with inference.render_image(mode="mapping_vis") on ``model`` (put in eval mode) and score
    it against its ground truth on the device.

    intrinsics [N, 4, 4] or [4, 4], poses [N, 4, 4] camera-to-world (already in the run's frame, see align_eval_poses),
    gt_rgb [N, H*W, 3] or [N, H, W, 3] with img_res = (H, W); ``indices`` selects views (default: all) and names the files.
    Chunked rendering equals a single pass bit for bit, so the chunk ``n_pixels`` (the reference uses split_n_pixels = 2580)
    changes the speed only.  With ``out_dir`` it writes what eval_rendering.py writes under
    out_dir/rendering_<interpolation|extrapolation>/: gt_%04d.png, eval_%04d.png, residual_%04d.png (clipped to [0, 1],
    see _to_uint8), psnr.csv, ssim.csv, and out_dir/<method>.log.  LPIPS is not computed.
    Returns {"indices", "psnr", "ssim" (numpy float64 [V]), "psnr_mean", "psnr_std", "ssim_mean", "ssim_std"}."""
    from .inference import render_image
    if method not in ("interpolate", "extrapolate"):
        raise ValueError(f"evaluate_views: method must be 'interpolate' or 'extrapolate', got {method!r}")
    H, W = int(img_res[0]), int(img_res[1])
    dev = poses.device
    gt = _images(gt_rgb.to(dev), "gt_rgb", img_res)
    N = gt.shape[0]
    if poses.shape[0] != N:
        raise ValueError(f"evaluate_views: {poses.shape[0]} poses for {N} images")
    K = intrinsics.to(dev).float()
    if K.dim() == 2:
        K = K[None].expand(N, 4, 4)
    idx = list(range(N)) if indices is None else [int(i) for i in indices]
    model.eval()
    uv = _uv(H, W, dev)[None]
    images_dir = None
    if out_dir is not None:
        images_dir = os.path.join(out_dir, "rendering_" + ("interpolation" if method == "interpolate" else "extrapolation"))
        os.makedirs(images_dir, exist_ok=True)
    psnrs, ssims = [], []
    for i in idx:
        inp = {"intrinsics": K[i:i + 1].contiguous(), "uv": uv, "pose": poses[i:i + 1].float().contiguous()}
        rgb = render_image(model, inp, torch.tensor([i], device=dev), mode="mapping_vis", n_pixels=n_pixels)["rgb_values"]
        p, s, _ = image_metrics(rgb.reshape(1, H * W, 3), gt[i:i + 1], (H, W))
        psnrs.append(float(p[0]))
        ssims.append(float(s[0]))
        if images_dir is not None:
            g = gt[i].reshape(H, W, 3).cpu().numpy()
            e = rgb.reshape(H, W, 3).float().cpu().numpy()
            _write_png(os.path.join(images_dir, "gt_%04d.png" % i), g)
            _write_png(os.path.join(images_dir, "eval_%04d.png" % i), e)
            _write_png(os.path.join(images_dir, "residual_%04d.png" % i), np.abs(g - e))
    p, s = np.array(psnrs, dtype=np.float64), np.array(ssims, dtype=np.float64)
    if images_dir is not None and idx:
        write_csv(os.path.join(images_dir, "psnr.csv"), p)
        write_csv(os.path.join(images_dir, "ssim.csv"), s)
        with open(os.path.join(images_dir, "..", method + ".log"), "w") as f:
            f.write("\n".join(summary_lines(p, s)) + "\n")
    return {"indices": idx, "psnr": p, "ssim": s, "psnr_mean": float(p.mean()) if idx else math.nan,
            "psnr_std": float(p.std()) if idx else math.nan, "ssim_mean": float(s.mean()) if idx else math.nan,
            "ssim_std": float(s.std()) if idx else math.nan}


# ---- scoring PNGs a run has written -----------------------------------------------------------------------------------

_EVAL_RE = re.compile(r"^eval_(\d{4,})\.png$")


def png_pairs(directory):
    """[(index, eval path, gt path)] of a rendering_* directory, by index.  Every eval_NNNN.png needs its gt_NNNN.png and
    vice versa; a directory without pairs is an error."""
    names = set(os.listdir(directory))
    evals = {int(m.group(1)): n for n in names if (m := _EVAL_RE.match(n))}
    gts = {int(n[3:-4]): n for n in names if re.match(r"^gt_\d{4,}\.png$", n)}
    missing = sorted(set(evals) ^ set(gts))
    if missing:
        raise ValueError(f"{directory}: no partner for index {missing[0]:04d} (eval_NNNN.png and gt_NNNN.png come in pairs)")
    if not evals:
        raise ValueError(f"{directory}: no eval_NNNN.png / gt_NNNN.png pairs")
    return [(i, os.path.join(directory, evals[i]), os.path.join(directory, gts[i])) for i in sorted(evals)]


def load_png(path):
    """An RGB PNG as float32 [H, W, 3] in [0, 1] (uint8 / 255)."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return a.astype(np.float32) / np.float32(255)


def load_pairs(directory):
    """[(index, eval [H, W, 3], gt [H, W, 3])]; a pair whose two images differ in size is an error."""
    out = []
    for i, e, g in png_pairs(directory):
        a, b = load_png(e), load_png(g)
        if a.shape != b.shape:
            raise ValueError(f"{directory}: eval_{i:04d}.png is {a.shape[1]}x{a.shape[0]}, gt_{i:04d}.png {b.shape[1]}x{b.shape[0]}")
        out.append((i, a, b))
    return out


def score_directory(directory, device="cuda"):
    """Score every eval/gt PNG pair of a rendering_* directory: {"indices", "psnr", "ssim", means and stds}."""
    idx, ps, ss = [], [], []
    for i, a, b in load_pairs(directory):
        H, W = a.shape[:2]
        p, s, _ = image_metrics(torch.from_numpy(a).to(device)[None], torch.from_numpy(b).to(device)[None], (H, W))
        idx.append(i)
        ps.append(float(p[0]))
        ss.append(float(s[0]))
    p, s = np.array(ps), np.array(ss)
    return {"indices": idx, "psnr": p, "ssim": s, "psnr_mean": float(p.mean()), "psnr_std": float(p.std()),
            "ssim_mean": float(s.mean()), "ssim_std": float(s.std())}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.render_eval",
                                 description="PSNR and SSIM of every eval_NNNN.png against gt_NNNN.png in a rendering_* directory "
                                             "that eval_rendering.py wrote, on the GPU.  Note: " + QUANTISED_NOTE + ".")
    ap.add_argument("directory")
    ap.add_argument("--json", action="store_true", help="print one JSON object instead of the reference's summary lines")
    a = ap.parse_args(argv)
    r = score_directory(a.directory)
    if a.json:
        print(json.dumps({"note": QUANTISED_NOTE, "indices": r["indices"], "psnr": r["psnr"].tolist(), "ssim": r["ssim"].tolist(),
                          **{k: r[k] for k in ("psnr_mean", "psnr_std", "ssim_mean", "ssim_std")}}))
    else:
        for i, p, s in zip(r["indices"], r["psnr"], r["ssim"]):
            print("%04d  psnr %.4f  ssim %.6f" % (i, p, s))
        print("\n".join(summary_lines(r["psnr"], r["ssim"])))
        print("note: " + QUANTISED_NOTE)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
