"""Time the rendering evaluation: image_metrics (C ABI Section 9) on 1, 8 and 32 views at 680x1200 and 480x640 with
the bytes and float64 operations its definition needs; the reference-shaped fp32 torch SSIM (five grouped conv2d) and PSNR on the
same device for context; one 680x1200 view through inference.render_image(mode="mapping_vis") with the Replica model conf in chunks
of 2580 (the reference's split_n_pixels) and 65536 rays; evaluate_views on 4 views end to end.  Device events, warm-up first,
medians of REPS runs; per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
usage: python tools/bench_render_eval.py [reps=5]"""
import sys

import torch
import torch.nn.functional as F

from benchlib import median_ms, model, positionals, write_results
from nicer_slam_amd import inference
from nicer_slam_amd.render_eval import image_metrics, evaluate_views, _uv

# float64 operations per pixel and channel: 3 products + 2 x 5 x 11 FMAs (two separable passes, FMA = 2) + 13 for the formula
# + 3 for the squared error; bytes: both images read once (the halo re-reads hit the caches)
FLOP_PER_VALUE = 3 + 2 * 5 * 11 * 2 + 13 + 3


def parse_args(argv):
    return positionals(argv, reps=(int, 5))


def ref_fp32(x, y, H, W, w):
    """rend_util.get_psnr + utils/SSIM shaped: permute to [n, 3, H, W] and five grouped fp32 convolutions."""
    a = x.reshape(-1, H, W, 3).permute(0, 3, 1, 2)
    b = y.reshape(-1, H, W, 3).permute(0, 3, 1, 2)
    mu1, mu2 = F.conv2d(a, w, padding=5, groups=3), F.conv2d(b, w, padding=5, groups=3)
    s11 = F.conv2d(a * a, w, padding=5, groups=3) - mu1 ** 2
    s22 = F.conv2d(b * b, w, padding=5, groups=3) - mu2 ** 2
    s12 = F.conv2d(a * b, w, padding=5, groups=3) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s11 + s22 + 9e-4))
    return m.mean((1, 2, 3)), ((a - b) ** 2).mean((1, 2, 3))


def view(H, W, n):
    K = torch.eye(4, device="cuda")[None].repeat(n, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = 600.0
    K[:, 0, 2], K[:, 1, 2] = W / 2 - 0.5, H / 2 - 0.5
    poses = torch.eye(4, device="cuda")[None].repeat(n, 1, 1)
    for i in range(n):
        poses[i, :3, 3] = torch.tensor([0.05 * i, 0.05, -0.2], device="cuda")
    return K, poses


def main(argv=None):
    REPS = parse_args(sys.argv[1:] if argv is None else argv).reps
    timed = lambda fn, reps=REPS: median_ms(fn, reps)
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS}
    g = torch.Generator(device="cuda").manual_seed(0)
    import ssim_ref
    g1 = torch.from_numpy(ssim_ref.window_1d())[:, None]
    w = (g1 @ g1.t()).float()[None, None].expand(3, 1, 11, 11).contiguous().cuda()
    for H, W in ((680, 1200), (480, 640)):
        for n in (1, 8, 32):
            x = torch.rand(n, H * W, 3, device="cuda", generator=g)
            y = (x + 0.05 * torch.randn(n, H * W, 3, device="cuda", generator=g)).clamp(0, 1)
            key = f"{H}x{W} n={n}"
            ms = timed(lambda: image_metrics(x, y, (H, W)))
            values = n * H * W * 3
            out[key + " image_metrics ms"] = ms
            out[key + " image_metrics GB/s"] = 2 * 4 * values / ms / 1e6
            out[key + " image_metrics fp64 GFLOP/s"] = FLOP_PER_VALUE * values / ms / 1e6
            out[key + " torch fp32 conv ms"] = timed(lambda: ref_fp32(x, y, H, W, w))
            del x, y
    m = model()
    H, W = 680, 1200
    K, poses = view(H, W, 4)
    uv = _uv(H, W, "cuda")[None]
    inp = {"intrinsics": K[:1], "uv": uv, "pose": poses[:1]}
    idx = torch.zeros(1, dtype=torch.long, device="cuda")
    for chunk in (2580, 65536):
        ms = timed(lambda: inference.render_image(m, inp, idx, mode="mapping_vis", n_pixels=chunk), reps=max(1, REPS // 2))
        out[f"render_image 680x1200 chunk {chunk} ms"] = ms
        out[f"render_image 680x1200 chunk {chunk} rays/s"] = H * W / ms * 1e3
    out["render_image engine"] = m.last_engine
    moved = poses.clone()
    moved[:, :3, 3] += 0.01                              # ground truth from nearby poses: finite PSNR
    gt = torch.stack([inference.render_image(m, {"intrinsics": K[i:i + 1], "uv": uv, "pose": moved[i:i + 1]}, idx,
                                             mode="mapping_vis")["rgb_values"].reshape(H * W, 3) for i in range(4)])
    out["evaluate_views 4 x 680x1200 ms"] = timed(lambda: evaluate_views(m, K, poses, gt, (H, W)), reps=max(1, REPS // 2))
    r = evaluate_views(m, K, poses, gt, (H, W))
    out["evaluate_views psnr / ssim means"] = [r["psnr_mean"], r["ssim_mean"]]
    write_results(out)


if __name__ == "__main__":
    main()
