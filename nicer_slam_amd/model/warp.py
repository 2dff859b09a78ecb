"""Patch-warp gather of the mapping objective (reference code/model/network.py:167-279, code/utils/general.py:129-145;
SURVEY 8f next-1).  Composed engine (torch ops): per-pixel work on a few thousand rays, not on the per-sample hot path.

For every patch size: the patch around each sampled pixel of every keyframe is lifted with the ray's RENDERED depth,
projected into every keyframe, and the full images are sampled there; the loss compares with the patch read directly
from the source image.  Returns {patchsize: (gt_warp_rgbs, target_sampled_rgb, total_warp_mask, depth_mask_ray_level)}
with the reference's shapes: [target, reference, n_pixels, patch^2, (3)]."""
import math

import torch
import torch.nn.functional as F

from ..utils import rend_util


def uv2patch(uv, patchsize):
    """[b, n, 2] pixel centres -> [b, n, p, p, 2] pixel coordinates of the p x p patch (general.py:129-145)."""
    if patchsize == 1:
        return uv.clone().reshape(-1, uv.shape[1], 1, 1, 2)
    half = patchsize // 2
    r = torch.arange(-half, half + 1, device=uv.device)
    gx, gy = torch.meshgrid(r, r, indexing="ij")
    return uv.unsqueeze(2).unsqueeze(2) + torch.stack([gx, gy], -1).to(uv.dtype)[None, None]


def patch_warp(model, uv, pose, intrinsics, rendered_depth, ground_truth, batch_size):
    H, W = model.H, model.W
    stacked = lambda t: t.stacked() if hasattr(t, "stacked") else t       # fused/warp.py::FrameStore (feed.py) or a plain tensor
    full_rgb = stacked(ground_truth["full_rgb"]).reshape(batch_size, H, W, 3)
    full_depth = stacked(ground_truth["full_depth"]).reshape(batch_size, H, W, 1)
    depth = rendered_depth.reshape(batch_size, -1, 1, 1)          # z of the centre ray, shared by its patch
    w2c = torch.linalg.inv(pose)
    out = {}
    for ps in model.patchsizes:
        p2 = ps * ps
        uvp = uv2patch(uv, ps).reshape(batch_size, -1, 2)                              # [b, n*p2, 2]
        dirs, cam_loc = rend_util.get_camera_params(uvp, pose, intrinsics)
        pts = cam_loc[:, None, None, :] + depth * dirs.reshape(batch_size, -1, p2, 3)  # [b, n, p2, 3] world
        flat = pts.reshape(-1, 3).t()                                                   # [3, b*n*p2]
        cam = w2c[:, :3, :3] @ flat + w2c[:, :3, 3:]                                    # [b_t, 3, M]
        proj = (intrinsics[:, :3, :3] @ cam).permute(0, 2, 1).reshape(batch_size, batch_size, -1, p2, 3)
        tz = proj[..., 2:]
        tuv = proj[..., :2] / (tz + 1e-8)
        grid = torch.stack([tuv[..., 0] / W, tuv[..., 1] / H], -1) * 2 - 1.0           # [-1, 1], align_corners=True
        grid = grid.reshape(batch_size, -1, 1, 2)
        sampled = F.grid_sample(full_rgb.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros",
                                align_corners=True)
        sampled = sampled.reshape(batch_size, 3, batch_size, -1, p2).permute(0, 2, 3, 4, 1)
        tmask = ((grid[..., 0] > -1) & (grid[..., 0] < 1) & (grid[..., 1] > -1) & (grid[..., 1] < 1)
                 & (tz.reshape(batch_size, -1, 1) > 0)).reshape(batch_size, batch_size, -1, p2)
        # the same patches read straight from their own image (ones outside the image)
        inside = (uvp[..., 0] >= 0) & (uvp[..., 1] >= 0) & (uvp[..., 0] < W) & (uvp[..., 1] < H)   # [b, n*p2]
        ui = uvp[..., 0].long().clamp(0, W - 1)
        vi = uvp[..., 1].long().clamp(0, H - 1)
        bidx = torch.arange(batch_size, device=uv.device)[:, None].expand_as(ui)
        gt_rgb = torch.where(inside[..., None], full_rgb[bidx, vi, ui], torch.ones_like(full_rgb[bidx, vi, ui]))
        gt_dep = torch.where(inside[..., None], full_depth[bidx, vi, ui], torch.ones_like(full_depth[bidx, vi, ui]))
        gmask = inside[None].expand(batch_size, -1, -1).reshape(batch_size, batch_size, -1, p2)
        gt_rgbs = gt_rgb.reshape(1, batch_size, -1, p2, 3).repeat(batch_size, 1, 1, 1, 1)
        total = gmask & tmask
        ray_level = None
        if ps > 1:   # keep only patches whose ground-truth depth is locally flat (network.py:259-270)
            flat_ok = torch.var(gt_dep.reshape(batch_size, -1, p2), dim=-1, unbiased=False) < 0.01
            ray_level = flat_ok.reshape(-1)
            total = total & flat_ok[None, :, :, None].expand(batch_size, -1, -1, p2)
        out[ps] = (gt_rgbs, sampled, total, ray_level)
    return out


def flow_reproject(uv, pose, intrinsics, rendered_depth, edges):
    """Optical-flow reprojection (network.py:150-165): the rendered 3-D point of every pixel of frame idii[e], projected into
    frame idjj[e], minus the pixel.  [n_edges, n, 2]."""
    bs = uv.shape[0]
    dirs, cam_loc = rend_util.get_camera_params(uv, pose, intrinsics)
    pts = (cam_loc.unsqueeze(1) + rendered_depth.reshape(bs, -1, 1) * dirs).permute(0, 2, 1)        # [b, 3, n]
    idii, idjj = edges[0], edges[1]
    w2c = torch.linalg.inv(pose[idjj])
    cam_pts = w2c[:, :3, :3] @ pts[idii] + w2c[:, :3, 3:]
    proj = (intrinsics[idjj][:, :3, :3] @ cam_pts).permute(0, 2, 1)
    return proj[..., :2] / (proj[..., 2:] + 1e-8) - uv[idii]


def ssim_window_1d(patch):
    """The p-tap sigma-1.5 Gaussian of pytorch_msssim's _fspecial_gauss_1d as csrc/patch_ssim.hip builds it: fp32 values of exp at the
    fp32 arguments -(k - p//2)^2 / 4.5, divided (in fp32) by their correctly rounded fp32 sum.  A CPU fp32 tensor [p]."""
    d = torch.arange(patch, dtype=torch.float32) - (patch // 2)
    arg = -(d * d) / 4.5
    g = torch.tensor([math.exp(float(a)) for a in arg], dtype=torch.float64).to(torch.float32)
    return g / g.double().sum().to(torch.float32)          # (the float64 sum of these few fp32 values is exact)


def patch_ssim_term(sampled, gt_rgb, mask, patch):
    """The SSIM form of the patch-warp term for one patch size (reference code/model/loss.py:145-152: pytorch_msssim's SSIM with
    win_size = patch, data_range 1): 0.05 * (1 - mean over patches and channels of SSIM), any dtype, any device, any odd
    patch >= 3.  The composed twin of fused/warp.py::patch_ssim, same definition (csrc/patch_ssim.hip): both patches are 0 outside
    the mask (zeroed, not excluded; the inputs are left alone), the 2-D weights are the exact products of the fp32 window, and
    the moments and the SSIM formula are evaluated in float64 -- sigma^2 = E[x^2] - mu^2 cancels on flat patches -- before
    1 - mean is rounded to the input's dtype.  A wholly masked patch counts with SSIM 1, as in the reference."""
    patch = int(patch)
    if patch < 3 or patch % 2 == 0:
        raise ValueError(f"patch_ssim_term: patch {patch} must be odd and >= 3")
    p2 = patch * patch
    wide = torch.promote_types(sampled.dtype, torch.float64)
    g = ssim_window_1d(patch).double()
    w = (g[:, None] * g[None, :]).reshape(1, p2, 1).to(sampled.device)
    m = mask.reshape(-1, p2, 1)
    x = sampled.reshape(-1, p2, 3)
    y = gt_rgb.to(sampled.device).reshape(-1, p2, 3)
    x = torch.where(m, x, torch.zeros_like(x)).to(wide)
    y = torch.where(m, y, torch.zeros_like(y)).to(wide)
    c1, c2 = 1e-4, 9e-4
    mx, my = (w * x).sum(1), (w * y).sum(1)
    sxx = (w * x * x).sum(1) - mx * mx
    syy = (w * y * y).sum(1) - my * my
    sxy = (w * x * y).sum(1) - mx * my
    ssim = (2 * mx * my + c1) / (mx * mx + my * my + c1) * ((2 * sxy + c2) / (sxx + syy + c2))
    return 0.05 * (1 - ssim.mean()).to(sampled.dtype)
