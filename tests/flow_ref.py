"""Float64 restatement of C ABI Section 13 (flow ground truth from depth and poses), independent of nicer_slam_amd/flow_cues.py and of
the kernels: the flow is composed through WORLD coordinates (the kernel gets one relative pose), the consistency rule goes through
torch.nn.functional.grid_sample in float64 (the kernel gathers four taps), the gather is plain indexing."""
import numpy as np
import torch
import torch.nn.functional as F


def induced_flow_ref(depth, c2w, K4, src, dst, near=1e-3):
    """depth [n, H, W] (any float type), c2w [n, 4, 4], K4 [n or 1, 4] rows (fx, fy, cx, cy) -> (flow [E, H, W, 2] float64 UNROUNDED,
    valid [E, H, W] bool)."""
    depth = np.asarray(depth)
    c2w = np.asarray(c2w, np.float64)
    K4 = np.asarray(K4, np.float64).reshape(-1, 4)
    n, H, W = depth.shape
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    flows, valids = [], []
    for i, j in zip(src, dst):
        fxi, fyi, cxi, cyi = K4[i if K4.shape[0] > 1 else 0]
        fxj, fyj, cxj, cyj = K4[j if K4.shape[0] > 1 else 0]
        raw = depth[i]
        ok = np.isfinite(raw) & (raw > 0)
        d = np.where(ok, raw, 1.0).astype(np.float64)
        cam = np.stack([(u - cxi) / fxi * d, (v - cyi) / fyi * d, d, np.ones_like(d)], -1)          # [H, W, 4]
        world = cam @ c2w[i].T
        tgt = world @ np.linalg.inv(c2w[j]).T
        ok = ok & (tgt[..., 2] > near)
        z = np.where(ok, tgt[..., 2], 1.0)
        fl = np.stack([fxj * tgt[..., 0] / z + cxj - u, fyj * tgt[..., 1] / z + cyj - v], -1)
        flows.append(np.where(ok[..., None], fl, 0.0))
        valids.append(ok)
    if not flows:
        return np.zeros((0, H, W, 2)), np.zeros((0, H, W), bool)
    return np.stack(flows), np.stack(valids)


def _warp(field, flow):
    """field [P, C, H, W] float64 sampled bilinearly at pixel + flow [P, H, W, 2], zeros outside (grid_sample, align_corners=True)."""
    P, _, H, W = field.shape
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    x = u[None] + flow[..., 0]
    y = v[None] + flow[..., 1]
    grid = torch.stack([2.0 * x / (W - 1) - 1.0, 2.0 * y / (H - 1) - 1.0], -1)
    return F.grid_sample(field, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def consistency_ref(fwd, bwd, fwd_valid=None, bwd_valid=None, alpha=0.01, beta=0.5):
    """fwd, bwd [P, H, W, 2] (taken to float64 as they are) -> (fwd_occ, bwd_occ [P, H, W] bool, fwd_margin, bwd_margin [P, H, W]
    float64): the margin is the distance of the pixel's deciding quantities from their thresholds, min(| |diff| - (alpha mag + beta) |,
    | w_inv - 1e-3 |); a pixel that is itself invalid is decided by that alone and has an infinite margin."""
    fwd = torch.as_tensor(np.asarray(fwd)).double()
    bwd = torch.as_tensor(np.asarray(bwd)).double()
    mag = fwd.norm(dim=-1) + bwd.norm(dim=-1)
    thr = alpha * mag + beta
    out = []
    for a, b, av, bv in ((fwd, bwd, fwd_valid, bwd_valid), (bwd, fwd, bwd_valid, fwd_valid)):
        wb = _warp(b.permute(0, 3, 1, 2), a).permute(0, 2, 3, 1)
        diff = (a + wb).norm(dim=-1)
        occ = diff > thr
        margin = (diff - thr).abs()
        if av is not None:
            av = torch.as_tensor(np.asarray(av)).bool()
            bv = torch.as_tensor(np.asarray(bv)).bool()
            w_inv = _warp((~bv).double()[:, None], a)[:, 0]
            occ = occ | (w_inv > 1e-3) | ~av
            margin = torch.minimum(margin, (w_inv - 1e-3).abs())
            margin = torch.where(av, margin, torch.full_like(margin, float("inf")))
        out.append((occ.numpy(), margin.numpy()))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def select_ref(flows, masks, sampling_idx, idii):
    """flows [E, HW, 2], masks [E, HW] bool, sampling_idx [b, n], idii [E] (torch, any device) -> ([E, n, 2], [E, n] bool); an index
    outside [0, HW) gives 0 / false."""
    E, HW, _ = flows.shape
    s = sampling_idx[idii]                                                  # [E, n]
    ok = (s >= 0) & (s < HW)
    sc = torch.where(ok, s, torch.zeros_like(s))
    e = torch.arange(E, device=flows.device)[:, None].expand_as(sc)
    f = torch.where(ok[..., None], flows[e, sc], torch.zeros((), dtype=flows.dtype, device=flows.device))
    return f, masks[e, sc] & ok
