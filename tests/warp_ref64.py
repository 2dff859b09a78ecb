"""A float64 restatement of the keyframe re-projection blocks with autograd (test infrastructure): patch warp, flow and the masked L1
mean of csrc/warp_terms.hip (C ABI section 5; reference code/model/network.py:153-279, code/utils/general.py:129-145,
code/model/loss.py:106-111,136-142).  Plain torch, ``dtype=torch.float64`` by default; ``dtype=torch.float32`` evaluates the same graph
in fp32 (the yardstick of tests/test_warp_float64_gpu.py; tests/test_warp_ref64_cpu.py holds that mode to model/warp.py and to the
golden ``reproj_blocks``).  Inputs are the explicit fp32 tensors the kernels see; ``w2c`` is an INDEPENDENT leaf (the kernels take it
as an input of its own and return its gradient separately from the pose's).

Geometry, as the header of warp_terms.hip states it: c = lift(K_s, u, v, 1) with skew; w = (P_s [c,1]) - o, d = w / |w|^2;
x = o + depth d; q = W_t [x,1]; pr = K_t[:3,:3] q; (tu, tv) = pr.xy / (pr.z + 1e-8).  The bilinear sample is written out (no
F.grid_sample) so that the texel cell (x0, y0) and the pixel coordinates (ix, iy) of every sample are returned: zeros outside the
image, align_corners=True on the normalised grid gx = tu / W * 2 - 1, ix = (gx + 1) / 2 * (W - 1).

What is DISCRETE is taken from the fp32 inputs and enters as data: the patch pixel (u, v) = uv + cell offset (an exact fp32 sum for
the coordinates used), its truncation for the patch read, and the ``inside`` test.  The texel cell floor(ix), the three mask
comparisons and the flatness test are decided in ``dtype``: they are what the exclusions of the GPU test are about."""
from collections import namedtuple

import numpy as np
import torch

from objective_ref64 import F64, _lift

F32 = torch.float32
OK_LIMIT = 1.0e8                                   # bilinear_setup: coordinates at or beyond it (or non-finite) sample nothing
FLAT_LIMIT = float(np.float32(0.01))               # `var < 0.01` on an fp32 tensor compares with fl32(0.01), in torch and in the kernel


def cell_offsets(patch):
    """[p2, 2] fp32: cell c = (c // p, c % p) -> (du, dv) = (c // p - half, c % p - half)   (general.py:139-144, indexing="ij")"""
    half = patch // 2
    c = torch.arange(patch * patch)
    return torch.stack([(c // patch - half), (c % patch - half)], -1).to(F32)


def patch_pixels(uv, patch):
    """uv [b,n,2] fp32 -> (u, v) [b,n,p2] fp32 (the kernel's fp32 sum) and inside [b,n,p2] for an image of any size via ``inside_of``"""
    assert uv.dtype == F32
    off = cell_offsets(patch)
    return uv[:, :, None, 0] + off[None, None, :, 0], uv[:, :, None, 1] + off[None, None, :, 1]


def inside_of(u, v, H, W):
    return (u >= 0) & (v >= 0) & (u < W) & (v < H)


Geometry = namedtuple("Geometry", "c w x q tz tu tv")


def geometry(u, v, pose, w2c, K, depth, targets=None, sources=None):
    """u, v [b,m] and depth [b,m] (any float dtype, all the same), pose / w2c / K [b,4,4] in that dtype.
    targets None: every source against every target -> q [b_t,b_s,m,3], tz / tu / tv [b_t,b_s,m];
    targets / sources (index tensors [ne]): pairs -> q [ne,m,3], tz / tu / tv [ne,m]."""
    x_l, y_l = _lift(torch.stack([u, v], -1), K)
    c = torch.stack([x_l, y_l, torch.ones_like(x_l)], -1)
    pts = torch.cat([c, torch.ones_like(x_l)[..., None]], -1).permute(0, 2, 1)
    w = torch.bmm(pose, pts).permute(0, 2, 1)[:, :, :3] - pose[:, None, :3, 3]
    d = w / (w * w).sum(-1, keepdim=True)                                   # divided by the SQUARED norm
    x = pose[:, None, :3, 3] + depth[..., None] * d                         # [b,m,3]
    if targets is None:
        q = torch.einsum("tkj,smj->tsmk", w2c[:, :3, :3], x) + w2c[:, None, None, :3, 3]
        pr = torch.einsum("tkj,tsmj->tsmk", K[:, :3, :3], q)
    else:
        q = torch.einsum("ekj,emj->emk", w2c[targets][:, :3, :3], x[sources]) + w2c[targets][:, None, :3, 3]
        pr = torch.einsum("ekj,emj->emk", K[targets][:, :3, :3], q)
    tz = pr[..., 2]
    den = tz + 1e-8
    return Geometry(c, w, x, q, tz, pr[..., 0] / den, pr[..., 1] / den)


def frames_of(images, frame_index, b):
    """[b, H*W, C]: the frame of every batch entry (frame_index None: entry i reads frame i)"""
    return images[:b] if frame_index is None else images.index_select(0, frame_index.long())


Warp = namedtuple("Warp", "sampled mask gt_rgb flat var ix iy gx gy tz x0 y0 ok inside geo leaves")


def patch_warp(uv, pose, w2c, K, depth, images, depths, frame_index, H, W, patch, dtype=F64, leaves=None):
    """uv [b,n,2], pose / w2c / K [b,4,4], depth [b,n], images [frames,H*W,3], depths [frames,H*W,1] or None (patch 1), all fp32.
    -> Warp(sampled [b_t,b_s,n,p2,3], mask [b_t,b_s,n,p2], gt_rgb [b_t,b_s,n,p2,3] fp32, flat [b_s,n] (None for patch 1),
            var [b_s,n] the biased variance behind flat, per sample ix, iy, gx, gy, tz [b_t,b_s,n,p2] (detached), x0, y0 (int64), ok,
            inside [b_s,n,p2], geo (the graph's intermediates), leaves = (depth, pose, w2c) in ``dtype``)
    leaves: (depth [b,n], pose, w2c) tensors of ``dtype`` that already belong to a graph, used in place of fresh leaves"""
    assert all(t.dtype == F32 for t in (uv, K, images)) and (leaves is not None or all(t.dtype == F32 for t in (pose, w2c, depth)))
    b, n = uv.shape[0], uv.shape[1]
    p2 = patch * patch
    u, v = patch_pixels(uv, patch)                                          # fp32, [b,n,p2]
    inside = inside_of(u, v, H, W)
    if leaves is None:
        leaves = tuple(t.detach().to(dtype).requires_grad_(True) for t in (depth.reshape(b, n), pose, w2c))
    dl, pl, wl = leaves
    g = geometry(u.reshape(b, -1).to(dtype), v.reshape(b, -1).to(dtype), pl, wl, K.to(dtype),
                 dl[:, :, None].expand(b, n, p2).reshape(b, -1))
    shape = (b, b, n, p2)
    tz, tu, tv = g.tz.reshape(shape), g.tu.reshape(shape), g.tv.reshape(shape)
    gx, gy = tu / W * 2 - 1.0, tv / H * 2 - 1.0                             # network.py:213-215
    ix, iy = (gx + 1.0) / 2.0 * (W - 1), (gy + 1.0) / 2.0 * (H - 1)
    ok = (ix.detach().abs() < OK_LIMIT) & (iy.detach().abs() < OK_LIMIT)    # (false for NaN as well)
    fx = torch.where(ok, ix.detach().floor(), torch.zeros_like(ix.detach()))
    fy = torch.where(ok, iy.detach().floor(), torch.zeros_like(iy.detach()))
    x0, y0 = fx.long(), fy.long()
    img = frames_of(images, frame_index, b).reshape(b, H * W, 3).to(dtype)
    t_of = torch.arange(b)[:, None, None, None].expand(shape)

    def texel(x, y):
        good = ok & (x >= 0) & (y >= 0) & (x < W) & (y < H)
        val = img[t_of, (y.clamp(0, H - 1) * W + x.clamp(0, W - 1))]
        return torch.where(good[..., None], val, torch.zeros_like(val))

    fx1, fy1, fx0, fy0 = (fx + 1.0) - ix, (fy + 1.0) - iy, ix - fx, iy - fy
    sampled = (texel(x0, y0) * (fx1 * fy1)[..., None] + texel(x0 + 1, y0) * (fx0 * fy1)[..., None]
               + texel(x0, y0 + 1) * (fx1 * fy0)[..., None] + texel(x0 + 1, y0 + 1) * (fx0 * fy0)[..., None])
    tmask = (gx > -1) & (gx < 1) & (gy > -1) & (gy < 1) & (tz > 0)          # network.py:224-230
    # the patch itself, read from its own image; ones outside (network.py:240-253); .long() truncates a fractional coordinate
    pix = (v.long().clamp(0, H - 1) * W + u.long().clamp(0, W - 1))
    s_of = torch.arange(b)[:, None, None].expand(b, n, p2)
    own = frames_of(images, frame_index, b).reshape(b, H * W, 3)[s_of, pix]
    gt = torch.where(inside[..., None], own, torch.ones_like(own))
    gt_rgb = gt[None].expand(b, b, n, p2, 3).contiguous()
    mask = tmask.detach() & inside[None]
    flat = var = None
    if patch > 1:
        own_d = frames_of(depths, frame_index, b).reshape(b, H * W)[s_of, pix]
        dd = torch.where(inside, own_d, torch.ones_like(own_d)).to(dtype)
        mean = dd.sum(-1, keepdim=True) / p2
        var = ((dd - mean) ** 2).sum(-1) / p2                               # biased (network.py:259-270)
        flat = var < FLAT_LIMIT
        mask = mask & flat[None, :, :, None]
    det = lambda t: t.detach()
    return Warp(sampled, mask, gt_rgb, flat, var, det(ix), det(iy), det(gx), det(gy), det(tz), x0, y0, ok, inside, g, leaves)


def flat_bound(var, depths_max, p2):
    """How far an fp32 evaluation of the biased variance of p2 values of size <= depths_max may lie from ``var``: the mean carries
    (p2 + 1) roundings of relative size u = 2^-24 on values of size depths_max, each difference one more, the squares and their sum
    p2 + 2 more: |d var| <= (p2 + 3) u (2 sqrt(var) depths_max + var) to first order."""
    return (p2 + 3) * 2.0 ** -24 * (2 * var.double().clamp_min(0).sqrt() * depths_max + var.double())


def backward(out_tensor, leaves, cot):
    """d/d (depth, pose, w2c) of  cot . out_tensor  (float64 or fp32 autograd, whatever the graph is in)"""
    obj = (cot.to(out_tensor.dtype).reshape(out_tensor.shape) * out_tensor).sum()
    if not obj.requires_grad:
        return tuple(torch.zeros_like(t) for t in leaves)
    gs = torch.autograd.grad(obj, leaves, allow_unused=True, retain_graph=True)
    return tuple(torch.zeros_like(t) if g is None else g for g, t in zip(gs, leaves))


Flow = namedtuple("Flow", "flow tz geo leaves")


def flow(uv, pose, w2c, K, depth, idii, idjj, dtype=F64, leaves=None):
    """-> Flow(flow [ne,n,2] = (tu, tv) of pixel i of frame idii[e] in frame idjj[e], minus the pixel; tz [ne,n]; leaves)"""
    assert uv.dtype == K.dtype == F32
    b, n = uv.shape[0], uv.shape[1]
    if leaves is None:
        leaves = tuple(t.detach().to(dtype).requires_grad_(True) for t in (depth.reshape(b, n), pose, w2c))
    dl, pl, wl = leaves
    ii, jj = idii.long(), idjj.long()
    uvd = uv.to(dtype)
    g = geometry(uvd[..., 0], uvd[..., 1], pl, wl, K.to(dtype), dl, targets=jj, sources=ii)
    fl = torch.stack([g.tu, g.tv], -1) - uvd[ii]
    return Flow(fl, g.tz.detach(), g, leaves)


def masked_l1(pred, target, mask, ch):
    """What nsa_masked_l1 documents: |pred - target| formed in fp32, summed in float64, divided by count * ch.
    pred, target [items, ch] fp32, mask [items] bool or None -> (loss float64 scalar, g_pred [items, ch] fp32 = sign(d) fl32(1 / (count ch))
    where selected, 0 elsewhere and on ties)"""
    assert pred.dtype == target.dtype == F32
    items = pred.shape[0]
    m = torch.ones(items, dtype=torch.bool) if mask is None else mask.bool()
    d = pred - target                                                        # fp32
    count = int(m.sum())
    total = d.abs().double()[m].sum()
    loss = total / (count * ch) if count else torch.tensor(float("nan"), dtype=F64)
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(count * ch), dtype=F32) if count else torch.tensor(0.0)
    g = torch.where(m[:, None], d.sign() * inv, torch.zeros_like(d))
    return loss, g


def masked_l1_float64(pred, target, mask, ch):
    """The mean and its gradient wholly in float64 (the differences NOT rounded to fp32 first)"""
    m = torch.ones(pred.shape[0], dtype=torch.bool) if mask is None else mask.bool()
    d = pred.double() - target.double()
    count = int(m.sum())
    if not count:
        return torch.tensor(float("nan"), dtype=F64), torch.zeros_like(d)
    return d.abs()[m].sum() / (count * ch), torch.where(m[:, None], d.sign() / (count * ch), torch.zeros_like(d))


# ------------------------------------------------------------------------------------------------------------------ kernel order
def _butterfly(v):
    """v [..., 64] -> [...]: the wave sum `for off in 32, 16, .., 1: x += shfl_xor(x, off)` as lane 0 forms it"""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def _strided_groups(parts):
    """parts [waves, 12] fp32, in the order k_pose_finish walks them -> [12]: group g adds waves g, g + 21, ... in turn, then the 21
    groups are added in turn"""
    waves = parts.shape[0]
    pad = (-waves) % 21
    p = torch.cat([parts, torch.zeros(pad, parts.shape[1], dtype=parts.dtype)]).reshape(-1, 21, parts.shape[1])
    acc = torch.zeros(21, parts.shape[1], dtype=parts.dtype)
    for r in range(p.shape[0]):
        acc = acc + p[r]
    out = torch.zeros(parts.shape[1], dtype=parts.dtype)
    for g in range(21):
        out = out + acc[g]
    return out


def _wave_partials(per_thread):
    """per_thread [b_s, threads, 12] -> [b_s, waves_per_image, 12]: threads padded with zeros to whole 256-thread blocks"""
    b, m, _ = per_thread.shape
    pad = (-m) % 256
    t = torch.cat([per_thread, torch.zeros(b, pad, 12, dtype=per_thread.dtype)], 1)
    return _butterfly(t.reshape(b, -1, 64, 12).permute(0, 1, 3, 2))


def pose_grads_kernel_order(geo, obj, per_source, slot_source_mask=None, slot_target=None):
    """A SECOND fp32 evaluation of g_pose and g_w2c, in the summation order warp_terms.hip documents: a thread owns one (source,
    pixel, cell) and forms its 12 + 12 products; a wave adds its 64 threads by the xor butterfly; k_pose_finish adds the wave
    partials in 21 strided groups and the groups in turn.  The per-thread cotangents of q, x and w come from fp32 autograd on the
    fp32 graph (``geo`` of an F32 evaluation, ``obj`` its scalar objective); only the ORDER of the sums over threads is the kernel's.

    per_source = m threads per image.  Patch warp: slots are the targets (geo.q [b_t,b_s,m,3]).  Flow: slots are the edges (geo.q
    [ne,m,3]); slot_source_mask [ne,b] says which source's threads carry slot e (the others add zeros), slot_target [ne].
    -> g_pose [b,4,4], g_w2c [b,4,4] fp32"""
    gq, gx, gw = torch.autograd.grad(obj, (geo.q, geo.x, geo.w), retain_graph=True, allow_unused=True)
    b, m = geo.x.shape[0], per_source
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    gq, gx, gw = zero(gq, geo.q), zero(gx, geo.x), zero(gw, geo.w)
    c = geo.c.detach()
    src = torch.cat([gw[..., :, None] * c[..., None, :], gx[..., :, None]], -1).reshape(b, m, 12)       # gP[4k+j] = gw_k c_j, gP[4k+3] = gx_k
    part_src = _wave_partials(src)                                                                  # [b, wpi, 12]
    g_pose = torch.zeros(b, 4, 4, dtype=F32)
    for s in range(b):
        g_pose[s, :3] = _strided_groups(part_src[s]).reshape(3, 4)
    x = geo.x.detach()
    g_w2c = torch.zeros(b, 4, 4, dtype=F32)
    if slot_target is None:                                                                         # patch warp: slot == target
        per = torch.cat([gq[..., :, None] * x[None, ..., None, :], gq[..., :, None]], -1).reshape(b, b, m, 12)   # [t, s, m, 12]
        for t in range(b):
            parts = _wave_partials(per[t])                                                          # [b_s, wpi, 12] = wave_global order
            g_w2c[t, :3] = _strided_groups(parts.reshape(-1, 12)).reshape(3, 4)
        return g_pose, g_w2c
    ne = gq.shape[0]
    acc = torch.zeros(b, 21, 12, dtype=F32)
    for e in range(ne):
        s = int(slot_source_mask[e].nonzero()[0])
        per = torch.zeros(b, m, 12, dtype=F32)
        per[s] = torch.cat([gq[e][:, :, None] * x[s][:, None, :], gq[e][:, :, None]], -1).reshape(m, 12)
        parts = _wave_partials(per).reshape(-1, 12)
        waves = parts.shape[0]
        p = torch.cat([parts, torch.zeros((-waves) % 21, 12)]).reshape(-1, 21, 12)
        t = int(slot_target[e])
        for r in range(p.shape[0]):                                                                 # (acc runs on across the slots of a target)
            acc[t] = acc[t] + p[r]
    for t in range(b):
        out = torch.zeros(12, dtype=F32)
        for g in range(21):
            out = out + acc[t, g]
        g_w2c[t, :3] = out.reshape(3, 4)
    return g_pose, g_w2c
