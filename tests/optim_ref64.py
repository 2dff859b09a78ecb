"""A float64 restatement of the kernels that turn gradients into parameters (test infrastructure): the Adam steps of csrc/map_tail.hip
and csrc/track_tail.hip, the flat weight norm and its backward, the tracker's two reductions (composed from tests/objective_ref64.py),
and exact numpy float32 statements of the voxel index and the Morton key.

``adam_step(..., dtype=torch.float64)`` is the reference; ``dtype=torch.float32`` is the yardstick of tests/test_optim_float64_gpu.py, in
one of two documented operation orders:
  order="table"   the comment above adam_one in map_tail.hip (torch's foreach Adam): m = m0 + w1 (g - m0); v = v0 b2 + (w2 g) g;
                  denom = sqrt(v) / fl(sqrt(bc2)) + eps; p = p0 - step_size (m / denom), step_size = fl(lr / bc1);
  order="camera"  adam_one of track_tail.hip: m = b1 m0 + (1 - b1) g; v = b2 v0 + ((1 - b2) g) g; the StepLR factor formed in double and
                  rounded, lr = fl(lr fl(gamma^k)); p = p0 - (step_size m) / denom.
Hyper-parameters are rounded to fp32 first, as the C ABI receives them; bc1 = 1 - b1^t, bc2 = 1 - b2^t and lr / bc1 are formed in double
from those fp32 values in every mode, as the host code (and the camera kernel) forms them.  tests/test_optim_ref64_cpu.py holds the float64
mode to torch.optim.Adam on float64 tensors and the fp32 mode to torch's fp32 Adam."""
import math

import numpy as np
import torch

import objective_ref64 as O

F64 = torch.float64
F32 = torch.float32


def f32(x):
    """a Python float rounded to fp32, as a C float argument arrives"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------ Adam
def step_lr_exponent(t, lr_step):
    """StepLR as the training loop drives it (scheduler.step() after optimizer.step()): step t (1-based) runs at gamma^floor((t-1)/lr_step)"""
    return (t - 1) // lr_step if lr_step else 0


def adam_step(p0, g, m0, v0, t, lr, b1, b2, eps, lr_step=0, lr_gamma=1.0, dtype=F64, order="table"):
    """one Adam step from the state (p0, m0, v0) with gradient g, step number t >= 1 -> (m, v, p) in ``dtype``; torch's semantics
    (no weight decay, no amsgrad): denom = sqrt(v) / sqrt(bc2) + eps, p -= lr / bc1 * m / denom."""
    assert t >= 1 and order in ("table", "camera")
    lr, b1, b2, eps, lr_gamma = f32(lr), f32(b1), f32(b2), f32(eps), f32(lr_gamma)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    k = step_lr_exponent(t, lr_step)
    p0, g, m0, v0 = (x.to(dtype) for x in (p0, g, m0, v0))
    if dtype == F64:
        lr_t = lr * lr_gamma ** k
        m = b1 * m0 + (1.0 - b1) * g
        v = b2 * v0 + (1.0 - b2) * g * g
        denom = v.sqrt() / math.sqrt(bc2) + eps
        return m, v, p0 - (lr_t / bc1) * m / denom
    assert dtype == F32
    w1, w2 = f32(1.0 - b1), f32(1.0 - b2)                     # (exact: b1, b2 in [0.5, 1) or 0)
    lr_t = f32(lr * f32(lr_gamma ** k)) if lr_step else lr
    step_size, bc2_sqrt = f32(lr_t / bc1), f32(math.sqrt(bc2))
    if order == "table":
        m = m0 + w1 * (g - m0)
        v = v0 * b2 + (w2 * g) * g
        p = p0 - step_size * (m / (v.sqrt() / bc2_sqrt + eps))
    else:
        m = b1 * m0 + w1 * g
        v = b2 * v0 + (w2 * g) * g
        p = p0 - (step_size * m) / (v.sqrt() / bc2_sqrt + eps)
    return m, v, p


def zero_grad_step(p0, m0, v0, t, lr, b1, b2, eps, dtype=F64):
    """the step of a parameter that received no gradient: adam_step with g = 0 (both moments decay, the parameter moves on)"""
    return adam_step(p0, torch.zeros_like(p0), m0, v0, t, lr, b1, b2, eps, dtype=dtype)


def keep_best(losses, cams, start=1e10):
    """the arg-min-loss candidate of a frame: after every step, (smallest loss so far, camera AFTER the step that produced it); strict <
    (a NaN loss never wins), start 1e10.  losses: fp32 scalars, cams: the stepped cameras -> [(best_loss, best_cam or None)] per step"""
    best, cam, out = np.float32(start), None, []
    for l, c in zip(losses, cams):
        if np.float32(l) < best:
            best, cam = np.float32(l), c
        out.append((best, cam))
    return out


# ------------------------------------------------------------------------------------------------------------------ weight norm
def weight_norm_flat(layers, dtype=F64, kernel_order=False):
    """layers: [(v [rows,cols], g [rows], bias [rows])] -> (flat = [W_0, b_0, W_1, b_1, .., 0], norms [total rows]) with
    W[r,:] = v[r,:] g[r] / ||v[r,:]||.  kernel_order (fp32): v g (1 / ||v||), the order of ATen's weight_norm kernel."""
    parts, norms = [], []
    for v, g, b in layers:
        v, g = v.to(dtype), g.to(dtype)
        n = (v * v).sum(1).sqrt()
        w = v * g[:, None] * (1 / n)[:, None] if kernel_order else v * g[:, None] / n[:, None]
        parts += [w.reshape(-1), b.to(dtype)]
        norms.append(n)
    return torch.cat(parts + [torch.zeros(1, dtype=dtype)]), torch.cat(norms)


def weight_norm_flat_backward(layers, g_flat, dtype=F64, kernel_order=False, drop_projection=False):
    """-> per layer [g_v (rows x cols) | g_g (rows) | g_bias (rows)], concatenated:
    g_g[r] = <gW[r], v[r]> / ||v||,  g_v[r] = g[r] (gW[r] / ||v|| - v[r] <gW[r], v[r]> / ||v||^3),  g_bias = its slice.
    kernel_order (fp32): with rn = 1 / ||v||:  g (rn gW - (rn rn rn) v s).  drop_projection: the mutant without the second term."""
    out, off = [], 0
    for v, g, _b in layers:
        rows, cols = v.shape
        v, g = v.to(dtype), g.to(dtype)
        gw = g_flat[off:off + rows * cols].to(dtype).reshape(rows, cols)
        gb = g_flat[off + rows * cols:off + rows * cols + rows].to(dtype)
        off += rows * cols + rows
        n = (v * v).sum(1).sqrt()
        s = (gw * v).sum(1)
        if kernel_order:
            rn = 1 / n
            g_v = g[:, None] * (rn[:, None] * gw - (rn * rn * rn)[:, None] * v * s[:, None])
            g_g = s * rn
        else:
            g_v = g[:, None] * (gw / n[:, None] - v * (s / n ** 3)[:, None])
            g_g = s / n
        if drop_projection:
            g_v = g[:, None] * gw / n[:, None]
        out += [g_v.reshape(-1), g_g, gb]
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------------------------ tracker reductions
def per_ray_cam_terms(uv, K, cam, g_o, g_d, dtype=F64):
    """[R,7]: every ray's own contribution to d/d cam of sum_r (g_o . rays_o + g_d . rays_d) -- each ray lifted as an image of its own"""
    R = uv.shape[0]
    r = O.rays(uv.reshape(R, 1, 2), cam.reshape(1, 7).repeat(R, 1), K.reshape(1, 4, 4).repeat(R, 1, 1), dtype)
    return O.rays_pose_backward(r, g_o.reshape(R, 1, 3), g_d.reshape(R, 1, 3))


def _message(g7, slot7, weight, dtype, scale_slot7=True):
    out = torch.cat([g7, torch.as_tensor([slot7], dtype=dtype)])
    if weight > 0:
        w = torch.tensor(f32(weight), dtype=dtype)
        out = torch.cat([out[:7] * w, out[7:] * w if scale_slot7 else out[7:], w.reshape(1)])
    return out


def track_tail_g_cam(uv, K, cam, g_o, g_d, weight=0.0, slot7=0.0, dtype=F64, scale_slot7=True):
    """nsa_track_tail's g_cam: d/d cam [7] of sum_r (g_o . rays_o + g_d . rays_d), then slot 7 (the rank's loss, written by the caller
    before the launch).  weight > 0: slots 0..7 times the weight and slot 8 = the weight -> [9]; else [8] with slot 7 untouched."""
    r = O.rays(uv[None], cam[None], K[None], dtype)
    g7 = O.rays_pose_backward(r, g_o, g_d)[0]
    return _message(g7, torch.as_tensor(slot7).to(dtype), weight, dtype, scale_slot7)


def track_finish_red(uv, K, cam, z, g_x, g_dir, ray_loss, weight=0.0, dtype=F64):
    """nsa_track_finish's message: rays_backward over the samples, the same pose reduction, and slot 7 = sum(ray_loss) / (3 R)"""
    g_o, g_d = O.rays_backward(z, g_x, g_dir, dtype)
    r = O.rays(uv[None], cam[None], K[None], dtype)
    g7 = O.rays_pose_backward(r, g_o, g_d)[0]
    loss = ray_loss.to(dtype).sum() / (3 * uv.shape[0])
    return _message(g7, loss, weight, dtype)


# ------------------------------------------------------------------------------------------------------------------ voxels and keys
_f = np.float32


def voxel_index(x, res):
    """x [P,3] float32 -> int64 [P]: the flat voxel of every point, -1 where it is skipped (|x_d| > 0.99f in any d).  Every operation
    of ((x + 1) / 2 * res) rounded to fp32, then truncated: exact."""
    x = np.asarray(x, dtype=_f)
    assert not np.isnan(x).any(), "the cast of a NaN is not defined"
    skip = (np.abs(x) > _f(0.99)).any(1)
    q = (((x + _f(1.0)) / _f(2.0)) * _f(res)).astype(_f).astype(np.int64)
    flat = q[:, 0] * res * res + q[:, 1] * res + q[:, 2]
    ok = ~skip & (flat >= 0) & (flat < res ** 3)
    return np.where(ok, flat, -1)


def voxel_counts(x, res):
    idx = voxel_index(x, res)
    out = np.zeros(res ** 3, dtype=_f)
    np.add.at(out, idx[idx >= 0], _f(1.0))
    return out


def _spread10(v):
    v = v & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton_key(x):
    """x [P,3] float32 -> int32 [P]: 30-bit Morton code of min(max((x + 1) 512, 0), 1023) truncated; a NaN coordinate gives cell 0"""
    x = np.asarray(x, dtype=_f)
    with np.errstate(invalid="ignore"):
        u = np.fmin(np.fmax(((x + _f(1.0)) * _f(512.0)).astype(_f), _f(0.0)), _f(1023.0))
    c = u.astype(np.uint32)
    return (_spread10(c[:, 0]) | (_spread10(c[:, 1]) << np.uint32(1)) | (_spread10(c[:, 2]) << np.uint32(2))).astype(np.int32)
