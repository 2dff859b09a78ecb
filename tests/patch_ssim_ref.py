"""float64 oracle for the SSIM form of the patch-warp term (C ABI section 5 nsa_patch_ssim, csrc/patch_ssim.hip), in
two independent forms:

* ``direct``: a direct 2-D window per patch with the closed-form gradient;
* ``conv_form``: pytorch_msssim's shape -- the separable window as two grouped ``conv2d`` passes (valid, so one value per patch
  and channel), sigma^2 = E[x^2] - mu^2, the gradient by autograd -- in any dtype on any device.

Definition: pred = x, target = y [N, p^2, 3], mask [N, p^2]; x and y count as 0 where the mask is false; the 1-D window is
g_k = fp32 exp of the fp32 argument -(k - p//2)^2 / 4.5 divided by the correctly rounded fp32 sum; w_ij = g_i g_j exactly;
SSIM = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * (2 s_xy + C2) / (s_xx + s_yy + C2); loss = 1 - mean SSIM over the 3 N
values; the reference's term is 0.05 * loss.
"""
import math

import numpy as np
import torch

C1, C2 = 1e-4, 9e-4


def window_1d(p):
    """fp32 [p]: exp at the fp32 arguments, rounded to fp32, divided by their fp32 sum (the float64 sum of these few fp32
    values is exact, so its rounding is the correctly rounded sum)."""
    d = np.arange(p, dtype=np.float32) - np.float32(p // 2)
    arg = (-(d * d) / np.float32(4.5)).astype(np.float32)
    g = np.array([math.exp(float(a)) for a in arg], dtype=np.float32)
    s = np.float32(g.astype(np.float64).sum())
    return (g / s).astype(np.float32)


def window_2d(p):
    """float64 [p * p]: the exact products of the fp32 1-D weights, pixel i * p + j."""
    g = window_1d(p).astype(np.float64)
    return np.outer(g, g).reshape(-1)


def _zeroed(pred, target, mask, p, dtype, device):
    x = torch.as_tensor(pred).to(device=device, dtype=dtype).reshape(-1, p * p, 3)
    y = torch.as_tensor(target).to(device=device, dtype=dtype).reshape(-1, p * p, 3)
    if mask is None:
        m = torch.ones(x.shape[:2], dtype=torch.bool, device=device)
    else:
        m = torch.as_tensor(mask).to(device).reshape(-1, p * p) != 0
    return x, y, m


def direct(pred, target, mask, p):
    """-> (loss, ssim [N, 3], d loss / d pred [N, p^2, 3]) in float64 (a python float and CPU tensors)."""
    x, y, m = _zeroed(pred, target, mask, p, torch.float64, "cpu")
    x = torch.where(m[..., None], x, torch.zeros_like(x))
    y = torch.where(m[..., None], y, torch.zeros_like(y))
    n = x.shape[0]
    w = torch.from_numpy(window_2d(p))[None, :, None]
    mx, my = (w * x).sum(1, keepdim=True), (w * y).sum(1, keepdim=True)
    sxx = (w * x * x).sum(1, keepdim=True) - mx * mx
    syy = (w * y * y).sum(1, keepdim=True) - my * my
    sxy = (w * x * y).sum(1, keepdim=True) - mx * my
    dA, dB = mx * mx + my * my + C1, sxx + syy + C2
    A, B = (2 * mx * my + C1) / dA, (2 * sxy + C2) / dB
    ssim = (A * B).reshape(n, 3)
    d_ssim = w * (B * (2 * my - 2 * mx * A) / dA + A * (2 * (y - my) - 2 * B * (x - mx)) / dB)
    grad = -(d_ssim * m[..., None]) / (3 * n) if n else d_ssim
    return float(1.0 - ssim.mean()) if n else math.nan, ssim, grad


def conv_form(pred, target, mask, p, dtype=torch.float64, device="cpu"):
    """-> (loss, d loss / d pred [N, p^2, 3]) as tensors of ``dtype`` on ``device``: two grouped conv2d passes and autograd."""
    x, y, m = _zeroed(pred, target, mask, p, dtype, device)
    x = x.clone().requires_grad_(True)
    zero = torch.zeros((), dtype=dtype, device=device)
    img = lambda t: torch.where(m[..., None], t, zero).reshape(-1, p, p, 3).permute(0, 3, 1, 2)
    X, Y = img(x), img(y)
    win = torch.from_numpy(window_1d(p)).to(device=device, dtype=dtype).reshape(1, 1, 1, p).repeat(3, 1, 1, 1)

    def blur(t):
        t = torch.nn.functional.conv2d(t, win.transpose(2, 3), groups=3)
        return torch.nn.functional.conv2d(t, win, groups=3)
    mu1, mu2 = blur(X), blur(Y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(X * X) - mu1_sq, blur(Y * Y) - mu2_sq, blur(X * Y) - mu1_mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs
    loss = 1 - ssim.flatten(2).mean(-1).mean()
    loss.backward()
    return loss.detach(), x.grad


def term(pred, target, mask, p):
    """0.05 * (1 - mean SSIM) in float64."""
    return 0.05 * direct(pred, target, mask, p)[0]


def ulp32(v):
    """One fp32 unit in the last place at |v| (float64)."""
    return float(np.spacing(np.float32(abs(v))))
