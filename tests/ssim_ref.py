"""float64 numpy oracle for the rendering metrics (C ABI Section 9, csrc/image_metrics.hip).

SSIM is code/utils/SSIM with size_average=True restated in float64 with a direct 2-D window: the 1-D window is built the
reference's way in fp32 (fp32 values of the Gaussian, divided by their fp32 sum), and the 2-D weights are the EXACT float64
products g_i * g_j (the reference rounds them to fp32).  PSNR is rend_util.get_psnr's -10 log10(mse) in float64.
"""
import math

import numpy as np

RADIUS = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_1d():
    """fp32 [11]: exp(-(k - 5)^2 / (2 * 1.5^2)) rounded to fp32, divided by their fp32 sum.  The sum is the correctly rounded
    one (the float64 sum of these 11 values is exact), which is what torch's sum gives for the reference's gaussian()."""
    g = np.array([math.exp(-((k - RADIUS) ** 2) / float(2 * 1.5 ** 2)) for k in range(2 * RADIUS + 1)], dtype=np.float32)
    s = np.float32(g.astype(np.float64).sum())
    return (g / s).astype(np.float32)


def window_2d():
    """float64 [11, 11]: the exact products of the fp32 1-D weights."""
    g = window_1d().astype(np.float64)
    return np.outer(g, g)


def _filter(img, w):
    """img [H, W] float64, zero padding RADIUS: out[r, c] = sum_ij w[i, j] img[r + i - 5, c + j - 5]."""
    H, W = img.shape
    p = np.zeros((H + 2 * RADIUS, W + 2 * RADIUS))
    p[RADIUS:RADIUS + H, RADIUS:RADIUS + W] = img
    out = np.zeros((H, W))
    for i in range(2 * RADIUS + 1):
        for j in range(2 * RADIUS + 1):
            out += w[i, j] * p[i:i + H, j:j + W]
    return out


def ssim_map(pred, gt):
    """pred, gt [H, W, 3] (any float dtype, converted to float64) -> float64 [H, W, 3] per-channel SSIM map."""
    x = np.asarray(pred, dtype=np.float64)
    y = np.asarray(gt, dtype=np.float64)
    w = window_2d()
    out = np.empty(x.shape)
    for c in range(x.shape[2]):
        xc, yc = x[..., c], y[..., c]
        mx, my = _filter(xc, w), _filter(yc, w)
        exx, eyy, exy = _filter(xc * xc, w), _filter(yc * yc, w), _filter(xc * yc, w)
        mxx, myy, mxy = mx * mx, my * my, mx * my
        sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
        out[..., c] = ((2 * mxy + C1) * (2 * sxy + C2)) / ((mxx + myy + C1) * (sxx + syy + C2))
    return out


def ssim(pred, gt):
    """Mean SSIM over the 3 channels and all pixels (float64)."""
    return float(ssim_map(pred, gt).mean())


def sq_err_sum(pred, gt):
    d = np.asarray(pred, dtype=np.float64) - np.asarray(gt, dtype=np.float64)
    return float((d * d).sum())


def psnr(pred, gt):
    mse = sq_err_sum(pred, gt) / np.asarray(pred).size
    return math.inf if mse == 0 else -10.0 * math.log10(mse)
