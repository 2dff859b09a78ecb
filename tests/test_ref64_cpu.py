"""tests/ref64.py (the float64 reference of tests/test_gemm_float64_gpu.py) evaluated in fp32 must be the oracle: sdf, grad sdf, the
feature vector and d/dx of any cotangent combination against oracle/render_ref.py::sdf_outputs + torch autograd, rgb and its four input
gradients against render_ref.colour_net (both color stages) -- to fp32 rounding, on golden models.  Then the reference is known to have
the reference's value and derivative structure before it judges a kernel."""
import pytest
import torch

import ref64
from helpers import load, params_of, oracle_config
from oracle import render_ref as R


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.999
    face = torch.randint(3, (n // 8,), generator=g)
    x[torch.arange(n // 8), face] = torch.sign(x[torch.arange(n // 8), face]) * (1 - torch.rand(n // 8, generator=g) * 1e-3)
    return x, g


def _close(a, b, what, tol=2e-5):
    """to fp32 rounding: per point, relative to that point's largest component (floor 1e-3 of the tensor's largest)"""
    a, b = a.detach().double().reshape(a.shape[0], -1), b.detach().double().reshape(b.shape[0], -1)
    scale = b.abs().amax(1, keepdim=True).clamp_min(1e-3 * float(b.abs().max()))
    err = float(((a - b).abs() / scale).max())
    assert err <= tol, f"{what}: {err:.2e}"


@pytest.mark.parametrize("name", ["full_vis_eval", "full_tracking_7scenes"])
@pytest.mark.parametrize("stage", ["coarse", "fine"])
def test_sdf_networks_equal_the_oracle_in_fp32(name, stage):
    fx = load(name)
    cfg, params = oracle_config(fx), params_of(fx)
    x, g = _points(3000, 1)
    nets = ("coarse",) if stage == "coarse" else ("coarse", "fine")
    sdf, grad, feat = ref64.sdf_forward(params, cfg, x, nets, dtype=torch.float32)
    s_o, f_o, g_o = R.sdf_outputs(params, cfg, x.clone(), stage)
    _close(sdf.unsqueeze(1), s_o, "sdf")
    _close(grad, g_o, "grad sdf")
    _close(feat, f_o, "feature")
    xs = x.clone().requires_grad_(True)
    s_o, f_o, g_o = R.sdf_outputs(params, cfg, xs, stage)
    cot = dict(g_sdf=torch.randn(x.shape[0], generator=g), g_feat=torch.randn(x.shape[0], 64, generator=g),
               g_grad=torch.randn(x.shape[0], 3, generator=g))
    outs = dict(g_sdf=s_o[:, 0], g_feat=f_o, g_grad=g_o)
    for keep in (("g_sdf",), ("g_feat",), ("g_grad",), ("g_sdf", "g_feat", "g_grad"), ("g_sdf", "g_grad")):
        obj = sum((cot[k] * outs[k]).sum() for k in keep)
        (gx_o,) = torch.autograd.grad(obj, xs, retain_graph=True)
        gx = ref64.sdf_backward(params, cfg, x, nets=nets, dtype=torch.float32, **{k: cot[k] for k in keep})
        _close(gx, gx_o, f"d/dx of {keep}")
        gx64 = ref64.sdf_backward(params, cfg, x, nets=nets, **{k: cot[k] for k in keep})
        _close(gx64, gx_o, f"d/dx of {keep}, float64 vs the fp32 oracle", 2e-3)


@pytest.mark.parametrize("name", ["full_vis_eval", "full_tracking_7scenes"])
@pytest.mark.parametrize("grid_grad", [0, 1])
def test_colour_network_equals_the_oracle_in_fp32(name, grid_grad):
    fx = load(name)
    cfg, params = oracle_config(fx), params_of(fx)
    x, g = _points(3000, 2)
    _s, feat, grad = R.sdf_outputs(params, cfg, x.clone(), "fine")
    feat, grad = feat.detach(), grad.detach()
    dirs = torch.nn.functional.normalize(torch.randn(x.shape[0], 3, generator=g), dim=-1) * 0.8
    ins = [t.clone().requires_grad_(True) for t in (x, grad, dirs, feat)]
    rgb_o = R.colour_net(params, cfg, *ins, color_stage="highfreq" if grid_grad else "base")
    _close(ref64.colour_forward(params, cfg, x, grad, dirs, feat, dtype=torch.float32), rgb_o, "rgb")
    # the ReLU kinks: points within 1e-5 of one are left out (their masks are decided by rounding)
    keep = R.colour_relu_margin(params, cfg, x, grad, dirs, feat) > 1e-5
    assert int((~keep).sum()) <= x.shape[0] // 100
    g_rgb = torch.randn(x.shape[0], 3, generator=g)
    gs_o = torch.autograd.grad((g_rgb * rgb_o).sum(), ins)
    gs = ref64.colour_backward(params, cfg, x, grad, dirs, feat, g_rgb, grid_grad, dtype=torch.float32)
    for k, go in zip(("x", "normals", "dirs", "feat"), gs_o):
        _close(gs[k][keep], go[keep], "d/d " + k)
