"""tests/ref64.py's PER-POINT weight gradients (sdf_weight_grads, colour_weight_grads: the reference of the emission-row gates of
tests/test_gemm_float64_gpu.py and tests/test_gemm_bf16_gpu.py) on the CPU, before they judge a kernel:

(1) their sum over the points is the whole batch's gradient: in float64 torch.autograd.grad of the unchanged ref64 graph with respect to
    the effective matrices, to 1e-12 of sum_p |term_p| per element; in fp32, pushed through the weight-norm backward, the parameter
    gradients of oracle/render_ref.py within the fp32 summation bound P 2^-24 sum_p |term_p| per element (pushed through the same map);
(2) d/dx of the per-point graph is sdf_backward's / colour_backward's bit for bit in float64, fp32 and quant mode, and in quant mode
    the recorded roundings are the same matrices in the same order (so Margin and the kept set are those of the d/dx cases);
(3) a point with all-zero cotangents has exactly zero per-point gradients, and the last layer's db[p] of an SDF network is the
    cotangent itself (g_sdf, g_feat): the fp32 yardstick's error there is exactly 0, which is why the GPU suites compare FB for equality."""
import types

import pytest
import torch

import ref64
from gemm_cases import colour_inputs, cot, cube_points, scaled, scales, sdf_families
from mlp_calls import perturbed
from oracle import render_ref as R

N = 1027
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def model():
    _fx, cfg, params = perturbed()
    return params, cfg


@pytest.fixture(scope="module")
def colour_case(model):
    params, cfg = model
    x, d, normals, feat = colour_inputs(types.SimpleNamespace(params=params, cfg=cfg), N, 7)
    c = scales(N, 8)
    return x, d, normals, feat, scaled(cot(N, 9, (3,)), c), c


def _layers(params, prefix, n):
    return [[params[f"{prefix}.lin{l}.{k}"] for k in ("weight_g", "weight_v", "bias")] for l in range(n)]


def _through_weight_norm(layers, rows, bound):
    """[dW_l | db_l] and a per-element bound on it -> per layer ((dg, dv, db), their bounds): the backward of W = v g / |v| in float64
    and the same map with absolute values applied to the bound"""
    out = []
    for (g, v, _b), r, bd in zip(layers, rows, bound):
        g, v = g.double(), v.double()
        n = v.norm(dim=1, keepdim=True)
        vh = v / n
        dW, B = r[:, :-1], bd[:, :-1]
        dg, Bg = (dW * vh).sum(1, keepdim=True), (B * vh.abs()).sum(1, keepdim=True)
        out.append(((dg, (g / n) * (dW - dg * vh), r[:, -1]), (Bg, (g / n).abs() * (B + Bg * vh.abs()), bd[:, -1])))
    return out


def _hold_sums(what, per_point, batch, oracle_grads, layers, P):
    """(1) for one graph: per_point / batch: namespaces of ref64 in (float64, fp32) / float64; oracle_grads: per layer (dg, dv, db)"""
    p64, p32 = per_point
    for l, (r, b) in enumerate(zip(p64.rows, batch.rows)):
        terms = r.abs().sum(0)
        bad = (r.sum(0) - b).abs() > 1e-12 * terms
        assert not bool(bad.any()), f"{what} layer {l}: the float64 sum over the points differs from the whole batch's gradient at {int(bad.sum())} elements"
    sums = [r.double().sum(0) for r in p32.rows]
    bound = [P * 2.0 ** -24 * r.double().abs().sum(0) for r in p32.rows]
    for l, ((mine, bnd), theirs) in enumerate(zip(_through_weight_norm(layers, sums, bound), oracle_grads)):
        for k, m, b, t in zip(("weight_g", "weight_v", "bias"), mine, bnd, theirs):
            bad = (m.reshape(t.shape) - t.double()).abs() > b.reshape(t.shape)
            assert not bool(bad.any()), f"{what} layer {l} {k}: the fp32 sum differs from the oracle's gradient beyond the summation bound at {int(bad.sum())} elements"


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_sdf_per_point_gradients_sum_to_the_batch_gradient_and_to_the_oracles(model, which):
    params, cfg = model
    prefix, spec = ref64.NETS[which], getattr(cfg, which)
    x = cube_points(N, 5)
    leaves = {k: (v.clone().requires_grad_(True) if k.startswith(prefix + ".lin") else v) for k, v in params.items()}
    layers = _layers(leaves, prefix, spec.n_linear)
    xs = x.clone().requires_grad_(True)
    so, fo, go = R._net_outputs(leaves, prefix, spec, xs)
    for name, (gs, gf, gg, _c) in sdf_families(N).items():
        per_point = [ref64.sdf_weight_grads(params, cfg, x, which, gs, gf, gg, dtype=dt) for dt in (F64, F32)]
        batch = ref64.sdf_weight_grads(params, cfg, x, which, gs, gf, gg, per_point=False)
        assert torch.equal(batch.x, per_point[0].x)
        obj = sum((g_ * y).sum() for g_, y in ((gs, so[:, 0]), (gf, fo), (gg, go)) if g_ is not None)
        leaf = [t for layer in layers for t in layer]
        flat = [torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(torch.autograd.grad(obj, leaf, retain_graph=True, allow_unused=True), leaf)]
        _hold_sums(f"{which}, {name}", per_point, batch, [flat[3 * l:3 * l + 3] for l in range(spec.n_linear)], layers, N)


@pytest.mark.parametrize("grid_grad", [0, 1])
def test_colour_per_point_gradients_sum_to_the_batch_gradient_and_to_the_oracles(model, colour_case, grid_grad):
    params, cfg = model
    x, d, normals, feat, g_rgb, _c = colour_case
    prefix = "rendering_network"
    leaves = {k: (v.clone().requires_grad_(True) if k.startswith(prefix + ".lin") else v) for k, v in params.items()}
    layers = _layers(leaves, prefix, cfg.colour_n_linear)
    rgb = R.colour_net(leaves, cfg, x, normals, d, feat, color_stage="highfreq" if grid_grad else "base")
    flat = torch.autograd.grad((g_rgb * rgb).sum(), [t for layer in layers for t in layer])
    args = (params, cfg, x, normals, d, feat, g_rgb, grid_grad)
    per_point = [ref64.colour_weight_grads(*args, dtype=dt) for dt in (F64, F32)]
    batch = ref64.colour_weight_grads(*args, per_point=False)
    _hold_sums(f"colour grid_grad {grid_grad}", per_point, batch, [flat[3 * l:3 * l + 3] for l in range(cfg.colour_n_linear)], layers, N)


def _modes():
    return (("float64", dict(), None), ("fp32", dict(dtype=F32), None), ("quant float64", dict(), "natural"),
            ("quant fp32, permuted order", dict(dtype=F32), "permuted"))


def _same_trace(what, a, b):
    assert len(a.trace) == len(b.trace) and all(torch.equal(u, v) for u, v in zip(a.trace, b.trace)), f"{what}: the recorded roundings differ"
    assert torch.equal(a.margin, b.margin)


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_sdf_per_point_graph_leaves_ddx_and_the_roundings_unchanged_and_zero_cotangents_give_zero(model, which):
    params, cfg = model
    x = cube_points(N, 5)
    for name, (gs, gf, gg, c) in sdf_families(N).items():
        for mode, kw, order in _modes():
            qa, qb = (ref64.Quant(order=order), ref64.Quant(order=order)) if order else (None, None)
            want = ref64.sdf_backward(params, cfg, x, gs, gf, gg, (which,), quant=qa, **kw)
            r = ref64.sdf_weight_grads(params, cfg, x, which, gs, gf, gg, quant=qb, **kw)
            assert torch.equal(r.x, want), f"{which}, {name}, {mode}: d/dx differs from sdf_backward's"
            if order:
                _same_trace(f"{which}, {name}, {mode}", qa, qb)
            zero = c == 0
            assert int(zero.sum()) >= 5 or "2^20" in name                 # (that family has no zero points)
            for l, rows in enumerate(r.rows):
                assert rows.shape[0] == N and bool((rows[zero] == 0).all()), f"{which}, {name}, {mode}: layer {l} at a zero-cotangent point"
            db = r.rows[-1][:, :, -1]
            cots = torch.cat(((torch.zeros(N) if gs is None else gs).unsqueeze(1), torch.zeros(N, 64) if gf is None else gf), dim=1)
            assert torch.equal(db, cots.to(db.dtype)), f"{which}, {name}, {mode}: the last layer's db[p] is not the cotangent"
            assert len(r.acts) == len(r.rows) and all(a.shape[1] + 1 == w.shape[2] for a, w in zip(r.acts, r.rows))


@pytest.mark.parametrize("grid_grad", [0, 1])
def test_colour_per_point_graph_leaves_the_input_gradients_unchanged_and_zero_cotangents_give_zero(model, colour_case, grid_grad):
    params, cfg = model
    x, d, normals, feat, g_rgb, c = colour_case
    for mode, kw, order in _modes():
        qa, qb = (ref64.Quant(order=order), ref64.Quant(order=order)) if order else (None, None)
        want = ref64.colour_backward(params, cfg, x, normals, d, feat, g_rgb, grid_grad, quant=qa, **kw)
        r = ref64.colour_weight_grads(params, cfg, x, normals, d, feat, g_rgb, grid_grad, quant=qb, **kw)
        for k in want:
            assert torch.equal(r.ins[k], want[k]), f"colour grid_grad {grid_grad}, {mode}: d/d {k} differs from colour_backward's"
        if order:
            _same_trace(f"colour grid_grad {grid_grad}, {mode}", qa, qb)
            assert torch.equal(qa.relu_margin, qb.relu_margin)
        for l, rows in enumerate(r.rows):
            assert bool((rows[c == 0] == 0).all()), f"colour grid_grad {grid_grad}, {mode}: layer {l} at a zero-cotangent point"


def test_the_unrounded_outer_product_is_what_quant_mode_returns_and_the_fault_rounds_it(model):
    """quant mode: db is the gradient at the layer's output and dW = g (x) x of the UNROUNDED vectors (the MAP bodies emit registers
    before the GEMM rounds them), so in a single-layer view dW[p] = db[p] (x) input[p] exactly wherever the double backward adds
    nothing (g_feat alone); "rounded emission rows" (the oracle's _LinQ behaviour) breaks exactly that"""
    params, cfg = model
    x = cube_points(N, 5)
    _gs, gf, _gg, c = sdf_families(N)["g_feat alone x c_p"]
    for fault, same in ((None, True), ("rounded emission rows", False)):
        r = ref64.sdf_weight_grads(params, cfg, x, "fine", None, gf, None, quant=ref64.Quant(fault=fault))
        for l, (rows, act) in enumerate(zip(r.rows, r.acts)):
            outer = rows[:, :, -1].unsqueeze(2) * act.unsqueeze(1)
            assert torch.equal(rows[:, :, :-1], outer) == same, (fault, l)
