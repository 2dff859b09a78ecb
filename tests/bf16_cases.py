"""Inputs and references of the bf16-operand suites (test infrastructure): the kernel families of tests/test_gemm_bf16_gpu.py as
CPU callables, so that tests/test_ref64_bf16_cpu.py fixes the gate's threshold on exactly the cases the GPU suite judges.

A case is a callable ``call(dtype=float64, quant=None) -> {output name: tensor [P, ...]}`` of tests/ref64.py; refs() evaluates it
three times -- B64 (quant, float64 accumulation; its Quant gives the rounding margin), the yardstick (quant, fp32 accumulation) and
plain float64 (for the size of the bf16 effect)."""
import types

import torch

import bf16_gate as G
import ref64
from gemm_cases import KINK, colour_inputs, cot, cube_points, scaled, scales
from gemm_cases import sdf_families as fp32_families

N = 4123                                        # 128 x 32 + 27: ragged for both tilings
UNIT = "all three x c_p in [1/8, 8]"            # the accumulate = 1 family: every point's c_p = 2^U{-3..3}


def refs(call, weights=None):
    """-> b64, y32 (natural order), perm (permuted order), f64, margin (both fp32 evaluations are its noise samples), relu_margin"""
    q64, q32, qp = ref64.Quant(weights), ref64.Quant(weights), ref64.Quant(weights, "permuted")
    b64, y32, perm = call(quant=q64), call(dtype=torch.float32, quant=q32), call(dtype=torch.float32, quant=qp)
    return types.SimpleNamespace(b64=b64, y32=y32, perm=perm, f64=call(), margin=ref64.Margin(q64, (q32, qp), G.LADDER),
                                 relu_margin=q64.relu_margin)


def emulate(call, weights=None, order="natural", fault=None):
    """the case in fp32 accumulation: a correct emulation (either order) or a deliberately wrong one (ref64.FAULTS)"""
    return call(dtype=torch.float32, quant=ref64.Quant(weights, order, fault))


def sdf_families(n=N):
    """tests/gemm_cases.py's cotangent families + UNIT -> name -> (g_sdf, g_feat, g_grad, c_p)"""
    fam = fp32_families(n)
    g = torch.Generator().manual_seed(31)
    c = torch.exp2(torch.randint(-3, 4, (n,), generator=g).double())
    fam[UNIT] = tuple(scaled(b, c) for b in (cot(n, 10, ()), cot(n, 11, (64,)), cot(n, 12, (3,)))) + (c,)
    return fam


def sdf_forward_case(params, cfg, x, nets):
    return lambda **kw: dict(zip(("sdf", "grad", "feat"), ref64.sdf_forward(params, cfg, x, nets, **kw)))


def sdf_backward_case(params, cfg, x, nets, gs, gf, gg):
    return lambda **kw: dict(x=ref64.sdf_backward(params, cfg, x, gs, gf, gg, nets, **kw))


def colour_forward_case(params, cfg, x, d, normals, feat):
    return lambda **kw: dict(rgb=ref64.colour_forward(params, cfg, x, normals, d, feat, **kw))


def colour_backward_case(params, cfg, x, d, normals, feat, g_rgb, grid_grad):
    return lambda **kw: ref64.colour_backward(params, cfg, x, normals, d, feat, g_rgb, grid_grad, **kw)


def colour_coarse_case(params, cfg, x, d, normals, feat, g_rgb, grid_grad, g_sdf):
    """d/dx of the colour backward + the coarse SDF backward for (g_sdf, the colour's feature and normal cotangents in the chain's own
    dtype); one Quant serves both graphs, so the margin covers both"""
    def call(**kw):
        c = ref64.colour_backward(params, cfg, x, normals, d, feat, g_rgb, grid_grad, **kw)
        return dict(x=c["x"] + ref64.sdf_backward(params, cfg, x, g_sdf, c["feat"], c["normals"], ("coarse",), **kw))
    return call


def layer(l):
    return f"[dW{l} | db{l}]"


def sdf_weight_grad_case(params, cfg, x, which, gs, gf, gg):
    """the per-point weight gradients of sdf_backward_case's graph (the same roundings in the same order: the same Margin and kept set)
    -> per layer "[dW_l | db_l]" [P, out, in + 1], and the Softplus outputs "H_k" [P, 64] (value path: a FORWARD quantity)"""
    def call(**kw):
        r = ref64.sdf_weight_grads(params, cfg, x, which, gs, gf, gg, **kw)
        out = {layer(l): rows for l, rows in enumerate(r.rows)}
        out.update({f"H{k}": r.acts[k] for k in range(1, len(r.acts))})
        return out
    return call


def colour_weight_grad_case(params, cfg, x, d, normals, feat, g_rgb, grid_grad):
    def call(**kw):
        r = ref64.colour_weight_grads(params, cfg, x, normals, d, feat, g_rgb, grid_grad, **kw)
        out = {layer(l): rows for l, rows in enumerate(r.rows)}
        out.update({f"H{k}": r.acts[k] for k in range(1, len(r.acts))})
        return out
    return call


def weight_grad_cases(params, cfg, n=N, i=None):
    """name -> (call, c_p, backward = True, colour?): the emission-row gates of tests/test_gemm_bf16_gpu.py, on the points and
    cotangents of the d/dx cases.  Not part of all_cases: a case's references are some GB at n = 4 123 (fine network), so they are
    built one case at a time and dropped."""
    out, i = {}, inputs(params, cfg, n) if i is None else i
    for which in ("coarse", "fine"):
        for name, (gs, gf, gg, c) in i.fam.items():
            out[f"weight gradients {which}: {name}"] = (sdf_weight_grad_case(params, cfg, i.xb, which, gs, gf, gg), c, True, False)
    for gg_ in (0, 1):
        out[f"weight gradients colour grid_grad {gg_}"] = (colour_weight_grad_case(params, cfg, i.x, i.d, i.normals, i.feat, i.g_rgb, gg_),
                                                            i.c, True, True)
    return out


def inputs(params, cfg, n=N):
    """every input of the suite (the fp32 suite's builders and seeds at n points): xf / xb the points of the SDF forwards / backwards,
    fam the cotangent families, x, d, normals, feat, c, g_rgb, g_sdf the colour kernels' inputs and cotangents"""
    x, d, normals, feat = colour_inputs(types.SimpleNamespace(params=params, cfg=cfg), n, 7)
    c = scales(n, 8)
    return types.SimpleNamespace(xf=cube_points(n, 1), xb=cube_points(n, 5), fam=sdf_families(n), x=x, d=d, normals=normals, feat=feat, c=c,
                                 g_rgb=scaled(cot(n, 9, (3,)), c), g_sdf=scaled(cot(n, 15, ()), c))


def all_cases(params, cfg, n=N):
    """name -> (call, norm [P] or None (forward: the B64 output's norm, floor 1), backward?, colour?): every family with a reference"""
    out, i = {}, inputs(params, cfg, n)
    for name, nets in (("coarse", ("coarse",)), ("fine", ("fine",)), ("pair", ("coarse", "fine"))):
        out[f"sdf forward {name}"] = (sdf_forward_case(params, cfg, i.xf, nets), None, False, False)
    for which in ("coarse", "fine"):
        for name, (gs, gf, gg, c) in i.fam.items():
            out[f"sdf backward {which}: {name}"] = (sdf_backward_case(params, cfg, i.xb, (which,), gs, gf, gg), c, True, False)
    col = (params, cfg, i.x, i.d, i.normals, i.feat)
    out["colour forward"] = (colour_forward_case(*col), None, False, True)
    for gg_ in (0, 1):
        out[f"colour backward grid_grad {gg_}"] = (colour_backward_case(*col, i.g_rgb, gg_), i.c, True, True)
        out[f"colour + coarse backward grid_grad {gg_}"] = (colour_coarse_case(*col, i.g_rgb, gg_, i.g_sdf), i.c, True, True)
    return out


def kink_keep(r):
    keep = r.relu_margin >= KINK
    assert int((~keep).sum()) <= keep.numel() // 100, int((~keep).sum())
    return keep
