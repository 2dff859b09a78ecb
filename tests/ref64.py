"""A float64 restatement of the reference's SDF and colour networks with the reference's derivative structure (test infrastructure).

The hash grids are not re-implemented in float64: at each point x0 the C oracle (oracle/hashenc.py) gives the fp32 features f0 and
their Jacobian (hash_encode_forward with calc_grad_inputs), and the grid is replaced by its linearisation
    f(x) = f0 + J (x - x0),   J constant,
promoted to float64.  At x0 this has the reference's value and first derivative; its second derivative through the grid is zero,
which is exactly the term the reference drops (hashgrid.py:134, restated in oracle/render_ref.py::_EncodeBwd).  Everything else --
positional encoding, weight norm, Softplus(beta = 100), ReLU, sigmoid, the COMBINE and color_stage = "base" -- is plain torch in the
requested dtype with autograd (create_graph for the double backward through grad sdf).

``grid="exact"`` puts tests/grid_ref64.py's encoder (the grid itself in the requested dtype, with the same dropped term and the discrete
part taken from the fp32 inputs) in the place of the linearisation and makes the tables differentiable inputs: sdf_table_grad and
colour_table_grad give the table gradients the mapping kernels accumulate -- the value path plus, for the SDF grids, the table's
share of the double backward through grad sdf.  The default stays the linearisation.

Inputs are the explicit fp32 tensors the kernels see; ``dtype=torch.float32`` evaluates the same graph in fp32 (tests/test_ref64_cpu.py
holds that to oracle/render_ref.py).

``quant=Quant(...)`` is the bf16-operand mode (what csrc/*_bf16.hip computes, NSA_PIECES == 1; the same dataflow as
oracle/render_ref.py::_LinQ, in any dtype): both operands of every matrix-core GEMM are rounded to bfloat16, round to nearest even,
products are exact, accumulation is in the working dtype; every derivative GEMM rounds the vector it multiplies, recursively (the
second-order sweeps through grad sdf included); the rounding has derivative 1.  Unrounded stay the sdf row of an SDF network's last
layer, the colour network's 64 -> 3 layer and everything the kernels do on the vector ALU.  The weights are the effective FP32
matrices (``Quant.weights``: what fused/pack.py::flat_params gives on the device, copied to the host; default: the oracle's fp32
weight norm), rounded once -- never a float64 weight norm: one weight that rounds the other way moves every point.
While it rounds, a Quant records every operand matrix (activations, cotangents, tangents: the forward graph and every backward
through it), from which ``Margin`` forms the per-point ROUNDING MARGIN: how far every rounded operand of the point lies from the
nearest rounding boundary (the midpoint of two neighbouring bf16 values), in units of the measured fp32 noise of the vector the
operand belongs to (class Margin states the unit).  On a point that is kept, two correct implementations take the same rounding
decisions and agree to working-precision noise; the others may flip (tests/bf16_gate.py).  ``Quant.margin`` is the same distance
in units of the operand's own bf16 spacing (no knowledge of the noise), kept for the report.

``sdf_weight_grads`` / ``colour_weight_grads`` evaluate the same graphs (bit for bit: the same calls in the same order, so d/dx and the
rounding trace are today's) and return, PER POINT, the gradient of the kernels' objective with respect to every layer's effective
matrix and bias -- what the MAP kernels' emission rows encode before nsa_emit_gemm sums them over the points (tests/emit_rows.py) --
and the layer inputs.  Every layer takes a zero-stride per-point leaf [P, out, in] next to its shared matrix (class _LinP / _LinQP:
the forward ignores the leaf, the backward returns g (x) x to it and applies itself to g and the transposed leaf, so the share of the
double backward through grad sdf arrives too); the bias gradient is the gradient at the layer's output.  In quant mode the outer
product is formed from the UNROUNDED vectors: the MAP bodies emit their registers before the GEMM rounds them."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import grid_ref64
from oracle.hashenc import OracleBackend

F64 = torch.float64


class ExactGrids:
    """grid="exact": per grid the table as a differentiable leaf in the working dtype and the discrete plan of the batch"""

    def __init__(self):
        self.tables, self.plans = {}, {}

    def features(self, key, x, x0, emb, spec, divide_factor, dtype):
        u32 = ((x0 / divide_factor + 1) / 2).contiguous()          # the fp32 unit coordinate decides range and cell
        self.plans[key] = plan = grid_ref64.Plan(u32, spec)
        plan.record = []
        self.tables[key] = table = emb.detach().to(dtype).requires_grad_(True)
        return grid_ref64.grid_features((x / divide_factor + 1) / 2, table, spec, plan=plan)


def _grid(exact, key, x, x0, emb, spec, divide_factor, dtype):
    if exact is None:
        return _linear_grid(x, x0, emb, spec, divide_factor, dtype)
    return exact.features(key, x, x0, emb, spec, divide_factor, dtype)


def _linear_grid(x, x0, emb, spec, divide_factor, dtype):
    """Linearised grid at the fp32 points x0 (the reference's map (x / df + 1) / 2 in fp32), evaluated at x (dtype, same values)."""
    u = ((x0 / divide_factor + 1) / 2).contiguous()
    B, D = u.shape
    L, C = spec.num_levels, spec.level_dim
    out = torch.empty(L, B, C)
    dy_du = torch.empty(B, L * D * C)
    OracleBackend.hash_encode_forward(u, emb.contiguous(), spec.offsets, out, B, D, C, L, float(np.log2(spec.per_level_scale)),
                                      spec.base_resolution, True, dy_du)
    f0 = out.permute(1, 0, 2).reshape(B, L * C)
    # dy_du[b, l, d, c] -> J[b, l*C + c, d]; du/dx = 1 / (2 df)
    J = dy_du.view(B, L, D, C).permute(0, 1, 3, 2).reshape(B, L * C, D).to(dtype) * (0.5 / divide_factor)
    return f0.to(dtype) + ((x - x0.to(dtype)).unsqueeze(1) * J).sum(-1)


def _pe(x, n_freq):
    parts = [x]
    for k in range(n_freq):
        parts += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(parts, -1)


def rne_bf16(x):
    """x (any float dtype) -> the nearest bfloat16 value, ties to even, in x's dtype, in ONE rounding (a float64 value must not pass
    through fp32 on its way), and the distance of x to the nearest rounding boundary in units of x's bf16 spacing."""
    m, e = torch.frexp(x)                                  # |m| in [0.5, 1): m * 256 has 8 bits in front of the binary point
    t = m * 256
    r = torch.round(t)                                     # half to even
    return torch.ldexp(r, e - 8), 0.5 - (t - r).abs()


FAULTS = ("truncated weights", "unrounded cotangents", "neighbour's operand group", "rounded sdf row")
WEIGHT_GRAD_FAULTS = ("rounded emission rows",)     # only the per-point weight gradients see it (g (x) x of the rounded vectors)


class Quant:
    """The bf16-operand mode of this module (module docstring) and the per-point rounding margin of the last call.
    weights: {"<network>.lin<l>": (W fp32 [out, in], b fp32 [out])} -- the effective matrices the pack takes (weights_of_model);
    None: the oracle's fp32 weight norm of ``params`` on the host.
    order: "natural" | "permuted" | ("permuted", seed) -- the k order of every GEMM's sum (correct emulations in fp32).
    fault: None, or one of FAULTS: a deliberately WRONG emulation (tests/test_ref64_bf16_cpu.py: the gate must refuse each)."""

    def __init__(self, weights=None, order="natural", fault=None):
        assert (order in ("natural", "permuted") or order[0] == "permuted") and (fault is None or fault in FAULTS + WEIGHT_GRAD_FAULTS), (order, fault)
        self.weights, self.order, self.fault = weights, order, fault
        self._w, self._perm = {}, {}
        self.trace = []                     # every operand matrix [P, K] as it reached a rounding, in order (Margin)
        self.margin = None                  # [P] smallest distance to a boundary in units of the operand's OWN bf16 spacing
        self.relu_margin = None             # [P] colour network: min |pre-activation| of its ReLU units

    def reset(self, P):
        """called where a graph is built; a Quant that serves several graphs of the same points keeps accumulating"""
        if self.margin is None:
            self.margin = torch.full((P,), 0.5, dtype=F64)
            self.relu_margin = torch.full((P,), float("inf"), dtype=F64)
        assert self.margin.shape[0] == P

    def weight(self, params, prefix, dtype):
        key = (prefix, dtype)
        if key not in self._w:
            if self.weights is not None:
                w, b = self.weights[prefix]
            else:
                g, v, b = (params[f"{prefix}.{k}"].float() for k in ("weight_g", "weight_v", "bias"))
                w = v * (g / v.norm(2, dim=1, keepdim=True))
            assert w.dtype == torch.float32 and b.dtype == torch.float32
            w = w.detach().cpu().to(dtype)
            if self.fault == "truncated weights":
                m, e = torch.frexp(w)
                wr = torch.ldexp(torch.trunc(m * 256), e - 8)
            else:
                wr = rne_bf16(w)[0]
            self._w[key] = (w, wr, b.detach().cpu().to(dtype))
        return self._w[key]

    def round(self, x, cotangent):
        if cotangent and self.fault == "unrounded cotangents":
            return x
        r, margin = rne_bf16(x)
        self.margin = torch.minimum(self.margin, margin.reshape(margin.shape[0], -1).amin(1).double())
        self.trace.append(x.detach())
        if not cotangent and self.fault == "neighbour's operand group" and x.shape[1] == 64:
            p = torch.arange(0, x.shape[0] - 1, 16)
            r = r.clone()
            r[p, 8:16] = r[p + 1, 8:16]
        return r

    def matmul(self, xr, wr):
        if self.order != "natural":
            K = wr.shape[1]
            if K not in self._perm:
                seed = 0 if self.order == "permuted" else int(self.order[1])
                self._perm[K] = torch.randperm(K, generator=torch.Generator().manual_seed(K + 1000 * seed))
            return xr[:, self._perm[K]] @ wr[:, self._perm[K]].t()
        return xr @ wr.t()


class Margin:
    """The per-point ROUNDING MARGIN of one reference call, from the Quant of its float64-accumulating evaluation (q64) and the Quants
    of fp32-accumulating evaluations of it (q32s: natural and permuted summation order) -- the same graph, so the same operand
    matrices in the same order.

    UNIT: the operand's own fp32 noise, measured: nu = the largest |fp32 - float64| difference of that operand before rounding over
    the fp32 evaluations (floor: half an fp32 spacing of the operand).  An operand's bf16 spacing does not know that noise: an entry
    that is small beside the sums it came out of (a Softplus output near ln 2 / 100, a cancelled sum, beta = 100 times the noise of a
    pre-activation) carries many of its own fp32 spacings of noise and flips at margins of 1e-3 of its bf16 spacing, while an entry
    with noise of its own size is safe at 1e-5 of it.  In this unit one threshold fits both.
    A point is KEPT at threshold t when every rounded operand x of it either lies at least t nu from the nearest rounding boundary, or
    is so noisy that a flip moves it by no more than 2 t nu (bf16 spacing of x <= 2 t nu: such an operand can never be t nu from a
    boundary, and its flip is of the size of the noise that the threshold tolerates anyway).  A point where an fp32 evaluation itself
    flipped has a large nu downstream and drops out.  kept(t) is computed for the thresholds given at construction."""

    def __init__(self, q64, q32s, thresholds):
        assert q32s and all(len(q64.trace) == len(q.trace) for q in q32s) and len(q64.trace) > 0
        self.own, self.relu_margin, self.n_operands = q64.margin, q64.relu_margin, len(q64.trace)
        self._kept = {t: torch.ones(q64.margin.shape[0], dtype=torch.bool) for t in thresholds}
        for i, x64 in enumerate(q64.trace):
            assert x64.dtype == F64
            nu = 2.0 ** -24 * x64.abs()
            for q in q32s:
                nu = torch.maximum(nu, (q.trace[i].double() - x64).abs())
            m, e = torch.frexp(x64)
            t = m * 256
            spacing = torch.ldexp(torch.ones_like(x64), e - 8)
            dist = (0.5 - (t - torch.round(t)).abs()) * spacing
            for thr, kept in self._kept.items():
                kept &= ((dist >= thr * nu) | (spacing <= 2 * thr * nu)).all(1)

    def kept(self, threshold):
        return self._kept[threshold]


class _RoundQ(torch.autograd.Function):
    """x -> bf16(x), derivative 1 (the rounding of a GEMM operand is not part of the differentiated graph)"""

    @staticmethod
    def forward(ctx, x, q, cotangent):
        return q.round(x, cotangent)

    @staticmethod
    def backward(ctx, g):
        return g, None, None


class _LinQ(torch.autograd.Function):
    """y = xr wr^T on rounded operands; every derivative GEMM rounds the vector it multiplies, recursively"""

    @staticmethod
    def forward(ctx, xr, wr, q):
        ctx.wr, ctx.q = wr, q
        return q.matmul(xr, wr)

    @staticmethod
    def backward(ctx, g):
        return _LinQ.apply(_RoundQ.apply(g, ctx.q, True), ctx.wr.t().contiguous(), ctx.q), None, None


class Taps:
    """What a graph records for the weight gradients.  per_point: every layer gets a zero-stride leaf [P, out, in] (class _LinP);
    otherwise (whole batch, quant is None) the effective matrix and bias themselves become leaves of the unchanged graph."""

    def __init__(self, per_point=True):
        self.per_point, self.layers = per_point, []            # layers: (prefix, leaves, layer input, layer output)

    def leaf(self, P, w):
        return torch.zeros((), dtype=w.dtype).expand(P, *w.shape).requires_grad_(True)


class _LinP(torch.autograd.Function):
    """y = F.linear(x, w, b) exactly; zw [P, out, in] receives the per-point g (x) x, of this product and of every derivative of it"""

    @staticmethod
    def forward(ctx, x, w, b, zw):
        ctx.save_for_backward(x, w, zw)
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w, zw = ctx.saved_tensors
        gx = _LinP.apply(g, w.t(), None, zw.transpose(1, 2)) if ctx.needs_input_grad[0] else None       # (as autograd: no unneeded GEMM)
        return gx, None, None, g.unsqueeze(2) * x.unsqueeze(1)


class _LinQP(torch.autograd.Function):
    """_LinQ(_RoundQ(x)) in one node (the same roundings in the same order); zw receives g (x) x of the UNROUNDED vectors"""

    @staticmethod
    def forward(ctx, x, wr, q, cotangent, zw):
        ctx.save_for_backward(x, zw)
        ctx.wr, ctx.q = wr, q
        return q.matmul(q.round(x, cotangent), wr)

    @staticmethod
    def backward(ctx, g):
        x, zw = ctx.saved_tensors
        # (no GEMM, hence no recorded rounding, where _LinQ's node would not exist: the trace stays sdf_backward's)
        gx = _LinQP.apply(g, ctx.wr.t().contiguous(), ctx.q, True, zw.transpose(1, 2)) if ctx.needs_input_grad[0] else None
        if ctx.q.fault == "rounded emission rows":
            return gx, None, None, None, rne_bf16(g)[0].unsqueeze(2) * rne_bf16(x)[0].unsqueeze(1)
        return gx, None, None, None, g.unsqueeze(2) * x.unsqueeze(1)


def _lin(params, prefix, h, dtype, quant=None, exact_rows=0, taps=None):
    """quant: rows [exact_rows:] are matrix-core rows (bf16 operands), rows [:exact_rows] vector-ALU rows (unrounded)"""
    if quant is None:
        g, v, b = (params[f"{prefix}.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
        w = v * (g / v.norm(2, dim=1, keepdim=True))
        if taps is None:
            return F.linear(h, w, b)
        if not taps.per_point:
            w, b = w.detach().requires_grad_(True), b.detach().requires_grad_(True)
            y = F.linear(h, w, b)
            taps.layers.append((prefix, (w, b), h, y))
            return y
        zw = taps.leaf(h.shape[0], w)
        y = _LinP.apply(h, w, b, zw)
        taps.layers.append((prefix, zw, h, y))
        return y
    w, wr, b = quant.weight(params, prefix, dtype)
    if quant.fault == "rounded sdf row" and exact_rows < w.shape[0]:
        exact_rows = 0
    assert taps is None or taps.per_point
    zw = taps.leaf(h.shape[0], w) if taps is not None else None
    parts = []
    if exact_rows:
        if zw is None:
            parts.append(F.linear(h, w[:exact_rows], b[:exact_rows]))
        else:
            parts.append(_LinP.apply(h, w[:exact_rows], b[:exact_rows], zw[:, :exact_rows]))
    if exact_rows < w.shape[0]:
        if zw is None:
            parts.append(_LinQ.apply(_RoundQ.apply(h, quant, False), wr[exact_rows:], quant) + b[exact_rows:])
        else:
            parts.append(_LinQP.apply(h, wr[exact_rows:], quant, False, zw[:, exact_rows:]) + b[exact_rows:])
    y = torch.cat(parts, dim=-1)
    if taps is not None:
        taps.layers.append((prefix, zw, h, y))
    return y


def weights_of_model(model):
    """Quant.weights of a SLAMNetwork on the GPU: the effective fp32 matrices exactly as the packs take them
    (fused/pack.py::flat_params, computed on the device), split per layer and copied to the host."""
    from nicer_slam_amd.fused import pack
    out = {}
    nets = {"implicit_network.coarse": model.implicit_network.coarse, "implicit_network.fine": model.implicit_network.fine,
            "rendering_network": model.rendering_network}
    for prefix, net in nets.items():
        with torch.no_grad():
            flat = pack.flat_params(net).detach().cpu()
        o = 0
        for l in range(net.num_layers - 1):
            rows, cols = getattr(net, f"lin{l}").weight_v.shape
            out[f"{prefix}.lin{l}"] = (flat[o:o + rows * cols].view(rows, cols).clone(), flat[o + rows * cols:o + rows * cols + rows].clone())
            o += rows * cols + rows
        assert o + 1 == flat.numel(), (prefix, o, flat.numel())
    return out


def _sdf_net(params, prefix, spec, x, x0, dtype, exact=None, quant=None, taps=None):
    feat = _grid(exact, prefix, x, x0, params[prefix + ".encoding.embeddings"], spec.grid, spec.divide_factor, dtype)
    h = torch.cat((_pe(x, spec.multires), feat), dim=-1)
    for l in range(spec.n_linear):
        h = _lin(params, f"{prefix}.lin{l}", h, dtype, quant, exact_rows=1 if l == spec.n_linear - 1 else 0, taps=taps)
        if l < spec.n_linear - 1:
            h = F.softplus(h, beta=100)
    return h


NETS = {"coarse": "implicit_network.coarse", "fine": "implicit_network.fine"}


def _sdf_graph(params, cfg, x0, nets, dtype, exact=None, quant=None, taps=None):
    assert quant is None or exact is None, "quant: linearised grids only"
    if quant is not None:
        quant.reset(x0.shape[0])
    x = x0.detach().to(dtype).requires_grad_(True)
    sdf, feat, grad = 0, 0, 0
    for which in nets:
        out = _sdf_net(params, NETS[which], getattr(cfg, which), x, x0, dtype, exact, quant, taps)
        s = out[:, 0]
        (g,) = torch.autograd.grad(s, x, torch.ones_like(s), create_graph=True)
        sdf, feat, grad = sdf + s, feat + out[:, 1:], grad + g
    return x, sdf, feat, grad


def _exact(grid):
    assert grid in ("linear", "exact"), grid
    return ExactGrids() if grid == "exact" else None


def sdf_forward(params, cfg, x0, nets=("coarse", "fine"), dtype=F64, grid="linear", quant=None):
    """-> sdf [P], grad sdf [P,3], feature [P,64] of the networks in ``nets`` (summed: the COMBINE for both)."""
    _x, sdf, feat, grad = _sdf_graph(params, cfg, x0, nets, dtype, _exact(grid), quant)
    return sdf.detach(), grad.detach(), feat.detach()


def _sdf_objective(sdf, feat, grad, g_sdf, g_feat, g_grad, dtype):
    obj = 0
    for g, y in ((g_sdf, sdf), (g_feat, feat), (g_grad, grad)):
        if g is not None:
            obj = obj + (g.to(dtype) * y).sum()
    return obj


def sdf_backward(params, cfg, x0, g_sdf=None, g_feat=None, g_grad=None, nets=("coarse", "fine"), dtype=F64, grid="linear", quant=None):
    """d/dx of  g_sdf . sdf + g_feat . feature + g_grad . grad sdf  (any cotangent may be None = absent) -> [P,3]."""
    x, sdf, feat, grad = _sdf_graph(params, cfg, x0, nets, dtype, _exact(grid), quant)
    obj = _sdf_objective(sdf, feat, grad, g_sdf, g_feat, g_grad, dtype)
    if not torch.is_tensor(obj):
        return torch.zeros_like(x).detach()
    (gx,) = torch.autograd.grad(obj, x)
    return gx


def _weight_grads(obj, ins, taps):
    """-> (d/d ins, the weight gradients of ``taps``: per layer [P, out, in + 1] = [dW_l | db_l] per point, resp. (whole batch)
    [out, in + 1]; the layer inputs [P, in])"""
    acts = [h.detach() for _p, _l, h, _y in taps.layers]
    if not torch.is_tensor(obj):
        shape = lambda l, h, y: ((h.shape[0],) if taps.per_point else ()) + (y.shape[1], h.shape[1] + 1)
        return [torch.zeros_like(t).detach() for t in ins], [torch.zeros(shape(l, h, y), dtype=h.dtype) for _p, l, h, y in taps.layers], acts
    n = len(taps.layers)
    if taps.per_point:
        gs = torch.autograd.grad(obj, list(ins) + [l for _p, l, _h, _y in taps.layers] + [y for _p, _l, _h, y in taps.layers], allow_unused=True)
        gi, gw, gb = gs[:len(ins)], gs[len(ins):len(ins) + n], gs[len(ins) + n:]
    else:
        gs = torch.autograd.grad(obj, list(ins) + [l[0] for _p, l, _h, _y in taps.layers] + [l[1] for _p, l, _h, _y in taps.layers], allow_unused=True)
        gi, gw, gb = gs[:len(ins)], gs[len(ins):len(ins) + n], gs[len(ins) + n:]
    rows = []
    for (_p, _l, h, y), w, b in zip(taps.layers, gw, gb):
        lead = (h.shape[0],) if taps.per_point else ()
        w = torch.zeros(lead + (y.shape[1], h.shape[1]), dtype=h.dtype) if w is None else w
        b = torch.zeros(lead + (y.shape[1],), dtype=h.dtype) if b is None else b
        rows.append(torch.cat((w, b.unsqueeze(-1)), dim=-1))
    return [torch.zeros_like(t).detach() if g is None else g for g, t in zip(gi, ins)], rows, acts


def sdf_weight_grads(params, cfg, x0, which, g_sdf=None, g_feat=None, g_grad=None, dtype=F64, quant=None, per_point=True):
    """The network ``which`` under the objective of sdf_backward -> namespace(x = d/dx [P,3] (sdf_backward's, bit for bit),
    rows = per layer [P, out, in + 1]: the point's [dW_l | db_l] with respect to the EFFECTIVE matrix and bias (features in the
    reference's order), acts = per layer its input [P, in] (acts[0]: the first-layer input, acts[k]: h_k)).
    per_point = False (quant is None): rows = the whole batch's [out, in + 1], from the unchanged graph with the matrices as leaves."""
    taps = Taps(per_point)
    x, sdf, feat, grad = _sdf_graph(params, cfg, x0, (which,), dtype, None, quant, taps)
    (gx,), rows, acts = _weight_grads(_sdf_objective(sdf, feat, grad, g_sdf, g_feat, g_grad, dtype), (x,), taps)
    return types.SimpleNamespace(x=gx, rows=rows, acts=acts)


def colour_weight_grads(params, cfg, x0, normals, dirs, feats, g_rgb, grid_grad=1, dtype=F64, quant=None, per_point=True):
    """The colour network under g_rgb . rgb -> namespace(ins = colour_backward's dict, bit for bit; rows, acts as sdf_weight_grads)"""
    taps = Taps(per_point)
    ins, rgb = _colour_graph(params, cfg, x0, normals, dirs, feats, grid_grad, dtype, quant=quant, taps=taps)
    gs, rows, acts = _weight_grads((g_rgb.to(dtype) * rgb).sum(), ins, taps)
    return types.SimpleNamespace(ins=dict(zip(("x", "normals", "dirs", "feat"), gs)), rows=rows, acts=acts)


def sdf_first_layer_input(params, cfg, x0, which, dtype=F64):
    """[PE(x) | grid features] of the network ``which`` [P, 39 + L C] with the GRID ITSELF in ``dtype`` (grid = "exact").  acts[0] of
    sdf_weight_grads carries the linearisation's f0, the C oracle's fp32 features promoted: right for everything downstream, but as
    a reference OF the features it would give an fp32 evaluation an error of exactly 0 there."""
    spec, x = getattr(cfg, which), x0.detach().to(dtype)
    with torch.no_grad():
        feat = ExactGrids().features(NETS[which], x, x0, params[NETS[which] + ".encoding.embeddings"], spec.grid, spec.divide_factor, dtype)
        return torch.cat((_pe(x, spec.multires), feat), dim=-1)


def colour_first_layer_input(params, cfg, x0, normals, dirs, feats, dtype=F64):
    """[x | PE(d) | n | feature | colour grid features] [P, 129] with the grid itself in ``dtype`` (see sdf_first_layer_input)"""
    x, n, d, f = (t.detach().to(dtype) for t in (x0, normals, dirs, feats))
    with torch.no_grad():
        gf = ExactGrids().features("colour", x, x0, params["rendering_network.encoding.embeddings"], cfg.colour_grid, cfg.colour_divide_factor, dtype)
        return torch.cat([x, _pe(d, cfg.multires_view), n, f, gf], dim=-1)


def sdf_table_grad(params, cfg, x0, which, g_sdf=None, g_feat=None, g_grad=None, dtype=F64):
    """grid="exact": -> (d/dx [P,3], d/d table [rows, C] of the network ``which``, plan).  The table gradient is the value path plus
    the table's share of the double backward through grad sdf.  plan.record lists what reached the grid, in order: ("first", g) for
    every first backward (the last one is the value path: g = d objective / d features), ("second", g, q) for the double backward
    (g = d sdf / d features, q = the cotangent of J^T g in unit coordinates): enough to form every row's contributions."""
    exact = ExactGrids()
    x, sdf, feat, grad = _sdf_graph(params, cfg, x0, (which,), dtype, exact)
    obj = _sdf_objective(sdf, feat, grad, g_sdf, g_feat, g_grad, dtype)
    table, plan = exact.tables[NETS[which]], exact.plans[NETS[which]]
    if not torch.is_tensor(obj):
        return torch.zeros_like(x).detach(), torch.zeros_like(table).detach(), plan
    gx, gt = torch.autograd.grad(obj, (x, table))
    return gx, gt, plan


def _colour_graph(params, cfg, x0, normals, dirs, feats, grid_grad, dtype, exact=None, quant=None, taps=None):
    assert quant is None or exact is None, "quant: linearised grids only"
    if quant is not None:
        quant.reset(x0.shape[0])
    x, n, d, f = (t.detach().to(dtype).requires_grad_(True) for t in (x0, normals, dirs, feats))
    gf = _grid(exact, "colour", x, x0, params["rendering_network.encoding.embeddings"], cfg.colour_grid, cfg.colour_divide_factor, dtype)
    if not grid_grad:                     # color_stage == "base": the colour grid feature is detached (base_networks.py:337-339)
        gf = gf.detach()
    h = torch.cat([x, _pe(d, cfg.multires_view), n, f, gf], dim=-1)
    for l in range(cfg.colour_n_linear):
        h = _lin(params, f"rendering_network.lin{l}", h, dtype, quant, exact_rows=3 if l == cfg.colour_n_linear - 1 else 0, taps=taps)
        if l < cfg.colour_n_linear - 1:
            if quant is not None:         # the ReLU kinks of THIS graph (its pre-activations differ from the unrounded ones by a bf16 effect)
                quant.relu_margin = torch.minimum(quant.relu_margin, h.detach().abs().amin(1).double())
            h = torch.relu(h)
    return (x, n, d, f), torch.sigmoid(h)


def colour_forward(params, cfg, x0, normals, dirs, feats, dtype=F64, quant=None):
    """-> rgb [P,3]."""
    with torch.no_grad():
        return _colour_graph(params, cfg, x0, normals, dirs, feats, False, dtype, quant=quant)[1]


def colour_backward(params, cfg, x0, normals, dirs, feats, g_rgb, grid_grad=1, dtype=F64, quant=None):
    """-> dict(x, normals, dirs, feat) of d(g_rgb . rgb); grid_grad = 0 is color_stage "base"."""
    ins, rgb = _colour_graph(params, cfg, x0, normals, dirs, feats, grid_grad, dtype, quant=quant)
    gs = torch.autograd.grad((g_rgb.to(dtype) * rgb).sum(), ins)
    return dict(zip(("x", "normals", "dirs", "feat"), gs))


def colour_table_grad(params, cfg, x0, normals, dirs, feats, g_rgb, dtype=F64):
    """grid="exact", grid_grad = 1: -> (dict(x, normals, dirs, feat), d/d colour table [rows, 2], plan) of d(g_rgb . rgb)."""
    exact = ExactGrids()
    ins, rgb = _colour_graph(params, cfg, x0, normals, dirs, feats, 1, dtype, exact)
    gs = torch.autograd.grad((g_rgb.to(dtype) * rgb).sum(), ins + (exact.tables["colour"],))
    return dict(zip(("x", "normals", "dirs", "feat"), gs[:4])), gs[4], exact.plans["colour"]
