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
holds that to oracle/render_ref.py)."""
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


def _lin(params, prefix, h, dtype):
    g, v, b = (params[f"{prefix}.{k}"].to(dtype) for k in ("weight_g", "weight_v", "bias"))
    return F.linear(h, v * (g / v.norm(2, dim=1, keepdim=True)), b)


def _sdf_net(params, prefix, spec, x, x0, dtype, exact=None):
    feat = _grid(exact, prefix, x, x0, params[prefix + ".encoding.embeddings"], spec.grid, spec.divide_factor, dtype)
    h = torch.cat((_pe(x, spec.multires), feat), dim=-1)
    for l in range(spec.n_linear):
        h = _lin(params, f"{prefix}.lin{l}", h, dtype)
        if l < spec.n_linear - 1:
            h = F.softplus(h, beta=100)
    return h


NETS = {"coarse": "implicit_network.coarse", "fine": "implicit_network.fine"}


def _sdf_graph(params, cfg, x0, nets, dtype, exact=None):
    x = x0.detach().to(dtype).requires_grad_(True)
    sdf, feat, grad = 0, 0, 0
    for which in nets:
        out = _sdf_net(params, NETS[which], getattr(cfg, which), x, x0, dtype, exact)
        s = out[:, 0]
        (g,) = torch.autograd.grad(s, x, torch.ones_like(s), create_graph=True)
        sdf, feat, grad = sdf + s, feat + out[:, 1:], grad + g
    return x, sdf, feat, grad


def _exact(grid):
    assert grid in ("linear", "exact"), grid
    return ExactGrids() if grid == "exact" else None


def sdf_forward(params, cfg, x0, nets=("coarse", "fine"), dtype=F64, grid="linear"):
    """-> sdf [P], grad sdf [P,3], feature [P,64] of the networks in ``nets`` (summed: the COMBINE for both)."""
    _x, sdf, feat, grad = _sdf_graph(params, cfg, x0, nets, dtype, _exact(grid))
    return sdf.detach(), grad.detach(), feat.detach()


def _sdf_objective(sdf, feat, grad, g_sdf, g_feat, g_grad, dtype):
    obj = 0
    for g, y in ((g_sdf, sdf), (g_feat, feat), (g_grad, grad)):
        if g is not None:
            obj = obj + (g.to(dtype) * y).sum()
    return obj


def sdf_backward(params, cfg, x0, g_sdf=None, g_feat=None, g_grad=None, nets=("coarse", "fine"), dtype=F64, grid="linear"):
    """d/dx of  g_sdf . sdf + g_feat . feature + g_grad . grad sdf  (any cotangent may be None = absent) -> [P,3]."""
    x, sdf, feat, grad = _sdf_graph(params, cfg, x0, nets, dtype, _exact(grid))
    obj = _sdf_objective(sdf, feat, grad, g_sdf, g_feat, g_grad, dtype)
    if not torch.is_tensor(obj):
        return torch.zeros_like(x).detach()
    (gx,) = torch.autograd.grad(obj, x)
    return gx


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


def _colour_graph(params, cfg, x0, normals, dirs, feats, grid_grad, dtype, exact=None):
    x, n, d, f = (t.detach().to(dtype).requires_grad_(True) for t in (x0, normals, dirs, feats))
    gf = _grid(exact, "colour", x, x0, params["rendering_network.encoding.embeddings"], cfg.colour_grid, cfg.colour_divide_factor, dtype)
    if not grid_grad:                     # color_stage == "base": the colour grid feature is detached (base_networks.py:337-339)
        gf = gf.detach()
    h = torch.cat([x, _pe(d, cfg.multires_view), n, f, gf], dim=-1)
    for l in range(cfg.colour_n_linear):
        h = _lin(params, f"rendering_network.lin{l}", h, dtype)
        if l < cfg.colour_n_linear - 1:
            h = torch.relu(h)
    return (x, n, d, f), torch.sigmoid(h)


def colour_forward(params, cfg, x0, normals, dirs, feats, dtype=F64):
    """-> rgb [P,3]."""
    with torch.no_grad():
        return _colour_graph(params, cfg, x0, normals, dirs, feats, False, dtype)[1]


def colour_backward(params, cfg, x0, normals, dirs, feats, g_rgb, grid_grad=1, dtype=F64):
    """-> dict(x, normals, dirs, feat) of d(g_rgb . rgb); grid_grad = 0 is color_stage "base"."""
    ins, rgb = _colour_graph(params, cfg, x0, normals, dirs, feats, grid_grad, dtype)
    gs = torch.autograd.grad((g_rgb.to(dtype) * rgb).sum(), ins)
    return dict(zip(("x", "normals", "dirs", "feat"), gs))


def colour_table_grad(params, cfg, x0, normals, dirs, feats, g_rgb, dtype=F64):
    """grid="exact", grid_grad = 1: -> (dict(x, normals, dirs, feat), d/d colour table [rows, 2], plan) of d(g_rgb . rgb)."""
    exact = ExactGrids()
    ins, rgb = _colour_graph(params, cfg, x0, normals, dirs, feats, 1, dtype, exact)
    gs = torch.autograd.grad((g_rgb.to(dtype) * rgb).sum(), ins + (exact.tables["colour"],))
    return dict(zip(("x", "normals", "dirs", "feat"), gs[:4])), gs[4], exact.plans["colour"]
