"""The MLP kernels of the render core through the C ABI, for the suites that hold them to float64 (test infrastructure):
tests/test_gemm_float64_gpu.py (fp32 operands), tests/test_gemm_bf16_gpu.py (Net(precision="bf16"): every k_* helper then calls the
nsa_*_bf16 entry point itself) and, for single kernels, tests/test_grid_float64_gpu.py.  Inputs are explicit fp32 points (colour
kernels: one sample per ray at z = 0, so x = o exactly); operands come from tests/gemm_cases.py.  The check_* functions are the
bit-for-bit properties that need no reference, shared by the fp32 and the bf16 suite; for the _params entries they cover the
emission buffer too, region by region (tests/emit_rows.py names the regions and says which are functions of the point alone)."""
import ctypes
import os
import re

import numpy as np
import torch

import emit_rows
from devcall import ptr, st
from gemm_cases import colour_inputs, cot, cube_points, scaled
from helpers import load, params_of, oracle_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the network
def perturbed(name="full_vis_eval", edit=None, seed=0):
    """-> (fixture, oracle config, parameters) of a golden model with every weight_v perturbed, optionally edited (CPU only)"""
    fx = dict(load(name))
    g = torch.Generator().manual_seed(seed)
    for k in sorted(fx):
        if k.startswith("param_") and k.endswith("weight_v"):
            v = torch.from_numpy(np.array(fx[k]))
            fx[k] = (v + 0.05 * torch.randn(v.shape, generator=g)).numpy()
    if edit:
        edit(fx, g)
    return fx, oracle_config(fx), params_of(fx)


def fn(net, name):
    """the entry point ``name`` for ``net``: the public one, or (Net(precision="bf16")) its bf16-operand twin, called directly"""
    from nicer_slam_amd._native import lib
    base = getattr(lib, name)
    if not net.suffix:
        return base
    twin = getattr(lib, name + net.suffix)
    twin.restype, twin.argtypes = base.restype, base.argtypes
    return twin


class Net:
    """A golden model's parameters with every weight_v perturbed (so that all input columns matter), optionally edited, on the CPU
    (references) and the GPU (kernels)."""

    def __init__(self, name="full_vis_eval", edit=None, seed=0, precision="fp32"):
        from test_model_cpu import build_model
        fx, self.cfg, self.params = perturbed(name, edit, seed)
        self.fx = fx
        self.model = build_model(fx).cuda().eval()
        for p in self.model.parameters():
            p.requires_grad_(False)
        # "bf16": the grid descriptors say precision 1 and every k_* helper below calls the nsa_*_bf16 entry point itself
        assert precision in ("fp32", "bf16"), precision
        self.model.mlp_precision = precision
        self.suffix = "_bf16" if precision == "bf16" else ""

    def sdf(self, which, tile):
        from nicer_slam_amd.fused import sampler as fs
        self.model.sdf_tile = tile
        gd, keep = fs.sdf_grid_desc(self.model, which)
        return gd, keep, fs.packed_sdf(self.model, which)

    def colour(self):
        from nicer_slam_amd.fused import render as fr, sampler as fs
        m = self.model
        gd, keep = fs.grid_desc(m.rendering_network.encoding, m.rendering_network.divide_factor, 2, fs.precision_of(m, "colour"))
        return gd, keep, fr.packed_colour(m)


def hl(P):
    from nicer_slam_amd.fused import render as fr
    return fr.hl_index(P, "cuda")


def to_hl(v):
    from nicer_slam_amd.fused import render as fr
    P = v.shape[0]
    buf = torch.zeros(fr.hl_size(P), device="cuda")
    buf[hl(P)] = v.cuda()
    return buf


def explicit(x):
    from nicer_slam_amd._native import PointsDesc
    return PointsDesc(None, None, None, x.data_ptr(), x.shape[0], 0, None)


def one_per_ray(o, d):
    """rays with ONE sample at z = 0: x = o + 0 d = o exactly, view dir d (the colour kernels need rays)"""
    from nicer_slam_amd._native import PointsDesc
    z = torch.zeros(o.shape[0], 1, device="cuda")
    return PointsDesc(o.data_ptr(), d.data_ptr(), z.data_ptr(), None, o.shape[0], 1, None), z


# ------------------------------------------------------------------------------------------------------------------ kernels
def k_sdf_forward(net, which, tile, x, accumulate=0, init=None):
    from nicer_slam_amd._native import lib, check
    P = x.shape[0]
    xd = x.cuda().contiguous()
    gd, _keep, pk = net.sdf(which, tile)
    sdf = torch.zeros(P, device="cuda") if init is None else init[0].cuda().clone()
    grad = torch.zeros(P, 3, device="cuda") if init is None else init[1].cuda().clone()
    feat = torch.zeros(((P + 31) // 32) * 2048, device="cuda") if init is None else to_hl(init[2])
    pts = explicit(xd)
    check(fn(net, "nsa_sdfnet_forward")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), accumulate, sdf.data_ptr(), grad.data_ptr(),
                                 feat.data_ptr(), st()))
    torch.cuda.synchronize()
    return dict(sdf=sdf.cpu(), grad=grad.cpu(), feat=feat[hl(P)].cpu())


def k_sdf_pair(net, x):
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import sampler as fs
    P = x.shape[0]
    xd = x.cuda().contiguous()
    net.model.sdf_tile = 16
    gc, kc = fs.sdf_grid_desc(net.model, "coarse", "coarse_pair")
    gf, kf = fs.sdf_grid_desc(net.model, "fine")
    pc, pf = fs.packed_sdf(net.model, "coarse", use="coarse_pair"), fs.packed_sdf(net.model, "fine")
    sdf, grad = torch.full((P,), float("nan"), device="cuda"), torch.full((P, 3), float("nan"), device="cuda")
    feat = torch.zeros(((P + 31) // 32) * 2048, device="cuda")
    pts = explicit(xd)
    check(fn(net, "nsa_sdfnet_forward_pair")(ctypes.byref(pts), ctypes.byref(gc), ctypes.byref(gf), pc.data_ptr(), pf.data_ptr(),
                                      sdf.data_ptr(), grad.data_ptr(), feat.data_ptr(), st()))
    torch.cuda.synchronize()
    return dict(sdf=sdf.cpu(), grad=grad.cpu(), feat=feat[hl(P)].cpu())


def k_sdf_backward(net, which, tile, x, g_sdf=None, g_feat=None, g_grad=None, accumulate=0, init=None, params=False):
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import mapping
    P = x.shape[0]
    xd = x.cuda().contiguous()
    gd, _keep, pk = net.sdf(which, tile)
    gs = g_sdf.cuda().contiguous() if g_sdf is not None else None
    gf = to_hl(g_feat) if g_feat is not None else None
    gg = g_grad.cuda().contiguous() if g_grad is not None else None
    g_x = torch.zeros(P, 3, device="cuda") if init is None else init.cuda().clone()
    pts = explicit(xd)
    if not params:
        check(fn(net, "nsa_sdfnet_backward")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), ptr(gs), ptr(gf), ptr(gg), accumulate,
                                      g_x.data_ptr(), st()))
        torch.cuda.synchronize()
        return dict(x=g_x.cpu())
    rows = fn(net, "nsa_sdfnet_emit_rows_tile")(gd.n_hidden, tile)
    assert rows > 0
    emit = torch.full((rows, mapping.emit_ld(P)), float("nan"), device="cuda")
    check(fn(net, "nsa_sdfnet_backward_params")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), ptr(gs), ptr(gf), ptr(gg), accumulate,
                                         g_x.data_ptr(), None, emit.data_ptr(), emit.shape[1], st()))
    torch.cuda.synchronize()
    return dict(x=g_x.cpu()), emit


def k_colour_forward(net, x, d, normals, feat):
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import render as fr
    P = x.shape[0]
    o, dd = x.cuda().contiguous(), d.cuda().contiguous()
    pts, _z = one_per_ray(o, dd)
    gd, _keep, pk = net.colour()
    grad, fh = normals.cuda().contiguous(), to_hl(feat)
    rgb = torch.full((P, 3), float("nan"), device="cuda")
    save = torch.zeros(fr.save_size(P), device="cuda")
    check(fn(net, "nsa_colour_forward")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), fh.data_ptr(), rgb.data_ptr(),
                                 save.data_ptr(), st()))
    torch.cuda.synchronize()
    return rgb.cpu(), (o, dd, _z, grad, fh, save)


def k_colour_backward(net, x, d, normals, feat, g_rgb, grid_grad, kind="plain", coarse_tile=32, g_sdf=None):
    """kind: plain (nsa_colour_backward), params (nsa_colour_backward_params), coarse (nsa_colour_coarse_backward: + the coarse SDF
    backward of the same points with g_sdf and the feature / normal cotangents just written)"""
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import mapping
    P = x.shape[0]
    _rgb, (o, dd, z, grad, fh, save) = k_colour_forward(net, x, d, normals, feat)
    pts, _z = one_per_ray(o, dd)
    gd, _keep, pk = net.colour()
    gr = g_rgb.cuda().contiguous()
    g_feat = torch.full((((P + 31) // 32) * 2048,), float("nan"), device="cuda")
    g_grad = torch.zeros(P, 3, device="cuda")
    g_x, g_dir = torch.full((P, 3), float("nan"), device="cuda"), torch.full((P, 3), float("nan"), device="cuda")
    emit = None
    if kind == "plain":
        check(fn(net, "nsa_colour_backward")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), fh.data_ptr(), save.data_ptr(),
                                      gr.data_ptr(), grid_grad, g_feat.data_ptr(), g_grad.data_ptr(), g_x.data_ptr(), g_dir.data_ptr(),
                                      st()))
    elif kind == "params":
        emit = torch.full((fn(net, "nsa_colour_emit_rows")(), mapping.emit_ld(P)), float("nan"), device="cuda")
        check(fn(net, "nsa_colour_backward_params")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), fh.data_ptr(),
                                             save.data_ptr(), gr.data_ptr(), grid_grad, g_feat.data_ptr(), g_grad.data_ptr(),
                                             g_x.data_ptr(), g_dir.data_ptr(), None, emit.data_ptr(), emit.shape[1], st()))
    else:
        gc, _kc, pc = net.sdf("coarse", coarse_tile)
        gs = g_sdf.cuda().contiguous()
        check(fn(net, "nsa_colour_coarse_backward")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), fh.data_ptr(),
                                             save.data_ptr(), gr.data_ptr(), grid_grad, g_feat.data_ptr(), g_grad.data_ptr(),
                                             g_x.data_ptr(), g_dir.data_ptr(), ctypes.byref(gc), pc.data_ptr(), gs.data_ptr(), st()))
    torch.cuda.synchronize()
    out = dict(feat=g_feat[hl(P)].cpu(), normals=g_grad.cpu(), x=g_x.cpu(), dirs=g_dir.cpu())
    return (out, emit) if kind == "params" else out


# ------------------------------------------------------------------------------------------------------------------ properties
def emit_outputs(emit, P, regions):
    """the emission buffer as outputs of a run: "emit <region>" -> [P, rows] on the host (a point's column as a row)"""
    return {f"emit {name}": emit[r0:r0 + n, :P].t().contiguous().cpu() for name, (r0, n, _point_only) in regions.items()}


def sdf_regions(net, which, tile):
    gd, _keep, _pk = net.sdf(which, tile)
    return emit_rows.sdf_regions(gd.n_hidden, tile)


def point_only(key):
    """is this output of a _params run a function of the point alone (untouched by the cotangents)?"""
    name = key[5:] if key.startswith("emit ") else None
    return name is not None and (name in ("IN", "H0") or name[0] == "H" or name[:2] == "DA")


def _sdf_params_run(net, which, tile, x, gs, gf, gg):
    out, emit = k_sdf_backward(net, which, tile, x, gs, gf, gg, params=True)
    out.update(emit_outputs(emit, x.shape[0], sdf_regions(net, which, tile)))
    return out


def _colour_params_run(net, xc, d, normals, feat, g_rgb, grid_grad):
    out, emit = k_colour_backward(net, xc, d, normals, feat, g_rgb, grid_grad, kind="params")
    out.update(emit_outputs(emit, xc.shape[0], emit_rows.colour_regions()))
    return out


def backward_runs(net, x, xc, d, normals, feat):
    """name -> f(scale [P]) running one backward kernel with every cotangent of point p multiplied by scale[p]"""
    P = x.shape[0]
    base = (cot(P, 50, ()), cot(P, 51, (64,)), cot(P, 52, (3,)))
    g_rgb, g_sdf = cot(P, 53, (3,)), cot(P, 54, ())
    runs = {}
    for which in ("coarse", "fine"):
        for tile in (16, 32):
            runs[f"sdfnet_backward {which} t{tile}"] = (
                lambda s, which=which, tile=tile: k_sdf_backward(net, which, tile, x, *(scaled(b, s) for b in base)))
            runs[f"sdfnet_backward_params {which} t{tile}"] = (
                lambda s, which=which, tile=tile: _sdf_params_run(net, which, tile, x, *(scaled(b, s) for b in base)))
    for grid_grad in (0, 1):
        runs[f"colour_backward gg {grid_grad}"] = (
            lambda s, grid_grad=grid_grad: k_colour_backward(net, xc, d, normals, feat, scaled(g_rgb, s), grid_grad))
        runs[f"colour_backward_params gg {grid_grad}"] = (
            lambda s, grid_grad=grid_grad: _colour_params_run(net, xc, d, normals, feat, scaled(g_rgb, s), grid_grad))
        runs[f"colour_coarse_backward gg {grid_grad}"] = (
            lambda s, grid_grad=grid_grad: k_colour_backward(net, xc, d, normals, feat, scaled(g_rgb, s), grid_grad, kind="coarse",
                                                             g_sdf=scaled(g_sdf, s)))
    return runs


def check_backwards_point_independent(net, P):
    """every backward kernel at P points, bit for bit: other points' cotangents change nothing (a point whose cotangents are all zero
    comes out exactly 0), and cotangents x 2^k (k = -40, -13, 17, 40) scale every output by exactly 2^k.  The _params runs also
    return their emission buffer, one output per region: the cotangent regions (TIN, TH_k, AB_k, FB; colour AB1, AB2, OB) obey the
    same three rules (scaling exact from 2^-102 on: below, terms lost to fp32 underflow show), the point-only regions (H0, H_k, DA_k; colour
    IN, H1, H2) must not move at all."""
    x = cube_points(P, 60)
    xc, d, normals, feat = colour_inputs(net, P, 61)
    ones = torch.ones(P).double()
    odd = torch.arange(P) % 2 == 1
    g = torch.Generator().manual_seed(62)
    other = torch.where(odd, torch.exp2(torch.randint(0, 3, (P,), generator=g).double() * 40 - 40), ones)   # 2^-40, 1, 2^40
    other[odd & (torch.arange(P) % 3 == 0)] = 0.0
    for name, run in backward_runs(net, x, xc, d, normals, feat).items():
        ref = run(ones)
        moved = run(other)
        for k in ref:
            assert torch.equal(moved[k][~odd], ref[k][~odd]), f"{name}: other points' cotangents change d/d {k}"
            if k.startswith("emit "):
                if point_only(k):
                    assert torch.equal(moved[k], ref[k]), f"{name}: the cotangents change the point-only region {k}"
                else:
                    assert bool((moved[k][other == 0] == 0).all()), f"{name}: a point with all-zero cotangents has a non-zero {k}"
        for kexp in (-40, -13, 17, 40):
            s = torch.where(odd, torch.full((P,), 2.0 ** kexp).double(), ones)
            out = run(s)
            for k in ref:
                want = ref[k].double() if point_only(k) else ref[k].double() * s.reshape((-1,) + (1,) * (ref[k].dim() - 1))
                got = out[k].double()
                if k.startswith("emit "):
                    # Scaling is exact as long as nothing underflows, in EITHER run.  A Softplus slope of 1e-34 times a tangent is a
                    # legitimate emission entry (TH_k, and a term of AB_k = sp' acc + e_k); it, or 2^-40 times it, lies below the
                    # smallest normal fp32 number 2^-126, where an fp32 product loses bits or is flushed.  Such a term moves a sum by up
                    # to its own size, which a sum below 2^24 x 2^-126 can see: where the entry of either run is below 2^-102 it only
                    # has to be within 2^-125 (two lost terms; times 2^k if they were lost in the unscaled run), from there on exact.
                    sk = s.reshape((-1,) + (1,) * (ref[k].dim() - 1))
                    under = torch.minimum(ref[k].double().abs(), want.abs()) < 2.0 ** -102
                    off = ((got - want).abs() / sk.clamp_min(1.0).expand_as(got))[under]
                    assert bool((off <= 2.0 ** -125).all()), \
                        f"{name}: cotangents x 2^{kexp}: an entry of {k} in the underflow range is off by {float(off.max()):.3e}"
                    got, want = got[~under], want[~under]
                    bad = got != want
                    assert not bool(bad.any()), (f"{name}: cotangents x 2^{kexp} do not scale {k} by 2^{kexp}: {int(bad.sum())} entries, "
                                                 f"got {got[bad][:4].tolist()} want {want[bad][:4].tolist()}")
                assert torch.equal(got, want), \
                    f"{name}: cotangents x 2^{kexp} do not scale d/d {k} by 2^{kexp}: {int((got != want).sum())} entries"


def check_forwards_point_independent(net):
    """every forward kernel and the sampler, bit for bit: other points' (rays') inputs change nothing"""
    P = 4097
    x = cube_points(P, 70)
    odd = torch.arange(P) % 2 == 1
    x2 = x.clone()
    x2[odd] = cube_points(P, 71)[odd]
    for which in ("coarse", "fine"):
        for tile in (16, 32):
            a, b = k_sdf_forward(net, which, tile, x), k_sdf_forward(net, which, tile, x2)
            for k in a:
                assert torch.equal(a[k][~odd], b[k][~odd]), f"sdfnet_forward {which} t{tile}: other points' positions change {k}"
    a, b = k_sdf_pair(net, x), k_sdf_pair(net, x2)
    for k in a:
        assert torch.equal(a[k][~odd], b[k][~odd]), f"sdfnet_forward_pair: other points' positions change {k}"
    xc, d, normals, feat = colour_inputs(net, P, 72)
    xc2, d2, n2, f2 = colour_inputs(net, P, 73)
    sw = lambda u, v: torch.where(odd.reshape((-1,) + (1,) * (u.dim() - 1)), v, u).contiguous()
    a, _ = k_colour_forward(net, xc, d, normals, feat)
    b, _ = k_colour_forward(net, sw(xc, xc2), sw(d, d2), sw(normals, n2), sw(feat, f2))
    assert torch.equal(a[~odd], b[~odd]), "colour_forward: other points' inputs change rgb"
    # the sampler: other rays' origins, directions and jitter changed (ragged ray count)
    from nicer_slam_amd.fused import sampler as fs
    g = torch.Generator().manual_seed(74)
    Rn, E = 261, net.model.ray_sampler.N_samples_eval
    rays = [(((torch.rand(Rn, 3, generator=g) * 2 - 1) * 0.8), torch.nn.functional.normalize(torch.randn(Rn, 3, generator=g), dim=-1),
             torch.rand(Rn, E, generator=g)) for _ in range(2)]
    odd_r = torch.arange(Rn) % 2 == 1
    mixed = [torch.where(odd_r.reshape((-1,) + (1,) * (u.dim() - 1)), v, u).contiguous() for u, v in zip(*rays)]
    for tile in (16, 32, 64):
        net.model.sdf_tile = tile
        a = fs.sampler_sdf(net.model, *(t.cuda() for t in rays[0]))
        b = fs.sampler_sdf(net.model, *(t.cuda() for t in mixed))
        for u, v, what in zip(a, b, ("z", "sdf", "far")):
            assert torch.equal(u[~odd_r.cuda()], v[~odd_r.cuda()]), f"sampler_sdf tile {tile}: other rays change {what}"


# ------------------------------------------------------------------------------------------------------------------ persistent kernels
def persistent_sweep():
    """points of one sweep of the persistent kernels: CU count x waves per workgroup x 16 (both read, not assumed)"""
    src = open(os.path.join(ROOT, "nicer_slam_amd", "csrc", "render_sdfnet4.hip")).read()
    nw = {k: int(re.search(r"#define\s+" + k + r"\s+(\d+)", src).group(1)) for k in ("NSA_NW4_PAIR", "NSA_NW4_BWD")}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * max(nw.values()) * 16


def long_inputs(n):
    """a ragged shape past one sweep whose first n points are cube_points(n, 5) -> P, x, g_sdf, g_feat, g_grad"""
    P = persistent_sweep() * 5 // 4 + 11
    x = torch.cat([cube_points(n, 5), cube_points(P - n, 95)]).contiguous()
    gs, gf, gg = cot(P, 96, ()), cot(P, 97, (64,)), cot(P, 98, (3,))
    return P, x, gs, gf, gg


def resident_child(path, n):
    """(child process) bf16 pair forward and fine backward on the long shape and on P = 1, 17, 33 -> path"""
    net = Net(precision="bf16")
    P, x, gs, gf, gg = long_inputs(n)
    out = {}
    for p in (P, 1, 17, 33):
        f = k_sdf_pair(net, x[:p].contiguous())
        out.update({f"pair {p} {k}": v for k, v in f.items()})
        out[f"bwd {p}"] = k_sdf_backward(net, "fine", 16, x[:p].contiguous(), gs[:p], gf[:p], gg[:p])["x"]
    torch.save(out, path)
