"""Every bf16-operand MLP kernel (csrc/*_bf16.hip, NSA_PIECES == 1: the twelve nsa_*_bf16 entry points of csrc/bf16_entries.hpp, each
called DIRECTLY) against the float64-accumulating bf16 reference (tests/ref64.py, quant mode), per point.

The launch helpers, input builders and cotangent families are the fp32 suite's (tests/mlp_calls.py, tests/gemm_cases.py; Net(precision="bf16") makes them
call the _bf16 twins); the gate is tests/bf16_gate.py's: kept points (rounding margin >= THRESHOLD) are held to the fp32
yardstick with no flip allowance, left-out points to the tensor's largest bf16 effect, with caps on how many points may be loose.
tests/test_ref64_bf16_cpu.py fixes THRESHOLD on the CPU and shows that the gate refuses four subtly wrong emulations.
The reference takes the effective fp32 weight matrices from the device (ref64.weights_of_model).

Shapes: N = 4 123 points (128 x 32 + 27: ragged for both tilings) wherever there is a reference; prefixes P = 1, 15, 17, 31, 33; one
reference-free shape past a single sweep of the persistent kernels (1.25 x CUs x waves per workgroup x 16 points + 11).
Without a reference, for ALL points and bit for bit: point independence (prefixes, other points' inputs changed, the long shape's
first N points), scale equivariance of every backward (cotangents x 2^k), zero cotangents -> zero output, nothing non-finite.

_params twins: wherever the plain and the _params entry take the same path the d/dx must agree bit for bit, as in the fp32 suite --
(coarse, 16), (fine, 32) (one template, MAP false / true) and also (fine, 16), which is new here: the plain entry runs the resident
persistent kernel k_sdfnet4_bwd_res, the _params entry the staged k_sdfnet4_bwd<.., MAP = true>.  Those are two kernel functions around
the same statements (sdfnet4_bwd_body.inc); under the compiler's default contraction each fused a * b + c on its own terms and the pair
differed at 2 of 4 123 points (a last-bit difference in front of a bf16 rounding is a flip).  render_sdfnet4_bf16.hip now compiles
under `fp contract(on)` -- fusion inside one expression only, the same in every function that includes the statements -- so
bit-identity is the right demand and is what is asserted.  (coarse, 32) recomputes the grid Jacobian in the plain kernel and reads
the stored one in the MAP kernel (the fp32 suite's LDS_JACOBIAN_ONLY_IN_MAP: other sums, 143 of 4 123 points differ): that pair
goes through the gate.

EMISSION ROWS of the _params twins (section "emission rows"): per point and per layer the [dW_l | db_l] they encode against ref64's
per-point weight gradients in quant mode, both fp32 summation orders as yardsticks; measured figures in DESIGN 7.

MEASURED on the MI355X (N = 4 123, threshold 3; e_k, e_y divided by the float64 output's norm, floor 1, or by c_p):
(ranges over tilings, accumulate, grid_grad and cotangent families; `cases` = how many gate lines a row sums up)
| kernel: output | cases | e_k rms | e_k max | e_y rms | e_y max | kept share | loose share (max) | flip / effect (max) |
|---|---|---|---|---|---|---|---|---|
| `sdfnet_forward_bf16 coarse: sdf` | 4 | 5.2e-08 .. 5.3e-08 | 1.8e-07 .. 1.9e-07 | 4.4e-08 .. 4.8e-08 | 1.9e-07 | 0.89 | 0.0010 | 0.13 |
| `sdfnet_forward_bf16 coarse: grad` | 4 | 9.7e-08 .. 1.2e-07 | 3.9e-07 .. 5.0e-07 | 1.4e-07 .. 1.7e-07 | 7.4e-07 | 0.89 | 0.0010 | 0.05 |
| `sdfnet_forward_bf16 coarse: feat` | 4 | 3.5e-08 .. 1.2e-07 | 2.1e-07 .. 1.7e-06 | 6.8e-08 .. 3.3e-07 | 1.3e-07 .. 8.6e-07 | 0.89 | 0.0015 | 0.15 |
| `sdfnet_forward_bf16 fine: sdf` | 4 | 5.7e-08 .. 6.2e-08 | 1.9e-07 .. 3.6e-07 | 4.7e-08 .. 5.2e-08 | 2.0e-07 | 0.68 | 0.0022 | 0.27 |
| `sdfnet_forward_bf16 fine: grad` | 4 | 1.1e-07 .. 1.2e-07 | 4.7e-07 .. 5.7e-07 | 1.5e-07 .. 1.6e-07 | 7.2e-07 .. 8.2e-07 | 0.68 | 0.0039 | 0.12 |
| `sdfnet_forward_bf16 fine: feat` | 4 | 3.7e-08 .. 1.2e-07 | 2.4e-07 .. 1.8e-06 | 6.7e-08 .. 2.6e-07 | 1.3e-07 .. 6.7e-07 | 0.68 | 0.0034 | 0.46 |
| `sdfnet_forward_pair_bf16: sdf` | 1 | 9.5e-08 | 7.3e-07 | 6.6e-08 | 2.4e-07 | 0.61 | 0.0024 | 0.26 |
| `sdfnet_forward_pair_bf16: grad` | 1 | 1.2e-07 | 6.6e-07 | 1.7e-07 | 8.0e-07 | 0.61 | 0.0036 | 0.07 |
| `sdfnet_forward_pair_bf16: feat` | 1 | 1.3e-07 | 1.9e-06 | 2.8e-07 | 8.5e-07 | 0.61 | 0.0034 | 0.22 |
| `sampler_sdf_bf16: sdf` | 3 | 6.1e-08 .. 8.9e-08 | 2.8e-07 .. 3.4e-07 | 6.6e-08 | 2.8e-07 | 0.63 | 0.0022 | 0.06 |
| `sdf_points_bf16: sdf` | 3 | 6.1e-08 .. 8.9e-08 | 2.8e-07 .. 3.4e-07 | 6.6e-08 | 2.8e-07 | 0.63 | 0.0022 | 0.06 |
| `sdfnet_backward_bf16 coarse: x` | 16 | 1.8e-07 .. 2.8e-05 | 1.3e-06 .. 3.8e-04 | 2.8e-07 .. 3.7e-05 | 2.0e-06 .. 4.9e-04 | 0.23 .. 0.84 | 0.0049 | 0.07 |
| `sdfnet_backward_bf16 fine: x` | 16 | 3.1e-07 .. 4.7e-05 | 2.0e-06 .. 5.5e-04 | 4.5e-07 .. 6.3e-05 | 3.1e-06 .. 6.6e-04 | 0.12 .. 0.57 | 0.0186 | 0.07 |
| `colour_forward_bf16: rgb` | 1 | 3.8e-08 | 7.9e-08 | 3.7e-08 | 7.9e-08 | 0.98 | 0.0010 | 0.00 |
| `colour_backward_bf16: feat` | 2 | 1.0e-09 | 3.3e-09 | 1.1e-09 | 4.2e-09 | 0.96 | 0.0012 | 0.01 |
| `colour_backward_bf16: normals` | 2 | 2.4e-10 | 1.9e-09 | 2.7e-10 | 1.9e-09 | 0.96 | 0.0012 | 0.00 |
| `colour_backward_bf16: x` | 2 | 2.2e-10 .. 1.4e-08 | 1.2e-09 .. 7.4e-08 | 2.5e-10 .. 1.2e-08 | 1.5e-09 .. 6.2e-08 | 0.96 | 0.0012 | 0.01 |
| `colour_backward_bf16: dirs` | 2 | 3.9e-09 | 1.9e-08 | 4.8e-09 | 2.2e-08 | 0.96 | 0.0012 | 0.00 |
| `colour_coarse_backward_bf16: x` | 2 | 1.9e-07 .. 1.9e-07 | 1.1e-06 .. 1.3e-06 | 2.9e-07 .. 2.9e-07 | 2.2e-06 .. 2.2e-06 | 0.77 | 0.0029 | 0.01 |
| `sdfnet_backward_params_bf16 coarse: x` | 2 | 7.3e-06 .. 7.7e-06 | 4.3e-05 .. 7.5e-05 | 1.1e-05 | 9.1e-05 | 0.78 | 0.0042 | 0.00 |
| `sdfnet_backward_params_bf16 fine: x` | 1 | 1.2e-05 | 6.2e-05 | 1.7e-05 | 1.0e-04 | 0.40 | 0.0154 | 0.03 |
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import bf16_cases as C
import bf16_gate as G
import emit_rows
import ref64
from devcall import st
from gemm_cases import cot
from mlp_calls import (Net, check_backwards_point_independent, check_forwards_point_independent, emit_outputs, fn, k_colour_backward,
                       k_colour_forward, k_sdf_backward, k_sdf_forward, k_sdf_pair, long_inputs, persistent_sweep, sdf_regions, to_hl)

pytestmark = pytest.mark.gpu

N = C.N
PREFIXES = (1, 15, 17, 31, 33)
GATED_PARAMS_TWINS = {("coarse", 32)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net():
    return Net(precision="bf16")


class Refs:
    """the references of every case, each built once per module (four ref64 evaluations) and left unchanged"""

    def __init__(self, net):
        self.weights = ref64.weights_of_model(net.model)
        self.cases = C.all_cases(net.params, net.cfg)
        self.inp = C.inputs(net.params, net.cfg)
        self._refs = {}

    def __call__(self, name):
        if name not in self._refs:
            self._refs[name] = C.refs(self.cases[name][0], self.weights)
        return self._refs[name]

    def gate(self, what, name, got, fails, norm=None, add=None, keys=None):
        """every output of ``got`` against case ``name``; add: {output: tensor} added to all three references (accumulate = 1)"""
        _call, c, backward, colour = self.cases[name]
        r = self(name)
        keep = C.kink_keep(r) if colour else None
        for k in (keys or got):
            b64, y32, f64 = ((t[k].double() + add[k].double()) if add else t[k] for t in (r.b64, r.y32, r.f64))
            n = norm if norm is not None else (c if c is not None else G.fwd_norm(b64))
            G.gate(f"{what}: {k}", got[k], b64, y32, f64, n, r.margin, backward, keep, failures=fails)


@pytest.fixture(scope="module")
def refs(net):
    return Refs(net)


def _done(fails):
    assert not fails, [(f["what"], f.get("why")) for f in fails]


# ------------------------------------------------------------------------------------------------------------------ SDF forward
@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_sdf_forward_bf16_vs_float64(net, refs, which, capsys):
    x = refs.inp.xf
    g = torch.Generator().manual_seed(2)
    init = dict(sdf=torch.randn(N, generator=g), grad=torch.randn(N, 3, generator=g), feat=torch.randn(N, 64, generator=g))
    fails = []
    with capsys.disabled():
        print()
        for tile in (16, 32):
            for acc in (0, 1):
                out = k_sdf_forward(net, which, tile, x, acc, (init["sdf"], init["grad"], init["feat"]) if acc else None)
                refs.gate(f"sdfnet_forward_bf16 {which} t{tile} acc {acc}", f"sdf forward {which}", out, fails, add=init if acc else None)
                if acc == 0:
                    for P in PREFIXES:
                        small = k_sdf_forward(net, which, tile, x[:P].contiguous())
                        for k in small:
                            assert torch.equal(small[k], out[k][:P]), f"{which} tile {tile}: P = {P} changes {k}"
    _done(fails)


def test_sdf_forward_pair_bf16_vs_float64(net, refs, capsys):
    x = refs.inp.xf
    fails = []
    with capsys.disabled():
        print()
        out = k_sdf_pair(net, x)
        refs.gate("sdfnet_forward_pair_bf16 (resident)", "sdf forward pair", out, fails)
    for P in PREFIXES:
        small = k_sdf_pair(net, x[:P].contiguous())
        for k in small:
            assert torch.equal(small[k], out[k][:P]), f"pair: P = {P} changes {k}"
    _done(fails)


# ------------------------------------------------------------------------------------------------------------------ the sampler
def k_sampler(net, tile, o, d, t_rand):
    """nsa_sampler_sdf_bf16 -> z [R,E], sdf [R,E], far [R] (fused/sampler.py::sampler_sdf with the entry point called directly)"""
    from nicer_slam_amd._native import check
    from nicer_slam_amd.fused import sampler as fs
    m = net.model
    m.sdf_tile = tile
    us = m.ray_sampler.uniform_sampler
    R, E = o.shape[0], m.ray_sampler.N_samples_eval
    gc, _kc = fs.sdf_grid_desc(m, "coarse", "sampler")
    gf, _kf = fs.sdf_grid_desc(m, "fine", "sampler")
    pc, pf = fs.packed_sdf(m, "coarse", use="sampler"), fs.packed_sdf(m, "fine", use="sampler")
    od, dd, tr = o.cuda().contiguous(), d.cuda().contiguous(), t_rand.cuda().contiguous()
    z, sdf, far = torch.empty(R, E, device="cuda"), torch.empty(R, E, device="cuda"), torch.empty(R, device="cuda")
    t_lin = torch.linspace(0.0, 1.0, steps=E, device="cuda")
    check(fn(net, "nsa_sampler_sdf")(od.data_ptr(), dd.data_ptr(), R, E, t_lin.data_ptr(), tr.data_ptr(), float(us.near),
                                      float(us.scene_bounding_sphere), float(us.far), ctypes.byref(gc), ctypes.byref(gf), pc.data_ptr(),
                                      pf.data_ptr(), z.data_ptr(), sdf.data_ptr(), far.data_ptr(), st()))
    torch.cuda.synchronize()
    return z.cpu(), sdf.cpu(), far.cpu()


def k_sdf_points(net, tile, x):
    """nsa_sdf_points_bf16 -> sdf [N] (inference.py::sdf_values with the entry point called directly)"""
    from nicer_slam_amd._native import check
    from nicer_slam_amd.fused import sampler as fs
    m = net.model
    m.sdf_tile = tile
    gc, _kc = fs.sdf_grid_desc(m, "coarse", "sampler")
    gf, _kf = fs.sdf_grid_desc(m, "fine", "sampler")
    pc, pf = fs.packed_sdf(m, "coarse", use="sampler"), fs.packed_sdf(m, "fine", use="sampler")
    xd = x.cuda().contiguous()
    out = torch.full((x.shape[0],), float("nan"), device="cuda")
    check(fn(net, "nsa_sdf_points")(xd.data_ptr(), x.shape[0], ctypes.byref(gc), ctypes.byref(gf), pc.data_ptr(), pf.data_ptr(),
                                     out.data_ptr(), st()))
    torch.cuda.synchronize()
    return out.cpu()


def test_sampler_and_sdf_points_bf16_vs_float64(net, capsys):
    """rays along coordinate axes with o on a 1/8 lattice (tests/test_gemm_float64_gpu.py::test_sampler_vs_float64): o + z d rounds once
    in any fp32 implementation, so the reference's points are the kernel's bit for bit"""
    from oracle import render_ref as R
    g = torch.Generator().manual_seed(4)
    E = net.model.ray_sampler.N_samples_eval
    Rn = -(-N // E)                                                   # just past N points
    axis, sign = torch.randint(3, (Rn,), generator=g), torch.randint(2, (Rn,), generator=g) * 2 - 1
    d = torch.zeros(Rn, 3)
    d[torch.arange(Rn), axis] = sign.float()
    o = torch.randint(-6, 7, (Rn, 3), generator=g).float() / 8
    t_rand = torch.rand(Rn, E, generator=g)
    fails, res, r = [], {}, None
    weights = ref64.weights_of_model(net.model)
    with capsys.disabled():
        print()
        for tile in (16, 32, 64):
            z, sdf, far = k_sampler(net, tile, o, d, t_rand)
            us = net.model.ray_sampler.uniform_sampler
            far_o = R.cube_far(o, d, float(us.scene_bounding_sphere), float(us.far)).reshape(-1)
            assert torch.equal(far, far_o), f"far plane (tile {tile}): {int((far != far_o).sum())} rays differ"
            res[tile] = z
            assert torch.equal(z, res[16]), f"tile {tile}: z differs from the quad tiling's"
            x = (o.unsqueeze(1) + z.unsqueeze(2) * d.unsqueeze(1)).reshape(-1, 3).contiguous()
            if r is None:
                r = C.refs(C.sdf_forward_case(net.params, net.cfg, x, ("coarse", "fine")), weights)
            for what, got in ((f"sampler_sdf_bf16 tile {tile}", sdf.reshape(-1)), (f"sdf_points_bf16 tile {tile}", k_sdf_points(net, tile, x))):
                G.gate(f"{what}: sdf", got, r.b64["sdf"], r.y32["sdf"], r.f64["sdf"], G.fwd_norm(r.b64["sdf"]), r.margin, False, failures=fails)
            for P in PREFIXES:
                assert torch.equal(k_sdf_points(net, tile, x[:P].contiguous()), k_sdf_points(net, tile, x)[:P]), f"sdf_points tile {tile}: P = {P}"
    _done(fails)


# ------------------------------------------------------------------------------------------------------------------ SDF backward
@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_sdf_backward_bf16_vs_float64(net, refs, which, capsys):
    x, fam = refs.inp.xb, refs.inp.fam
    init = cot(N, 40, (3,))
    fails = []
    with capsys.disabled():
        print()
        for tile in (16, 32):
            for name, (gs, gf, gg, c) in fam.items():
                out = k_sdf_backward(net, which, tile, x, gs, gf, gg)
                refs.gate(f"sdfnet_backward_bf16 {which} t{tile}: {name}", f"sdf backward {which}: {name}", out, fails)
                if name == C.UNIT:           # accumulate 1 onto O(1) values: every point of this family has c_p in [1/8, 8]
                    acc = k_sdf_backward(net, which, tile, x, gs, gf, gg, accumulate=1, init=init)
                    refs.gate(f"sdfnet_backward_bf16 {which} t{tile}: accumulate 1, c_p in [1/8, 8]", f"sdf backward {which}: {name}", acc, fails,
                              norm=torch.ones(N).double(), add=dict(x=init))
                if name == "all three x c_p":
                    for P in PREFIXES:
                        small = k_sdf_backward(net, which, tile, x[:P].contiguous(), gs[:P], gf[:P], gg[:P])["x"]
                        assert torch.equal(small, out["x"][:P]), f"{which} tile {tile}: P = {P} changes d/dx"
                if "NULL" in name:
                    assert bool(torch.isfinite(out["x"]).all()), f"{which} tile {tile}: non-finite d/dx with g_sdf alone"
    _done(fails)


# ------------------------------------------------------------------------------------------------------------------ colour
def test_colour_kernels_bf16_vs_float64(net, refs, capsys):
    i = refs.inp
    ins = (i.x, i.d, i.normals, i.feat)
    fails = []
    with capsys.disabled():
        print()
        rgb, _bufs = k_colour_forward(net, *ins)
        refs.gate("colour_forward_bf16", "colour forward", dict(rgb=rgb), fails)
        for P in PREFIXES:
            small, _b = k_colour_forward(net, *(t[:P].contiguous() for t in ins))
            assert torch.equal(small, rgb[:P]), f"colour forward: P = {P} changes rgb"
        for grid_grad in (0, 1):
            out = k_colour_backward(net, *ins, i.g_rgb, grid_grad)
            refs.gate(f"colour_backward_bf16 grid_grad {grid_grad}", f"colour backward grid_grad {grid_grad}", out, fails)
            for P in PREFIXES:
                small = k_colour_backward(net, *(t[:P].contiguous() for t in ins), i.g_rgb[:P].contiguous(), grid_grad)
                for k in small:
                    assert torch.equal(small[k], out[k][:P]), f"colour backward: P = {P} changes d/d {k}"
            outc = k_colour_backward(net, *ins, i.g_rgb, grid_grad, kind="coarse", g_sdf=i.g_sdf)
            for k in ("feat", "normals", "dirs"):
                assert torch.equal(outc[k], out[k]), f"colour_coarse_backward_bf16: d/d {k} differs from nsa_colour_backward_bf16's"
            refs.gate(f"colour_coarse_backward_bf16 grid_grad {grid_grad}", f"colour + coarse backward grid_grad {grid_grad}", dict(x=outc["x"]), fails)
    _done(fails)


def test_colour_forward_composite_and_track_bf16_write_the_plain_kernels_rgb(net):
    """nsa_colour_forward_composite_bf16 / nsa_colour_forward_track_bf16 (128 samples per ray: a workgroup of the colour forward is one
    ray, whose first wave adds the ray tail after the colours are stored): the per-sample rgb is nsa_colour_forward_bf16's bit for bit on
    the same inputs (render_colour.hip: one colour_fwd_body.inc for all three).  Their composite and loss tails belong to
    tests/test_objective_float64_gpu.py and tests/test_tiling_gpu.py."""
    from nicer_slam_amd._native import PointsDesc, check
    from nicer_slam_amd.fused import render as fr
    g = torch.Generator().manual_seed(21)
    Rn, S = 5, 128
    P = Rn * S
    o = ((torch.rand(Rn, 3, generator=g) * 2 - 1) * 0.3).cuda()
    d = torch.nn.functional.normalize(torch.randn(Rn, 3, generator=g), dim=-1).cuda()
    z = (torch.rand(Rn, S, generator=g) * 0.6).sort(dim=1).values.cuda().contiguous()
    grad, feat = torch.randn(P, 3, generator=g).cuda(), to_hl(torch.randn(P, 64, generator=g) * 0.2)
    sdf = (torch.randn(P, generator=g) * 0.05).cuda()
    gt = torch.rand(Rn, 3, generator=g).cuda()
    m = net.model
    vox = m.voxels.contiguous()
    pts = PointsDesc(o.data_ptr(), d.data_ptr(), z.data_ptr(), None, P, S, None)
    gd, _keep, pk = net.colour()
    new = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    rgb, save = {}, {}
    for kind in ("plain", "composite", "track"):
        rgb[kind], save[kind] = new(P, 3), torch.zeros(fr.save_size(P), device="cuda")
    check(fn(net, "nsa_colour_forward")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), feat.data_ptr(),
                                         rgb["plain"].data_ptr(), save["plain"].data_ptr(), st()))
    w, rv, dep, nm, ent = new(Rn, S), new(Rn, 3), new(Rn), new(Rn, 3), new(Rn)
    check(fn(net, "nsa_colour_forward_composite")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), feat.data_ptr(),
                                                   rgb["composite"].data_ptr(), save["composite"].data_ptr(), sdf.data_ptr(), vox.data_ptr(),
                                                   m.voxel_res, w.data_ptr(), rv.data_ptr(), dep.data_ptr(), nm.data_ptr(), ent.data_ptr(), st()))
    rv2, loss, g_sdf, g_rgb, g_grad = new(Rn, 3), new(Rn), new(P), new(P, 3), new(P, 3)
    check(fn(net, "nsa_colour_forward_track")(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), feat.data_ptr(),
                                               rgb["track"].data_ptr(), save["track"].data_ptr(), sdf.data_ptr(), vox.data_ptr(), m.voxel_res,
                                               gt.data_ptr(), Rn, rv2.data_ptr(), loss.data_ptr(), g_sdf.data_ptr(), g_rgb.data_ptr(),
                                               g_grad.data_ptr(), st()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rgb["plain"]).all())
    for kind in ("composite", "track"):
        assert torch.equal(rgb[kind], rgb["plain"]), f"colour_forward_{kind}_bf16: rgb differs from colour_forward_bf16's"
    # what the composite form saves for the backward (ReLU masks as bit patterns in a float buffer: compare the words)
    assert torch.equal(save["composite"].view(torch.int32), save["plain"].view(torch.int32)), "colour_forward_composite_bf16: the saved state differs"
    assert torch.equal(rv, rv2) and bool(torch.isfinite(rv).all()) and bool(torch.isfinite(loss).all())


# ------------------------------------------------------------------------------------------------------------------ _params twins
@pytest.mark.parametrize("which,tile", [("coarse", 16), ("coarse", 32), ("fine", 16), ("fine", 32)])
def test_sdf_params_bf16_data_path_and_padding(net, refs, which, tile, capsys):
    x, fam = refs.inp.xb, refs.inp.fam
    gs, gf, gg, c = fam["all three x c_p"]
    outs = {}
    for P in (33, N):
        out, emit = k_sdf_backward(net, which, tile, x[:P].contiguous(), gs[:P], gf[:P], gg[:P], params=True)
        end = -(-P // tile) * tile
        assert bool((emit[:, P:end] == 0).all()), f"sdfnet_backward_params_bf16 {which} t{tile} P={P}: padding columns are not 0"
        assert bool(torch.isfinite(emit[:, :P]).all()), f"sdfnet_backward_params_bf16 {which} t{tile} P={P}: non-finite emission rows"
        if P == N:           # the emission columns of a prefix are the big run's, bit for bit
            for n in PREFIXES:
                small = k_sdf_backward(net, which, tile, x[:n].contiguous(), gs[:n], gf[:n], gg[:n], params=True)[1]
                assert torch.equal(small[:, :n], emit[:, :n]), f"sdfnet_backward_params_bf16 {which} t{tile}: P = {n} changes the emission columns"
        del emit
        outs[P] = out["x"]
        plain = k_sdf_backward(net, which, tile, x[:P].contiguous(), gs[:P], gf[:P], gg[:P])["x"]
        diff = (out["x"] != plain).any(1)
        if (which, tile) not in GATED_PARAMS_TWINS:
            assert not bool(diff.any()), f"sdfnet_backward_params_bf16 {which} t{tile} P={P}: d/dx differs from the plain kernel's at {int(diff.sum())} points"
        elif P == N:
            with capsys.disabled():
                print(f"\n  sdfnet_backward_params_bf16 {which} t{tile}: d/dx differs from the plain kernel's at {int(diff.sum())} of {N} points")
    assert torch.equal(outs[33], outs[N][:33]), "sdfnet_backward_params_bf16: P = 33 changes d/dx"
    fails = []
    with capsys.disabled():
        refs.gate(f"sdfnet_backward_params_bf16 {which} t{tile}: all three x c_p", f"sdf backward {which}: all three x c_p", dict(x=outs[N]), fails)
    _done(fails)


@pytest.mark.parametrize("P", [33, N])
def test_colour_params_bf16_data_path_is_bit_identical_and_padding_zero(net, refs, P):
    i = refs.inp
    ins = tuple(t[:P].contiguous() for t in (i.x, i.d, i.normals, i.feat))
    g_rgb = i.g_rgb[:P].contiguous()
    for grid_grad in (0, 1):
        plain = k_colour_backward(net, *ins, g_rgb, grid_grad)
        out, emit = k_colour_backward(net, *ins, g_rgb, grid_grad, kind="params")
        end = -(-P // 32) * 32
        assert bool((emit[:, P:end] == 0).all()), "colour_backward_params_bf16: padding columns are not 0"
        for k in plain:
            assert torch.equal(out[k], plain[k]), f"colour_backward_params_bf16 grid_grad {grid_grad}: d/d {k} differs"
        if P == N:           # the emission columns of a prefix are the big run's, bit for bit
            for n in PREFIXES:
                small = k_colour_backward(net, *(t[:n].contiguous() for t in ins), g_rgb[:n].contiguous(), grid_grad, kind="params")[1]
                assert torch.equal(small[:, :n], emit[:, :n]), f"colour_backward_params_bf16 grid_grad {grid_grad}: P = {n} changes the emission columns"


# ------------------------------------------------------------------------------------------------------------------ emission rows
# The per-point vectors of the _params twins that nsa_emit_gemm multiplies into dW and db, judged BEFORE that sum (one wrong column is
# one term among thousands after it): per point and per layer the [dW_l | db_l] they encode (tests/emit_rows.py, production's row
# maps) against ref64's per-point weight gradients in quant mode -- the graphs of the d/dx cases, hence their Margin and kept sets --
# through the gate with backward = True and BOTH fp32 summation orders as yardsticks (bf16_gate.gate, ``second``); the Softplus / ReLU
# outputs H_k as forward quantities; H0 / IN, which no bf16 operand enters, through the fp32 suite's gate.  The references of a case
# are built once, serve both tilings and are dropped (some GB for the fine network).  The MAP kernels are not persistent (one tile
# per wave), so there is no sweep to run past; the production tie of the helper is the fp32 suite's (nsa_emit_gemm has no bf16 twin).
def _emission_gates(what, r, c, point, acts, keep, fails):
    for l, got in enumerate(point):
        k = C.layer(l)
        assert got.shape == r.b64[k].shape, (k, got.shape, r.b64[k].shape)
        G.gate(f"{what}: {k}", got, r.b64[k], r.y32[k], r.f64[k], c, r.margin, True, keep, failures=fails, second=r.perm[k])
    for k in range(1, len(acts)):
        b64 = r.b64[f"H{k}"]
        G.gate(f"{what}: H{k}", acts[k], b64, r.y32[f"H{k}"], r.f64[f"H{k}"], G.fwd_norm(b64), r.margin, False, keep, failures=fails)


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_sdf_emission_rows_bf16_vs_float64(net, refs, which, capsys):
    """nsa_sdfnet_backward_params_bf16 at both tilings, every cotangent family (tests/test_gemm_float64_gpu.py::
    test_sdf_emission_rows_vs_float64 states the regions): the gates above; FB is g_feat itself; TIN, TH_k, AB_k, FB are exactly 0 at
    points with all-zero cotangents and TIN, TH_k everywhere without g_grad; the point-only regions H0, H_k, DA_k are bit-identical
    across the families."""
    x, fam = refs.inp.xb, refs.inp.fam
    cases = C.weight_grad_cases(net.params, net.cfg, i=refs.inp)
    spec = getattr(net.cfg, which).grid
    L, Cdim = spec.num_levels, spec.level_dim
    h0 = tuple(ref64.sdf_first_layer_input(net.params, net.cfg, x, which, dt) for dt in (torch.float64, torch.float32))
    fails, gate64_fails, first = [], [], {}
    with capsys.disabled():
        print()
        for name, (gs, gf, gg, c) in fam.items():
            r = C.refs(cases[f"weight gradients {which}: {name}"][0], refs.weights)
            for tile in (16, 32):
                regions = sdf_regions(net, which, tile)
                NH = sum(1 for k in regions if k.startswith("AB"))
                _out, emit = k_sdf_backward(net, which, tile, x, gs, gf, gg, params=True)
                cols = emit_outputs(emit, N, regions)
                for k, v in cols.items():
                    if regions[k[5:]][2]:
                        assert torch.equal(v, first.setdefault((tile, k), v)), f"{which} t{tile}, {name}: the cotangents change the point-only region {k}"
                    else:
                        assert bool((v[c == 0] == 0).all()), f"{which} t{tile}, {name}: {k} is not 0 at a point with all-zero cotangents"
                assert torch.equal(cols["emit FB"], torch.zeros(N, 64) if gf is None else gf), f"{which} t{tile}, {name}: FB is not g_feat"
                if gg is None:
                    assert all(not bool(cols[k].any()) for k in cols if k[5:7] in ("TI", "TH")), f"{which} t{tile}, {name}: a tangent without g_grad"
                acts = emit_rows.sdf_activations(emit, N, L, Cdim, NH, tile)
                _emission_gates(f"emission rows bf16 {which} t{tile}: {name}", r, c, emit_rows.sdf_point_grads(emit, gs, N, L, Cdim, NH, tile),
                                acts, None, fails)
                if name == "all three x c_p":
                    emit_rows.gate_first_layer_input(f"emission rows bf16 {which} t{tile}: H0", acts[0], h0, L * Cdim, None, gate64_fails)
                del emit
            del r
    assert not gate64_fails, [f["what"] for f in gate64_fails]
    _done(fails)


@pytest.mark.parametrize("grid_grad", [0, 1])
def test_colour_emission_rows_bf16_vs_float64(net, refs, grid_grad, capsys):
    """nsa_colour_backward_params_bf16: the gates above off the ReLU kinks; AB1, AB2, OB exactly 0 at points with all-zero
    cotangents; IN, H1, H2 bit-identical for the other grid_grad and another g_rgb"""
    i = refs.inp
    ins = (i.x, i.d, i.normals, i.feat)
    case = C.weight_grad_cases(net.params, net.cfg, i=i)[f"weight gradients colour grid_grad {grid_grad}"]
    r = C.refs(case[0], refs.weights)
    keep = C.kink_keep(r)
    regions = emit_rows.colour_regions()
    spec = net.cfg.colour_grid
    fails, gate64_fails = [], []
    with capsys.disabled():
        print()
        _out, emit = k_colour_backward(net, *ins, i.g_rgb, grid_grad, kind="params")
        cols = emit_outputs(emit, N, regions)
        other = emit_outputs(k_colour_backward(net, *ins, C.scaled(cot(N, 16, (3,)), i.c), 1 - grid_grad, kind="params")[1], N, regions)
        for k, v in cols.items():
            if regions[k[5:]][2]:
                assert torch.equal(v, other[k]), f"colour grid_grad {grid_grad}: g_rgb or grid_grad change the point-only region {k}"
            else:
                assert bool((v[i.c == 0] == 0).all()), f"colour grid_grad {grid_grad}: {k} is not 0 at a point with all-zero cotangents"
        acts = emit_rows.colour_activations(emit, N)
        _emission_gates(f"emission rows bf16 colour grid_grad {grid_grad}", r, i.c, emit_rows.colour_point_grads(emit, N), acts, keep, fails)
        first = tuple(ref64.colour_first_layer_input(net.params, net.cfg, i.x, i.normals, i.d, i.feat, dt) for dt in (torch.float64, torch.float32))
        emit_rows.gate_first_layer_input(f"emission rows bf16 colour grid_grad {grid_grad}: IN", acts[0], first, spec.num_levels * spec.level_dim,
                                         keep, gate64_fails)
    assert not gate64_fails, [f["what"] for f in gate64_fails]
    _done(fails)


# ------------------------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("P", [33, N])
def test_bf16_backwards_are_point_independent_and_scale_equivariant_bit_for_bit(net, P):
    """bf16 rounding commutes with powers of two: cotangents x 2^k (k = -40, -13, 17, 40) scale every backward output exactly; other
    points' cotangents change nothing; a point whose cotangents are all zero comes out exactly 0 (the fp32 suite's test on the bf16
    entry points: plain, _params and colour + coarse twins)"""
    check_backwards_point_independent(net, P)


def test_bf16_forwards_are_point_independent(net):
    check_forwards_point_independent(net)


def test_persistent_kernels_past_one_sweep_repeat_the_first_points_bit_for_bit(net):
    """the resident paired forward and fine backward loop over their tiles: a shape past one sweep (and ragged) makes later iterations
    of that loop and the last partial tile run, and its first N points must be the N-point run's bit for bit"""
    P, x, gs, gf, gg = long_inputs(N)
    assert P > persistent_sweep() and P % 32 not in (0, 16)
    long_f, short_f = k_sdf_pair(net, x), k_sdf_pair(net, x[:N].contiguous())
    for k in long_f:
        assert bool(torch.isfinite(long_f[k]).all()), k
        assert torch.equal(long_f[k][:N], short_f[k]), f"sdfnet_forward_pair_bf16: {k} of the first {N} points changes at P = {P}"
    # the tail (later sweeps, last ragged tile) against the one-network kernels of the same tiling, which are not persistent
    tail = x[P - 4001:].contiguous()
    a = k_sdf_pair(net, tail)
    for k in a:
        assert torch.equal(long_f[k][P - 4001:], a[k]), f"sdfnet_forward_pair_bf16: {k} of the last 4001 points depends on the points before"
    for which, tile in (("fine", 16), ("fine", 32), ("coarse", 16)):
        long_b = k_sdf_backward(net, which, tile, x, gs, gf, gg)["x"]
        short_b = k_sdf_backward(net, which, tile, x[:N].contiguous(), gs[:N], gf[:N], gg[:N])["x"]
        assert bool(torch.isfinite(long_b).all())
        assert torch.equal(long_b[:N], short_b), f"sdfnet_backward_bf16 {which} t{tile}: d/dx of the first {N} points changes at P = {P}"
        t = k_sdf_backward(net, which, tile, tail, gs[P - 4001:], gf[P - 4001:], gg[P - 4001:])["x"]
        assert torch.equal(long_b[P - 4001:], t), f"sdfnet_backward_bf16 {which} t{tile}: d/dx of the last 4001 points depends on the points before"


# ------------------------------------------------------------------------------------------------------------------ resident vs staged
def test_resident_and_staged_forms_agree_at_kernel_level(tmp_path, capsys):
    """NSA_BF16_RESIDENT is read once per process: two fresh child processes, each under its own time limit, every exit status checked.
    The paired forward must agree bit for bit; the fine backward is a different kernel function in the two forms (same statements,
    the compiler may contract differently): to the last bits, the allowance tests/test_precision_gpu.py states (1e-6 of the largest)."""
    script = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import mlp_calls; mlp_calls.resident_child(sys.argv[1], %d)" % (
        ROOT, os.path.join(ROOT, "tests"), N)
    res = {}
    for flag in ("1", "0"):
        path = str(tmp_path / f"res{flag}.pt")
        p = subprocess.run([sys.executable, "-c", script, path], capture_output=True, text=True, timeout=180,
                           env=dict(os.environ, NSA_BF16_RESIDENT=flag), cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        res[flag] = torch.load(path)
    assert set(res["1"]) == set(res["0"])
    for k, v in res["1"].items():
        s = res["0"][k]
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
        if k.startswith("pair"):
            assert torch.equal(v, s), f"{k}: resident and staged differ at {int((v != s).sum())} entries"
        else:
            diff = float((v - s).abs().max())
            with capsys.disabled():
                print(f"\n  fine backward, {k}: resident vs staged differ at {int((v != s).any(1).sum())} of {v.shape[0]} points, max {diff:.3e}")
            assert diff <= 1e-6 * float(s.abs().max()), (k, diff)
