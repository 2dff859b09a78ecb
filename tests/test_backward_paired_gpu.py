"""The data-path SDF backward of the quad tiling against its _params twin, bit for bit.

nsa_sdfnet_backward (tile 16, fp32 operands) stages each weight block once and multiplies it with two operands: the forward beside the
tangent sweep, the reverse pass beside the reverse sweep (csrc/render_sdfnet4.hip::SdfOps4Data, csrc/mlp16.hpp::gemm16_staged2).
nsa_sdfnet_backward_params keeps the one-operand sequence of 4 NH + 1 GEMMs.  Both form the same products in the same order per
accumulator with the same per-point scales and hints, so their d/dx must be EQUAL (torch.equal), for the coarse (NH = 1) and the fine
(NH = 3) network, and every call must be equal to itself when repeated.

Shapes: the smallest that can go wrong with 8 waves x 16 points per workgroup -- one point, a partial tile, a full tile, idle (clamped)
waves, a full workgroup, a second workgroup, a ragged third -- and 3 rays x 128 samples through the ray form of the point source.
Operands: each paired-scale path -- every cotangent alone, all three, each one passed as NULL, g_grad exactly zero on every other
point (the tangent operand of a pair then takes the all-zero rule of point_scale_of beside a live forward operand), cotangent scales
alternating between 2^-60 and 2^40 from point to point, accumulate 0 / 1 into a pre-filled g_x, and a ray that leaves the grid
(a sample exactly on the face, the rest outside: Jacobian and tangent input exactly zero)."""
import ctypes

import pytest
import torch

from devcall import ptr, st
from gemm_cases import cot, cube_points, scaled
from mlp_calls import Net, to_hl

pytestmark = pytest.mark.gpu

SHAPES = (1, 15, 16, 17, 127, 128, 129, 300)
P_CASES = 300           # two full workgroups and a third with two full tiles, a 12-point tile and five clamped waves


@pytest.fixture(scope="module")
def net():
    return Net()


def backward(net, which, points, P, gs, gf, gg, accumulate=0, init=None, params=False):
    """d/dx [P, 3] of one launch; points: explicit [P, 3] tensor or (o [R, 3], d [R, 3], z [R, S])"""
    from nicer_slam_amd._native import PointsDesc, check, lib
    from nicer_slam_amd.fused import mapping
    gd, _keep, pk = net.sdf(which, 16)
    if isinstance(points, tuple):
        o, d, z = (t.cuda().contiguous() for t in points)
        pts = PointsDesc(o.data_ptr(), d.data_ptr(), z.data_ptr(), None, P, z.shape[1], None)
    else:
        xd = points.cuda().contiguous()
        pts = PointsDesc(None, None, None, xd.data_ptr(), P, 0, None)
    gs = gs.cuda().contiguous() if gs is not None else None
    gf = to_hl(gf) if gf is not None else None
    gg = gg.cuda().contiguous() if gg is not None else None
    g_x = torch.zeros(P, 3, device="cuda") if init is None else init.cuda().clone()
    if params:
        rows = lib.nsa_sdfnet_emit_rows_tile(gd.n_hidden, 16)
        assert rows > 0
        emit = torch.empty((rows, mapping.emit_ld(P)), device="cuda")
        check(lib.nsa_sdfnet_backward_params(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), ptr(gs), ptr(gf), ptr(gg), accumulate,
                                             g_x.data_ptr(), None, emit.data_ptr(), emit.shape[1], st()))
    else:
        check(lib.nsa_sdfnet_backward(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), ptr(gs), ptr(gf), ptr(gg), accumulate,
                                      g_x.data_ptr(), st()))
    torch.cuda.synchronize()
    return g_x.cpu()


def hold(net, which, what, points, P, gs, gf, gg, accumulate=0, init=None):
    runs = [backward(net, which, points, P, gs, gf, gg, accumulate, init) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r, runs[0]), f"{which} {what}: nsa_sdfnet_backward differs from itself between two calls"
    twin = backward(net, which, points, P, gs, gf, gg, accumulate, init, params=True)
    assert bool(torch.isfinite(twin).all()), f"{which} {what}: the twin's d/dx is not finite"
    diff = runs[0] != twin
    assert not bool(diff.any()), (f"{which} {what}: d/dx differs from nsa_sdfnet_backward_params' at {int(diff.any(1).sum())} of {P} "
                                  f"points, first at point {int(diff.any(1).nonzero()[0])}")
    return runs[0]


def base(P):
    return cot(P, 80, ()), cot(P, 81, (64,)), cot(P, 82, (3,))


@pytest.mark.parametrize("which", ["coarse", "fine"])
@pytest.mark.parametrize("P", SHAPES)
def test_shapes(net, which, P):
    gs, gf, gg = base(P)
    out = hold(net, which, f"P = {P}", cube_points(P, 83), P, gs, gf, gg)
    assert bool((out != 0).any())


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_tracker_shape_three_rays_of_128_samples(net, which):
    g = torch.Generator().manual_seed(84)
    o = (torch.rand(3, 3, generator=g) * 2 - 1) * 0.3
    d = torch.nn.functional.normalize(torch.randn(3, 3, generator=g), dim=-1)
    z = torch.sort(torch.rand(3, 128, generator=g) * 0.6, dim=1).values
    gs, gf, gg = base(384)
    hold(net, which, "3 x 128 samples", (o, d, z), 384, gs, gf, gg)


def operand_cases(P):
    gs, gf, gg = base(P)
    odd = torch.arange(P) % 2 == 1
    cases = {"all three": (gs, gf, gg), "g_sdf alone": (gs, None, None), "g_feat alone": (None, gf, None), "g_grad alone": (None, None, gg),
             "g_sdf NULL": (None, gf, gg), "g_feat NULL": (gs, None, gg), "g_grad NULL": (gs, gf, None)}
    zg = gg.clone()
    zg[odd] = 0.0
    cases["g_grad zero on every other point"] = (gs, gf, zg)
    cases["g_grad alone, zero on every other point"] = (None, None, zg)
    c = torch.where(odd, 2.0 ** 40, 2.0 ** -60).double()
    cases["scales alternating 2^-60 / 2^40"] = tuple(scaled(b, c) for b in (gs, gf, gg))
    return cases


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_operand_cases(net, which):
    x = cube_points(P_CASES, 85)
    for name, (gs, gf, gg) in operand_cases(P_CASES).items():
        hold(net, which, name, x, P_CASES, gs, gf, gg)


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_accumulate_into_a_prefilled_g_x(net, which):
    x = cube_points(P_CASES, 86)
    gs, gf, gg = base(P_CASES)
    init = cot(P_CASES, 87, (3,))
    over = hold(net, which, "accumulate 0, g_x pre-filled", x, P_CASES, gs, gf, gg, 0, init)
    added = hold(net, which, "accumulate 1, g_x pre-filled", x, P_CASES, gs, gf, gg, 1, init)
    assert torch.equal(over, hold(net, which, "accumulate 0", x, P_CASES, gs, gf, gg)), f"{which}: accumulate 0 reads g_x"
    assert torch.equal(added, over + init), f"{which}: accumulate 1 is not g_x + d/dx"       # (one fp32 addition per value, as the kernel's)


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_a_ray_leaving_the_grid(net, which):
    gd, _keep, _pk = net.sdf(which, 16)
    edge = float(gd.divide_factor)                     # the grid covers [-edge, edge]^3
    S = 128
    o = torch.tensor([[0.0, 0.1 * edge, -0.2 * edge], [0.05 * edge, 0.0, 0.3 * edge]])
    d = torch.tensor([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    z = torch.empty(2, S)
    z[0] = torch.cat([torch.linspace(0.5, 0.99, 40) * edge, torch.tensor([edge]), torch.linspace(1.001, 1.6, S - 41) * edge])
    z[1] = torch.linspace(0.0, 0.9, S) * edge          # a ray that stays inside, in the same tiles' neighbourhood
    assert float(o[0, 0] + z[0, 40] * d[0, 0]) == edge
    gs, gf, gg = base(2 * S)
    out = hold(net, which, "ray leaving the grid", (o, d, z), 2 * S, gs, gf, gg)
    assert bool(torch.isfinite(out).all())
    hold(net, which, "ray leaving the grid, g_grad alone", (o, d, z), 2 * S, None, None, gg)
