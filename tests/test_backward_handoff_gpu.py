"""The two-phase launch nsa_colour_coarse_backward hands the colour phase's results to the coarse SDF phase in registers (feature
cotangent, updated normal cotangent, d/dx to accumulate onto) and the 32-point SDF backward forms the grid slots of its tangent input
in the pass that gathers the rows for the recompute.  Neither may change a bit: the launch is held to nsa_colour_backward followed by
nsa_sdfnet_backward(coarse, accumulate = 1) with torch.equal on every output, at the smallest shapes where the hand-off or the moved
tangent can go wrong -- a single point, a partial tile, exactly one tile, one tile and a point (idle waves, a clamped wave), more
than one workgroup, the tracker's 128 samples per ray -- with g_grad and g_x pre-filled (the hand-off has to reproduce `+=`), the
colour-grid gradient on and off, both stages, and a ray that crosses the SDF grid's boundary (a sample ON the face, samples outside:
features and their tangent are zero there).  The coarse backward of the 32-point tiling is also held to the quad tiling's, and every
call to itself (run-to-run identity)."""
import ctypes

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

# (R, S): P = 1, 31, 32, 33, 100 points; 300 points = 10 tiles = three workgroups; the tracker's path, 128 samples per ray
SHAPES = [(1, 1), (1, 31), (1, 32), (3, 11), (10, 10), (3, 100), (3, 128)]


@pytest.fixture(scope="module")
def model():
    from nicer_slam_amd.model.network import SLAMNetwork
    from nicer_slam_amd.utils.conf import replica_model_conf
    torch.manual_seed(0)
    m = SLAMNetwork(replica_model_conf(use_warp_loss=False), n_images=1,
                    colour_grid=dict(base_resolution=16, desired_resolution=128, log2_hashmap_size=13)).cuda().train()
    for p in m.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        for enc in (m.implicit_network.coarse.encoding, m.implicit_network.fine.encoding, m.rendering_network.encoding):
            enc.embeddings.copy_((torch.rand(enc.embeddings.shape, device="cuda", generator=g) * 2 - 1) * 0.05)
        for n_, p in m.named_parameters():
            if n_.endswith("weight_v"):
                p.add_(0.05 * torch.randn(p.shape, device="cuda", generator=g))
    return m


_CASES = {}


def _case(model, R, S, stage):
    """Forward buffers and cotangents of one shape, computed once and shared (never written by the backward calls)."""
    key = (R, S, stage)
    if key in _CASES:
        return _CASES[key]
    from nicer_slam_amd.fused import render as fr
    g = torch.Generator(device="cuda").manual_seed(100 * R + S)
    P = R * S
    rays_d = torch.nn.functional.normalize(torch.randn(R, 3, device="cuda", generator=g), dim=-1)
    rays_o = ((torch.rand(R, 3, device="cuda", generator=g) - 0.5) * 0.4).contiguous()
    z = torch.rand(R, S, device="cuda", generator=g) * 1.4 + 0.05
    if S >= 8:
        # ray 0 leaves the coarse SDF grid along +z: the sample at depth 0.5 sits ON the face x_z = divide_factor (o_z + 0.5 is exact),
        # the deeper samples are outside, the nearer ones inside
        df = float(model.implicit_network.coarse.divide_factor)
        rays_d[0] = torch.tensor([0.0, 0.0, 1.0], device="cuda")
        rays_o[0] = torch.tensor([0.0625, -0.125, df - 0.5], device="cuda")
        z[0, S // 2] = 0.5
    z = torch.sort(z, dim=1).values.contiguous()
    rays_d = rays_d.contiguous()
    if S >= 8:
        x_z = rays_o[0, 2] + z[0] * rays_d[0, 2]
        assert bool((x_z == df).any()) and bool((x_z > df).any()) and bool((x_z < df).any())
    b = fr.composite_forward_raw(model, rays_o, rays_d, z, stage, True, composite=False)
    cot = dict(g_rgb=torch.randn(P, 3, device="cuda", generator=g), g_sdf=torch.randn(P, device="cuda", generator=g),
               g_grad=torch.randn(P, 3, device="cuda", generator=g), g_x=torch.randn(P, 3, device="cuda", generator=g))
    torch.cuda.synchronize()
    _CASES[key] = (rays_o, rays_d, z, b, cot)
    return _CASES[key]


def _descs(model, tile):
    from nicer_slam_amd.fused import sampler as fs
    net = model.implicit_network.coarse
    gr, keep_r = fs.grid_desc(model.rendering_network.encoding, model.rendering_network.divide_factor, 2, fs.precision_of(model, "colour"))
    gc, keep_c = fs.grid_desc(net.encoding, net.divide_factor, net.num_layers - 2, fs.precision_of(model, "sdf"), tile)
    with torch.no_grad():
        pc = fs.pack.pack_sdf_net4(net) if tile == 16 else fs.pack.pack_sdf_net(net)
    return gr, gc, pc, (keep_r, keep_c)


def _colour(model, case, grid_grad, merged):
    """The data-path backward of the colour network and the coarse SDF network: one launch (merged) or two.  Returns the outputs and,
    for the two-launch form, what the colour backward alone left (the inputs of the coarse backward)."""
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import render as fr
    rays_o, rays_d, z, b, cot = case
    R, S = z.shape
    P = R * S
    pts = fr._pts(rays_o, rays_d, z)
    gr, gc, pc, keep = _descs(model, 32)
    pr = b["packs"][2]
    st = torch.cuda.current_stream().cuda_stream
    g_feat = torch.full((fr.hl_size(P),), float("nan"), device="cuda")
    g_grad, g_x = cot["g_grad"].clone(), cot["g_x"].clone()             # pre-filled: g_grad is added to, g_x overwritten then added to
    g_dir = torch.full((P, 3), float("nan"), device="cuda")
    mid = None
    if merged:
        check(lib.nsa_colour_coarse_backward(ctypes.byref(pts), ctypes.byref(gr), pr.data_ptr(), b["grad"].data_ptr(), b["feat"].data_ptr(),
                                             b["save"].data_ptr(), cot["g_rgb"].data_ptr(), grid_grad, g_feat.data_ptr(), g_grad.data_ptr(),
                                             g_x.data_ptr(), g_dir.data_ptr(), ctypes.byref(gc), pc.data_ptr(), cot["g_sdf"].data_ptr(), st))
    else:
        check(lib.nsa_colour_backward(ctypes.byref(pts), ctypes.byref(gr), pr.data_ptr(), b["grad"].data_ptr(), b["feat"].data_ptr(),
                                      b["save"].data_ptr(), cot["g_rgb"].data_ptr(), grid_grad, g_feat.data_ptr(), g_grad.data_ptr(),
                                      g_x.data_ptr(), g_dir.data_ptr(), st))
        mid = dict(g_feat=g_feat.clone(), g_grad=g_grad.clone(), g_x=g_x.clone())
        check(lib.nsa_sdfnet_backward(ctypes.byref(pts), ctypes.byref(gc), pc.data_ptr(), cot["g_sdf"].data_ptr(), g_feat.data_ptr(),
                                      g_grad.data_ptr(), 1, g_x.data_ptr(), st))
    torch.cuda.synchronize()
    return dict(g_x=g_x, g_dir=g_dir, g_grad=g_grad, g_feat=g_feat), mid


def _same(a, b, P, what):
    from nicer_slam_amd.fused import render as fr
    live = fr.hl_index(P, "cuda")        # (the columns of the last tile's dead lanes derive from never-written forward features)
    for name in a:
        x, y = a[name], b[name]
        if name == "g_feat":
            x, y = x[live], y[live]
        assert bool(torch.isfinite(x).all()), f"{what}: {name} not finite"
        assert torch.equal(x, y), f"{what}: {name}: {int((x != y).sum())} of {x.numel()} differ, max {float((x - y).abs().max()):.3g}"


@pytest.mark.parametrize("grid_grad", [1, 0])
@pytest.mark.parametrize("stage", ["fine", "coarse"])
@pytest.mark.parametrize("R,S", SHAPES)
def test_one_launch_equals_two_launches_bit_for_bit(model, R, S, stage, grid_grad):
    case = _case(model, R, S, stage)
    P = R * S
    two, mid = _colour(model, case, grid_grad, merged=False)
    one, _ = _colour(model, case, grid_grad, merged=True)
    again, _ = _colour(model, case, grid_grad, merged=True)
    assert float(two["g_x"].abs().max()) > 0
    # the pre-filled values took part: g_grad is the colour phase's `+=` onto them, g_x was overwritten (not added to) by it
    assert not torch.equal(mid["g_grad"], case[4]["g_grad"]) and not torch.equal(mid["g_x"], case[4]["g_x"])
    assert torch.equal(two["g_grad"], mid["g_grad"])                # the coarse backward only reads the normal cotangent
    _same(one, two, P, "one launch vs two")
    _same(again, one, P, "one launch, run twice")


@pytest.mark.parametrize("R,S", SHAPES)
def test_coarse_backward_of_both_tilings_agrees_and_repeats(model, R, S):
    """nsa_sdfnet_backward of the coarse network, 32-point tiling against quad tiling, from the cotangents the colour backward leaves
    (accumulate = 1 onto its d/dx): the tolerance tests/test_tiling_gpu.py holds the two tilings' data-path gradient to."""
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import render as fr
    case = _case(model, R, S, "fine")
    rays_o, rays_d, z, b, cot = case
    _, mid = _colour(model, case, 1, merged=False)
    pts = fr._pts(rays_o, rays_d, z)
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for tile, tag in ((32, "a"), (32, "b"), (16, "quad")):
        gr, gc, pc, keep = _descs(model, tile)
        g_x = mid["g_x"].clone()
        check(lib.nsa_sdfnet_backward(ctypes.byref(pts), ctypes.byref(gc), pc.data_ptr(), cot["g_sdf"].data_ptr(), mid["g_feat"].data_ptr(),
                                      mid["g_grad"].data_ptr(), 1, g_x.data_ptr(), st))
        torch.cuda.synchronize()
        out[tag] = g_x
    assert bool(torch.isfinite(out["a"]).all()) and not torch.equal(out["a"], mid["g_x"])
    assert torch.equal(out["a"], out["b"]), "32-point coarse backward: two runs differ"
    ref = out["quad"]
    print(f"P={R * S}: max |g_x32 - g_x16| = {float((out['a'] - ref).abs().max()):.3g}, max |g_x| = {float(ref.abs().max()):.3g}")
    assert_close(out["a"], ref.cpu().numpy(), 1e-7 + 1e-4 * float(ref.abs().max()), 1e-4, "g_x, 32-point vs quad")
