"""Pin tests/grid_ref64.py (the grid encoder in dtype-generic torch) without a GPU:
  * its fp32 mode against the C oracle -- level geometry and row map equal, value and Jacobian bit for bit (the restatement keeps the
    oracle's statement order and torch's element-wise CPU kernels round every operation on its own), J^T g and J q bit for bit as
    well, the two table scatters at 1e-6 of the row's summed contributions (same (point, corner) order; index_add_ may reassociate);
  * its float64 mode against the committed goldens (the reference's wrappers and its pure-torch twin) at the tolerances
    tests/test_hashenc_gpu.py and tests/test_oracle_golden.py hold fp32 implementations to against the same files;
  * the path counters of tests/test_grid_float64_gpu.py on that file's inputs: every count non-zero where the geometry has the
    path at all, so an input change that empties a path fails here."""
import numpy as np
import pytest
import torch

import grid_ref64 as G
from helpers import load, tt, assert_close
from mlp_calls import perturbed
from oracle import hashenc
from oracle import render_ref as R

GEOMS, TINY, _spec = G.GEOMS, G.TINY, G.spec_of


@pytest.mark.parametrize("name", list(GEOMS) + list(TINY))
def test_level_geometry_and_rows_equal_the_oracle(name):
    spec = _spec(name)
    S = float(np.log2(spec.per_level_scale))
    rng = np.random.default_rng(3)
    for l, lv in enumerate(G.levels(spec)):
        row0, rows, res, scale = hashenc.level_geometry(spec.offsets.numpy(), l, S, spec.base_resolution)
        assert (lv.row0, lv.rows, lv.res) == (row0, rows, res) and float(lv.scale) == scale, (l, lv)
        q = np.concatenate([rng.integers(0, res + 1, (200, 3)), [[res, res, res], [0, 0, 0], [res - 1, res, 0]]]).astype(np.uint32)
        assert G.level_row(lv, q, 3).tolist() == [hashenc.level_row(rows, res, c) for c in q]


@pytest.mark.parametrize("name", list(GEOMS))
def test_fp32_mode_equals_the_c_oracle(name):
    spec = _spec(name)
    B = 4123
    u, emb = G.points(B, spec), G.table(spec)
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(B, spec.num_levels, spec.level_dim, generator=gen)
    q = torch.randn(B, 3, generator=gen)
    o = G.oracle_suite(spec, emb, u, g, q)
    plan = G.Plan(u, spec)
    y, J = G.encode(plan, u, emb)
    gu, gt, n1 = G.backward(plan, u, g, J, with_norms=True)
    gg, g2, n2 = G.second_backward(plan, u, g, J, q, with_norms=True)
    for k, got in (("y", y), ("J", J), ("gu", gu), ("gg", gg)):
        assert torch.equal(got, o[k]), f"{k}: {int((got != o[k]).sum())} of {got.numel()} elements differ"
    for k, got, n in (("gt", gt, n1), ("g2", g2, n2)):
        err = (got.double() - o[k].double()).norm(dim=1)
        assert bool((err <= 1e-6 * n[0]).all()), f"{k}: worst {float((err / n[0].clamp_min(1e-300)).max()):.3g} of the row's contributions"
        assert bool((got[n[1] == 0] == 0).all())
    out = ~plan.inside
    assert int(out.sum()) > 0 and float(y[out].abs().max()) == 0 and float(J[out].abs().max()) == 0


@pytest.mark.parametrize("name", ["coarse", "fine"])
def test_autograd_pair_equals_the_oracle_pair(name):
    """the Function pair in fp32 against oracle/render_ref.py::_Encode under the same double backward"""
    spec = _spec(name)
    B = 700
    gen = torch.Generator().manual_seed(6)
    v, q, r = torch.randn(B, spec.out_dim, generator=gen), torch.randn(B, 3, generator=gen), torch.randn(B, spec.out_dim, generator=gen)
    res = []
    for mine in (True, False):
        emb, u, vv = G.table(spec).requires_grad_(True), G.points(B, spec).requires_grad_(True), v.clone().requires_grad_(True)
        y = G.grid_features(u, emb, spec) if mine else R._Encode.apply(u, emb, spec.offsets, spec.per_level_scale, spec.base_resolution, True)
        (gx,) = torch.autograd.grad(y, u, vv, create_graph=True)
        ((gx * q).sum() + (y * r).sum()).backward()
        res.append((y.detach(), gx.detach(), vv.grad, emb.grad, u.grad))
    for k, a, b in zip(("y", "gx", "v.grad", "emb.grad", "u.grad"), *res):
        if k == "emb.grad":
            assert_close(a, b, 1e-6 * float(b.abs().max()), 1e-5, k)
        else:
            assert torch.equal(a, b), k


def _golden_suite(fx, dtype):
    L, C, base, end, logmap = [int(t) for t in fx["meta_grid"]]
    spec = R.make_grid_spec(L, C, base, end, logmap)
    assert spec.offsets.tolist() == fx["param_offsets"].tolist()
    x = tt(fx["in_x"])
    u32 = (x + 1.0) / 2.0
    xd = x.to(dtype).requires_grad_(True)
    emb = tt(fx["param_embeddings"]).to(dtype).requires_grad_(True)
    v = tt(fx["in_v"]).to(dtype).requires_grad_(True)
    y = G.grid_features((xd + 1.0) / 2.0, emb, spec, u32=u32)
    (gx,) = torch.autograd.grad(y, xd, v, create_graph=True)
    (first,) = torch.autograd.grad(y, emb, v, retain_graph=True)
    return spec, xd, emb, v, y, gx, first


@pytest.mark.parametrize("name", ["enc_coarse", "enc_fine", "enc_colour"])
def test_float64_mode_against_the_wrapper_goldens(name):
    fx = load(name)
    _spec_, x, emb, v, y, gx, first = _golden_suite(fx, G.F64)
    ((gx * tt(fx["in_q"]).double()).sum() + (y * tt(fx["in_r"]).double()).sum()).backward()
    assert_close(y, fx["out_y"], 1e-5, 1e-4, "y")
    assert_close(gx, fx["out_gx"], 2e-5 * float(np.abs(fx["out_gx"]).max()), 1e-4, "J^T v")
    assert_close(v.grad, fx["out_v_grad"], 2e-5 * float(np.abs(fx["out_v_grad"]).max()), 1e-4, "d/dv (J q)")
    for got, key in ((first, "out_first_emb"), (emb.grad, "out_emb_grad")):
        assert_close(got, fx[key], 1e-4 * float(np.abs(fx[key]).max()), 1e-3, key)
    assert_close(x.grad, fx["out_x_grad"], 2e-5 * float(np.abs(fx["out_x_grad"]).max()), 1e-4, "x.grad")
    assert float(y[3].abs().max()) == 0 and float(y[4].abs().max()) == 0


@pytest.mark.parametrize("name", ["twin_dense", "twin_dense_c8", "twin_dense_c2"])
def test_float64_mode_against_the_torch_twin_goldens(name):
    from test_oracle_golden import twin_checks
    fx = load(name)
    _spec_, _x, emb, v, y, gx, first = _golden_suite(fx, G.F64)
    v2, e2 = torch.autograd.grad((gx * tt(fx["in_q"]).double()).sum(), [v, emb])
    assert_close(y, fx["out_y"], 5e-5, 1e-4, "y vs torch_forward")
    assert_close(gx, fx["out_gx"], 5e-5 * float(np.abs(fx["out_gx"]).max()), 1e-4, "J^T v vs autograd(torch_forward)")
    twin_checks(fx, first, v2, e2)


def test_float64_cell_border_is_continuous():
    """points on an interior cell border: float64 from the cell fp32 chose and from its lower neighbour agree to rounding"""
    spec = _spec("fine")
    lv = G.levels(spec)[3]
    m = 17
    c = np.float32(m) / lv.scale
    cands = [x for x in (c, np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-1))) if np.float32(x) * lv.scale == np.float32(m)]
    assert cands
    u = torch.tensor([[float(cands[0]), 0.3, 0.7]])
    emb = G.table(spec).double()
    plan = G.Plan(u, spec)
    assert int(plan.cell[3][0, 0]) == m
    y0, J0 = G.encode(plan, u.double(), emb)
    plan.cell[3][0, 0] = m - 1                                   # the neighbour cell: t = 1 + O(ulp) there
    q = plan.cell[3].numpy().astype(np.uint32)
    for corner in range(8):
        bits = np.array([(corner >> d) & 1 for d in range(3)], np.uint32)
        plan.rows[3][:, corner] = torch.from_numpy(G.level_row(lv, q + bits[None], 3).astype(np.int64) + lv.row0)
    y1, J1 = G.encode(plan, u.double(), emb)
    scale = float(emb[plan.rows[3][0]].abs().max())
    assert float((y0 - y1).abs().max()) <= 1e-12 * scale
    assert float((J0 - J1).abs().max()) <= 1e-5 * scale * float(lv.scale)      # dw = 6 t (1 - t) with |t - 1| <= 2^-24 scale


PATHS_ALWAYS = ("up", "run_pairs", "full_wave_runs", "equal_across_wave", "equal_across_block", "equal_across_invalid")


@pytest.mark.parametrize("name", ["coarse", "fine", "colour_small"] + list(TINY))
def test_every_scatter_path_is_walked_by_the_gpu_inputs(name):
    spec = _spec(name)
    n = G.paths(G.Plan(G.points(4123, spec), spec))
    print(name, n)
    for k in PATHS_ALWAYS:
        assert n[k] > 0, (k, n)
    lv = G.levels(spec)
    if any(v.hashed for v in lv):
        assert n["down"] > 0, n
        if any(v.hashed and v.rows > 2 for v in lv):      # with two rows x and x + 1 always land on the two of them: no single path
            assert n["single_hashed_odd_x"] > 0, n
    if any(not v.hashed for v in lv):
        assert n["single_dense_wrap"] > 0, n
    if any(not v.hashed and v.rows & (v.rows - 1) for v in lv):
        assert n["face_dense_nonpow2"] > 0, n
    if name in TINY:        # an up lane next to a down lane with the same base needs two cells whose hashes differ in bit 0 only: a collision
        assert n["corners_collide"] > 0 and n["up_next_to_down"] > 0, n


def _listening_model(seed=0):
    """the golden model with every weight_v perturbed, as tests/mlp_calls.py::Net does: its networks then listen to their
    grid features (the golden's own first-layer grid columns are zero)"""
    _fx, cfg, params = perturbed(seed=seed)
    return params, cfg


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_ref64_exact_grid_in_fp32_equals_the_oracle_renderer(which):
    """tests/ref64.py with grid="exact" in fp32 mode against oracle/render_ref.py: sdf, grad sdf, feature, d/dx and the table gradient
    (value path + the double backward's share).  The grid part is the oracle's bit for bit; the MLP part is the same torch graph."""
    import ref64
    params, cfg = _listening_model()
    gen = torch.Generator().manual_seed(12)
    P = 600
    x = (torch.rand(P, 3, generator=gen) * 2 - 1) * 0.999
    x[:4] = torch.tensor([[1.0, 0.2, -0.3], [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.1, 1.25, 0.0]])
    gs, gf, gg = torch.randn(P, generator=gen), torch.randn(P, 64, generator=gen), torch.randn(P, 3, generator=gen)
    key = ref64.NETS[which] + ".encoding.embeddings"
    prm = dict(params)
    prm[key] = params[key].clone().requires_grad_(True)
    xs = x.clone().requires_grad_(True)
    so, fo, go = R._net_outputs(prm, ref64.NETS[which], getattr(cfg, which), xs)
    ox, ot = torch.autograd.grad((gs * so[:, 0]).sum() + (gf * fo).sum() + (gg * go).sum(), (xs, prm[key]))
    assert float(ot.abs().max()) > 1e-3 and float(fo.abs().max()) > 1e-3
    sdf, grad, feat = ref64.sdf_forward(params, cfg, x, (which,), dtype=torch.float32, grid="exact")
    assert torch.equal(sdf, so[:, 0].detach()) and torch.equal(grad, go.detach()) and torch.equal(feat, fo.detach())
    gx, gt, plan = ref64.sdf_table_grad(params, cfg, x, which, gs, gf, gg, dtype=torch.float32)
    assert torch.equal(gx, ox)
    assert_close(gt, ot, 1e-6 * float(ot.abs().max()), 1e-5, "table gradient")
    assert [r[0] for r in plan.record] == ["first", "second", "first"]
    assert torch.equal(ref64.sdf_backward(params, cfg, x, gs, gf, gg, (which,), dtype=torch.float32, grid="exact"), ox)


def test_ref64_exact_colour_grid_in_fp32_equals_the_oracle_renderer():
    import ref64
    params, cfg = _listening_model()
    gen = torch.Generator().manual_seed(13)
    P = 400
    x = (torch.rand(P, 3, generator=gen) * 2 - 1) * 0.999
    n, d, f = torch.randn(P, 3, generator=gen), torch.randn(P, 3, generator=gen), torch.randn(P, 64, generator=gen)
    g_rgb = torch.randn(P, 3, generator=gen)
    key = "rendering_network.encoding.embeddings"
    prm = dict(params)
    prm[key] = params[key].clone().requires_grad_(True)
    ins = [t.clone().requires_grad_(True) for t in (x, n, d, f)]
    rgb = R.colour_net(prm, cfg, *ins, color_stage="highfreq")
    want = torch.autograd.grad((g_rgb * rgb).sum(), ins + [prm[key]])
    got, gt, _plan = ref64.colour_table_grad(params, cfg, x, n, d, f, g_rgb, dtype=torch.float32)
    assert float(want[4].abs().max()) > 1e-4
    for k, w in zip(("x", "normals", "dirs", "feat"), want):
        assert torch.equal(got[k], w), k
    assert_close(gt, want[4], 1e-6 * float(want[4].abs().max()), 1e-5, "colour table gradient")


@pytest.mark.parametrize("name", ["coarse", "fine", "tiny3_c2"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257])
def test_small_batches_carry_the_families_and_the_boundaries(B, name):
    """the batch sizes on both sides of the wave (64) and block (256) boundaries: what each of them walks"""
    spec = _spec(name)
    plan = G.Plan(G.points(B, spec), spec)
    n = G.paths(plan)
    lv = G.levels(spec)
    hashed = any(v.hashed for v in lv)
    if B == 1:
        assert bool(plan.inside.all()) and n["up"] + n["down"] + n["single_hashed_odd_x"] + n["single_dense_wrap"] == 4 * len(lv), n
        return
    assert int((~plan.inside).sum()) == 1 and int(plan.face1.sum()) == 1
    assert n["up"] > 0 and n["run_pairs"] > 0 and n["equal_across_invalid"] > 0 and (n["down"] > 0 or not hashed), n
    if B >= 65:
        assert n["equal_across_wave"] > 0, n          # copies on both sides of lane 63 | 64
    if B >= 255:
        assert n["full_wave_runs"] > 0, n
        if name == "fine":
            assert n["single_hashed_odd_x"] > 0 and n["face_dense_nonpow2"] > 0, n
        if name == "tiny3_c2":
            assert n["corners_collide"] > 0 and n["single_hashed_odd_x"] > 0, n
    if B == 257:
        assert n["equal_across_block"] > 0, n         # consecutive ray samples on both sides of point 255 | 256
