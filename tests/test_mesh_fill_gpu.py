"""Hole filling on the device (header Section 23, csrc/mesh_fill.hip) against the numpy statement of tests/fill_ref.py:
every array of the report and every total element for element, the loops' float64 rows and the fp32 positions and colours BIT FOR
BIT -- the statement is + - * / on float64 in a stated order, so no tolerance takes part -- and a second run byte-identical.  Then
the public interface, the normals, the other tools on the result, the extract_mesh keywords, a PLY round trip and the command line."""
import json

import numpy as np
import pytest
import torch

import clean_ref
import fill_ref as R
import simplify_ref
import smooth_ref as S
import topology_ref as T

pytestmark = pytest.mark.gpu

ITEM_KEYS = (("halfedges", "halfedges"), ("next", "next"), ("item_leader", "leader"), ("rank", "rank"))


def _check(mesh, **kw):
    """the device against the oracle, twice; returns (device result, device report, oracle result)"""
    from nicer_slam_amd import mesh_fill as M
    got, rep = M.fill_holes(mesh, normals="none", return_report=True, **kw)
    again, rep2 = M.fill_holes(mesh, normals="none", return_report=True, **kw)
    ref = R.fill_holes(mesh, **kw)
    tr = ref["trace"]
    print(f"V {len(mesh['verts'])} F {len(mesh['faces'])} -> {rep['totals']}")
    for k in ("verts", "faces", "colors"):
        assert (k in got) == (k in ref)
        if k in ref:
            assert got[k].tobytes() == again[k].tobytes(), k
    for k in ("halfedges", "next", "flags", "item_leader", "rank", "order", "ints", "reals", "new_vertex"):
        assert rep[k].tobytes() == rep2[k].tobytes(), k
    assert rep["totals"] == rep2["totals"] == ref["totals"]
    for k, name in ITEM_KEYS:
        assert rep[k].dtype == np.int32 and rep[k].tolist() == tr[name].tolist(), k
    assert rep["flags"].tolist() == (tr["blocked"] * 1 + tr["pinch"] * 2 + tr["open_chain"] * 4).tolist()
    assert rep["order"].tolist() == tr["order"].tolist()
    assert rep["ints"].shape == ref["ints"].shape and (rep["ints"] == ref["ints"]).all()
    assert rep["class"] == [R.CLASSES[c] for c in ref["ints"][:, 3]] and rep["n"] == ref["ints"][:, 1].tolist()
    assert rep["reals"].shape == ref["reals"].shape and (rep["reals"].view(np.uint64) == ref["reals"].view(np.uint64)).all()
    assert np.array_equal(rep["new_vertex"], ref["new_vertex"])
    assert got["faces"].dtype == np.int32 and got["faces"].shape == ref["faces"].shape and (got["faces"] == ref["faces"]).all()
    for k in ("verts", "colors"):
        if k in ref:
            assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape
            diff = (got[k].view(np.uint32) != ref[k].view(np.uint32)).any(1)
            assert not diff.any(), (k, int(diff.sum()), np.nonzero(diff)[0][:5], got[k][diff][:3], ref[k][diff][:3])
    return got, rep, ref


@pytest.fixture(scope="module")
def cases():
    return R.table_cases()


def _mesh(v, f):
    return dict(verts=np.ascontiguousarray(v, np.float32), faces=np.ascontiguousarray(f, np.int32).reshape(-1, 3))


# ---- the rows of DESIGN 4v ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.table_cases()))
def test_table_rows(cases, name):
    mesh, kw = cases[name]
    _check(mesh, **kw)


def test_nothing_to_fill():
    from nicer_slam_amd import mesh_fill as M
    for V in (0, 5):
        mesh = _mesh(np.arange(3 * V).reshape(V, 3), np.zeros((0, 3)))
        got, rep, _ = _check(mesh)
        assert got["verts"].shape == (V, 3) and got["faces"].shape == (0, 3) and rep["totals"]["n_boundary"] == 0
    closed = _mesh(simplify_ref.TET_V, simplify_ref.TET_F)
    got, rep, _ = _check(closed)
    assert got["verts"].tobytes() == closed["verts"].tobytes() and rep["totals"] == dict.fromkeys(M.TOTALS, 0)
    one = _mesh(simplify_ref.TET_V, simplify_ref.TET_F[:1])                               # one face: a loop of three, closed by three faces
    got, rep, _ = _check(one)
    assert rep["n"] == [3] and rep["class"] == ["filled"] and got["faces"].shape == (4, 3)


def test_high_indices():
    f, V = T.high_index_faces(2 ** 16 + 3)
    got, rep, _ = _check(_mesh(S.index_only_mesh(f, V), f[:3]))
    assert rep["n"] == [3] and got["faces"][3:].max() == V and got["verts"].shape == (V + 1, 3)


@pytest.mark.parametrize("skip_folded", [True, False])
def test_a_loop_over_several_blocks(skip_folded):
    f, V = T.strip(5000)
    got, rep, _ = _check(R.with_colors(_mesh(S.index_only_mesh(f, V), f)), skip_folded=skip_folded)
    assert rep["n"] == [5002] and rep["class"] == ["folded" if skip_folded else "filled"] and R.n_rounds(5002) == 14
    assert rep["rank"].max() == 5001 and len(got["faces"]) == (5000 if skip_folded else 5000 + 5002 * (2 * rep["rings"][0] - 1))


@pytest.mark.parametrize("method", ["polar", "min_area"])
def test_a_scan_over_more_blocks_than_the_offsets_workgroup_has_lanes(method):
    """a flat 128 x 128 quad sheet (topology_ref.quad_sheet) without the quads (4 a + 1, 4 b + 1), a, b < 32: 3 F = 92 160 half-edges are
    360 scan blocks of 256 for the 256 lanes of the one workgroup that scans the block sums (csrc/block_scan.hpp), so a lane owns two
    blocks.  In closed form: 1024 loops of four edges and the outer loop of 512, which max_edges leaves open; a polar patch of a
    square is four faces about a new vertex, a minimum-area patch two faces and no vertex, and either gives back a sheet with
    the edges of the full one and one boundary loop"""
    from nicer_slam_amd import mesh_fill as M, mesh_topology
    a = 128
    f, V = T.quad_sheet(a, a)
    quad = torch.arange(a * a, device="cuda")
    hole = ((quad // a) % 4 == 1) & ((quad % a) % 4 == 1)
    f = f.reshape(a * a, 2, 3)[~hole].reshape(-1, 3).contiguous()
    k, F = int(hole.sum()), f.shape[0]
    assert k == 1024 and 3 * F == 92160 > 256 * 256
    i = torch.arange(V, device="cuda")
    v = torch.stack([i // (a + 1), i % (a + 1), torch.zeros_like(i)], 1).float()
    got, rep = M.fill_holes(dict(verts=v, faces=f), max_edges=4, method=method, return_report=True)
    assert sorted(rep["n"]) == [4] * k + [4 * a] and rep["totals"]["n_too_many_edges"] == 1 and rep["totals"]["n_filled"] == k
    per_hole = 4 if method == "polar" else 2
    assert torch.equal(got["faces"][:F], f) and got["faces"].shape[0] == F + per_hole * k
    assert got["verts"].shape[0] == V + (k if method == "polar" else 0)
    if method == "min_area":
        assert rep["area_class"].count("area_filled") == k and rep["area_totals"]["n_area_filled"] == k
    t = mesh_topology.edge_table(got["faces"], got["verts"].shape[0])
    E = 3 * a * a + 2 * a + (3 * k if method == "polar" else 0)          # a polar patch: four spokes for one diagonal
    assert [t[key] for key in ("n_edges", "n_boundary", "n_nonmanifold", "n_inconsistent", "n_boundary_loops")] == [E, 4 * a, 0, 0, 1]


def _grid65(both_diagonals):
    cells = [(4 * a + 1, 4 * b + 1) for a in range(16) for b in range(16)]
    if both_diagonals:
        cells += [(4 * a + 2, 4 * b + 2) for a in range(16) for b in range(16)]
    return _mesh(*R.grid_without(65, cells))


def test_many_small_loops():
    got, rep, _ = _check(_grid65(False), max_edges=4)
    assert sorted(rep["n"]) == [4] * 256 + [256] and rep["totals"]["n_filled"] == 256 and rep["totals"]["n_too_many_edges"] == 1
    assert rep["totals"]["n_pinched"] == 0 and len(got["faces"]) == 2 * (64 * 64 - 256) + 4 * 256
    top = T.topology(got["faces"], len(got["verts"]))
    assert top["n_boundary"] == 256 and top["n_boundary_loops"] == 1 and top["euler"] == 1


def test_many_pinched_loops():
    mesh = _grid65(True)
    got, rep, _ = _check(mesh, max_edges=8)
    assert sorted(rep["n"]) == [8] * 256 + [256] and rep["totals"]["n_pinched"] == 256 and rep["totals"]["n_filled"] == 0
    assert got["faces"].tobytes() == mesh["faces"].tobytes() and got["verts"].tobytes() == mesh["verts"].tobytes()


def test_adversarial_lists_and_non_finite_vertices():
    for name, (f, V) in clean_ref.adversarial_cases(2000).items():
        mesh = R.with_colors(_mesh(simplify_ref.adversarial_mesh(f, V), f))
        for kw in (dict(skip_folded=False), dict(max_edges=6, max_size=1.0, rings=2)):
            _check(mesh, **kw)


# ---- the public interface -------------------------------------------------------------------------------------------------------------

def test_kinds_in_and_out(cases):
    from nicer_slam_amd import mesh_fill as M
    mesh = cases["grid with a hole"][0]
    ref = M.fill_holes(mesh)
    assert all(isinstance(ref[k], np.ndarray) for k in ("verts", "faces", "colors"))
    for dev in ("cpu", "cuda"):
        out = M.fill_holes({k: torch.from_numpy(x).to(dev) for k, x in mesh.items()})
        for k in ("verts", "faces", "colors"):
            assert torch.is_tensor(out[k]) and out[k].device.type == dev and out[k].cpu().numpy().tobytes() == ref[k].tobytes(), (dev, k)
    loops = M.boundary_loops(dict(verts=mesh["verts"], faces=mesh["faces"]))
    start, verts, tr = R.boundary_loops(mesh["faces"], len(mesh["verts"]))
    assert loops["loop_start"].tolist() == start.tolist() and loops["vertices"].tolist() == verts.tolist()
    assert loops["class"] == ["filled", "filled"] and loops["n_open_chain"] == 0 and loops["halfedges"].tolist() == tr["order"].tolist()


def test_normals(cases):
    from nicer_slam_amd import mesh_fill as M
    mesh = dict(cases["cut sphere"][0])
    V = len(mesh["verts"])
    stored = np.random.default_rng(0).standard_normal((V, 3)).astype(np.float32)
    ref = R.fill_holes(mesh)
    want = S.vertex_normals(ref["verts"], ref["faces"], "angle")
    kept = M.fill_holes(dict(mesh, normals=stored))
    assert kept["normals"].shape == ref["verts"].shape and kept["normals"][:V].tobytes() == stored.tobytes()
    assert np.abs(kept["normals"][V:] - want[V:]).max() <= 2.0 ** -23
    assert "normals" not in M.fill_holes(mesh) and "normals" not in M.fill_holes(dict(mesh, normals=stored), normals="none")
    assert np.abs(M.fill_holes(mesh, normals="angle")["normals"] - want).max() <= 2.0 ** -23
    area = M.fill_holes(dict(mesh, normals=stored), normals="area")["normals"]
    assert area.tobytes() == S.vertex_normals(ref["verts"], ref["faces"], "area").tobytes()


def test_fairing(cases):
    from nicer_slam_amd import mesh_fill as M
    mesh = cases["cut sphere"][0]
    ref = R.fill_holes(mesh)
    want, _ = S.smooth_steps(ref["verts"], ref["faces"], S.factors_of("laplacian", 5, 0.5), fixed=~ref["new_vertex"])
    got = M.fill_holes(mesh, fair=5)
    assert got["verts"].tobytes() == want.tobytes() and got["colors"].tobytes() == ref["colors"].tobytes()


def test_other_tools_take_the_result_and_ply_round_trip(cases, tmp_path):
    from nicer_slam_amd import inference, mesh_fill as M, mesh_sdf, mesh_topology
    mesh = {k: torch.from_numpy(x).cuda() for k, x in cases["cut sphere"][0].items()}
    assert mesh_sdf.resolve_sign(mesh, "auto") == "winding"
    out = M.fill_holes(mesh, normals="angle")
    r = mesh_topology.topology(out)
    assert r["is_watertight"] and r["is_oriented"] and r["euler"] == 2
    assert mesh_sdf.resolve_sign(out, "auto") == "normal"
    path = str(tmp_path / "filled.ply")
    inference.write_ply(path, out)
    back = inference.read_ply(path)
    assert back["verts"].tobytes() == out["verts"].cpu().numpy().tobytes() and np.array_equal(back["faces"], out["faces"].cpu().numpy())


def test_weld(cases):
    """a seam of repeated vertices is no boundary with weld=True: only the real hole is filled"""
    from nicer_slam_amd import mesh_fill as M
    v, f = S.grid_mesh(9, hole=(2, 3, 3))
    left = f[v[f].mean(1)[:, 0] < 4.0]
    right = f[v[f].mean(1)[:, 0] >= 4.0] + len(v)                                        # the right half on a copy of the vertices
    mesh = _mesh(np.concatenate([v, v]), np.concatenate([left, right]))
    _, plain = M.fill_holes(mesh, return_report=True)
    _, welded = M.fill_holes(mesh, weld=True, return_report=True)
    assert plain["totals"]["n_loops"] == 2 and sorted(welded["n"]) == [12, 32] and welded["totals"]["n_filled"] == 2
    assert sorted(welded["n"]) != sorted(plain["n"])


def test_command_line(cases, tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_fill as M
    mesh = cases["grid with a hole"][0]
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    full = dict(mesh, normals=S.vertex_normals(mesh["verts"], mesh["faces"], "area"))
    inference.write_ply(src, {k: torch.from_numpy(x) for k, x in full.items()})
    t = M.main([src, "--out", dst, "--max-edges", "12", "--json"])
    assert json.loads(capsys.readouterr().out) == t and t["n_filled"] == 1 and t["n_too_many_edges"] == 1
    assert len(inference.read_ply(dst)["faces"]) == len(mesh["faces"]) + t["n_new_faces"] == 146
    M.main([src, "--list", "--rings", "1", "--keep-folded", "--normals", "none", "--fair", "2"])
    out = capsys.readouterr().out
    assert "loop 0: 32 edges, filled, 1 rings" in out and "loop 1: 12 edges, filled" in out and "2 loops (2 filled)" in out
    with pytest.raises(SystemExit):
        M.main([src, "--out", dst, "--rings", "some"])
    capsys.readouterr()


def test_extract_mesh_keywords():
    """fill_holes=dict(...) equals the call made by hand before the other steps; fill_holes=None is today's result bit for bit"""
    from nicer_slam_amd import inference, mesh_fill as M, mesh_topology
    from nicer_slam_amd.mesh_decimate import decimate
    from nicer_slam_amd.tsdf import TSDFVolume
    from test_mesh_gpu import _model
    import tsdf_ref
    m = _model()
    kw = dict(max_edges=4096, normals="angle")
    plain = inference.extract_mesh(m, 32, (-0.5, 0.5))                                  # the box cuts the surface
    same = inference.extract_mesh(m, 32, (-0.5, 0.5), fill_holes=None)
    assert set(plain) == set(same) and all(torch.equal(plain[k], same[k]) for k in plain)
    by_hand, rep = M.fill_holes(plain, return_report=True, **kw)
    fused = inference.extract_mesh(m, 32, (-0.5, 0.5), fill_holes=kw)
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)
    assert fused["faces"].shape[0] == plain["faces"].shape[0] + rep["totals"]["n_new_faces"]
    assert fused["colors"].shape == fused["verts"].shape == fused["normals"].shape
    both = inference.extract_mesh(m, 32, (-0.5, 0.5), fill_holes=kw, decimate=dict(target_faces=200))
    want = decimate(by_hand, target_faces=200)                                           # filled first, then decimated
    assert set(both) == set(want) and all(torch.equal(both[k], want[k]) for k in both)
    poses = tsdf_ref.ring_poses(4)
    depth, rgb = tsdf_ref.room_frames(poses, 60, 80, 50.0)
    vl = 0.03
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl, True)
    vol.integrate(depth, rgb, poses, tsdf_ref.pinhole(60, 80, 50.0))
    plain = vol.extract_mesh()
    before = mesh_topology.topology(plain)
    kw = dict(max_edges=100000, skip_folded=False)
    by_hand, rep = M.fill_holes(plain, return_report=True, **kw)
    fused = vol.extract_mesh(fill_holes=kw)
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)
    after = mesh_topology.topology(fused)
    print(before, rep["totals"], after)
    assert before["n_boundary"] > 0 and rep["totals"]["n_boundary"] == before["n_boundary"]
    assert after["n_boundary"] == before["n_boundary"] - sum(n for n, c in zip(rep["n"], rep["class"]) if c == "filled")
