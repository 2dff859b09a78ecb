"""Mesh topology on the device (csrc/mesh_topology.hip, nicer_slam_amd/mesh_topology.py; header Section 18) against the
numpy oracle tests/topology_ref.py: every array and every total element for element, each case run twice and compared bit for bit;
then where it plugs in -- keep_components(connectivity="edge"), mesh_sdf's sign="auto", TriIndex.topology, the command line.  It is all
integer work: no tolerance anywhere.  The small cases come first in the file."""
import json

import numpy as np
import pytest
import torch

import clean_ref as C
import p2m_ref as P
import sdf_ref as S
import topology_ref as T

pytestmark = pytest.mark.gpu

ARRAYS = ("edges", "edge_count", "edge_forward", "edge_start", "edge_halfedges", "face_edges")
TOTALS = ("n_edges", "n_contributing", "n_used_verts", "n_boundary", "n_nonmanifold", "n_inconsistent", "n_boundary_loops")


@pytest.fixture(scope="module")
def cases():
    return T.table_cases()


def _check(faces, V, mask=None, ref=None):
    """device == oracle on every array and total of the edge table and on the face labels; a second run is bit-identical.
    Returns (device table, device labels, n_components)."""
    from nicer_slam_amd import mesh_topology as M
    f = torch.as_tensor(np.asarray(faces)).cuda()
    m = None if mask is None else torch.as_tensor(np.asarray(mask)).cuda()
    t = M.edge_table(f, V, m)
    label, n = M.face_components(f, V, m)
    ref = ref or T.edge_table(faces, V, mask)
    for k in TOTALS:
        assert t[k] == ref[k], (k, t[k], ref[k])
    for k in ARRAYS:
        got = t[k].cpu().numpy()
        assert got.dtype == np.int32 and got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
        assert np.array_equal(got, ref[k]), k
    rl, rn = T.face_components(faces, V, mask, ref)
    assert n == rn and np.array_equal(label.cpu().numpy(), rl)
    t2 = M.edge_table(f, V, m)
    label2, n2 = M.face_components(f, V, m)
    for k in TOTALS:
        assert t2[k] == t[k], k
    for k in ARRAYS:
        assert torch.equal(t[k], t2[k]), k
    assert n2 == n and torch.equal(label, label2)
    return t, label, n


def test_hand_derived_cases(cases):
    from nicer_slam_amd import mesh_topology as M
    for name, (f, V, row) in cases.items():
        _check(f, V)
        r = M.topology({"verts": np.zeros((V, 3), np.float32), "faces": f})
        assert T.row_of(r) == row, name                                # the row the CPU test derives with the oracle
        assert r == {k: T.topology(f, V)[k] for k in M.REPORT_KEYS}, name
        assert isinstance(r["is_watertight"], bool) and isinstance(r["is_oriented"], bool)


def test_no_faces_and_a_single_face():
    from nicer_slam_amd import mesh_topology as M
    for V in (0, 5):
        t, label, n = _check(np.zeros((0, 3), np.int32), V)
        assert t["n_edges"] == 0 and n == 0 and label.numel() == 0 and t["edge_start"].tolist() == [0]
        r = M.topology({"verts": np.zeros((V, 3), np.float32), "faces": np.zeros((0, 3), np.int32)})
        assert r["n_faces"] == 0 and r["euler"] == 0 and not r["is_watertight"] and not r["is_oriented"]
    t, label, n = _check(np.array([[4, 2, 9]], np.int32), 10)
    assert t["edges"].tolist() == [[2, 4], [2, 9], [4, 9]] and t["edge_forward"].tolist() == [0, 1, 0]
    assert (t["n_boundary"], t["n_boundary_loops"], n) == (3, 1, 1) and label.tolist() == [0]
    _check(np.array([[4, 2, 9]], np.int32), 0)                         # faces without vertices: nothing contributes


def test_adversarial_face_lists():
    for name, (f, V) in C.adversarial_cases(2000).items():
        _check(f, V)


@pytest.mark.parametrize("V", [2 ** 16 + 3, 2 ** 24 + 3])
def test_key_width(V):
    """four faces on the highest indices: with 2^16 + 3 the third byte pass of both sort stages decides, with 2^24 + 3 the fourth"""
    f, V = T.high_index_faces(V)
    t, _, n = _check(f, V)
    assert t["n_edges"] == 6 and t["edges"][0].tolist() == [V - 4, V - 3] and n == 1
    low = np.concatenate([T.TET, f]).astype(np.int32)                  # and with keys in the lowest byte beside them
    assert _check(low, V)[2] == 2


def test_runs_across_workgroup_boundaries():
    f, V = T.fan(300)                                                  # one run of 300 half-edges
    t, _, _ = _check(f, V)
    assert t["edge_count"][0].item() == 300 and t["edge_forward"][0].item() == 300
    f, V = T.strip(5000)                                               # 15000 half-edges: 15 scan blocks, 4 sort blocks
    t, _, n = _check(f, V)
    assert (t["n_edges"], t["n_boundary"], t["n_inconsistent"], t["n_boundary_loops"], n) == (10001, 5002, 0, 1, 1)


# a x b quad sheets whose counts sit at the seams of the scans (csrc/block_scan.hpp): B = 1024 lanes to a block of the rank and count
# kernels, W = 1024 lanes in the one workgroup that scans the block counts.  3 F = 1020 and 1026 half-edges (3 F = 1024 does not
# exist); V = 1023, 1024, 1025 vertices; F = 1022, 1024, 1026 faces; and 3 F = 1 053 366 > W B, where a lane of the offsets scan owns
# more than one block.
SEAM_SHEETS = [(10, 17), (9, 19), (32, 30), (31, 31), (24, 40), (7, 73), (16, 32), (19, 27), (419, 419)]


@pytest.mark.parametrize("a,b", SEAM_SHEETS)
def test_sheets_at_the_seams_of_the_scans(a, b):
    """the sheet's table in closed form (topology_ref.quad_sheet), checked on the device; the small ones against the oracle as well"""
    from nicer_slam_amd import mesh_topology as M
    f, V = T.quad_sheet(a, b)
    F, E = 2 * a * b, 3 * a * b + a + b
    if F < 5000:
        _check(f.cpu().numpy(), V)
    t = M.edge_table(f, V)
    label, n = M.face_components(f, V)
    assert [t[k] for k in TOTALS] == [E, F, V, 2 * (a + b), 0, 0, 1]
    assert n == 1 and int(label.abs().max()) == 0
    lo, hi = t["edges"][:, 0].long(), t["edges"][:, 1].long()
    key = lo * V + hi
    assert bool((lo < hi).all()) and bool((key[1:] > key[:-1]).all())                  # every edge once, in (lo, hi) order
    count, start = t["edge_count"].long(), t["edge_start"].long()
    assert start[0].item() == 0 and start[E].item() == 3 * F and torch.equal(start[1:] - start[:-1], count)
    assert int((count == 1).sum()) == 2 * (a + b) and int((count == 2).sum()) == E - 2 * (a + b)
    assert bool((t["edge_forward"][count == 2] == 1).all())
    ends = torch.stack([f.long(), f.long().roll(-1, 1)], 2).reshape(-1, 2)            # half-edge 3 f + k runs from corner k to k + 1
    assert torch.equal(t["edges"].long()[t["face_edges"].reshape(-1).long()], ends.sort(1).values)


def test_face_mask(cases):
    f, V, _ = cases["mc sphere"]
    mask = (np.arange(len(f)) % 7 != 0).astype(np.uint8)
    keep = np.nonzero(mask)[0]
    c = T.edge_table(f[keep], V)                                       # the oracle on the compacted list, ids mapped back
    ref = dict(c)
    ref["edge_halfedges"] = 3 * keep[c["edge_halfedges"] // 3] + c["edge_halfedges"] % 3
    ref["face_edges"] = np.full((len(f), 3), -1, np.int64)
    ref["face_edges"][keep] = c["face_edges"]
    t, label, n = _check(f, V, mask, ref)
    assert t["n_boundary"] > 0 and (label.cpu().numpy()[mask == 0] == -1).all()
    _check(f, V, mask * 5)                                             # any non-zero byte sets a face
    _check(f, V, np.zeros(len(f), np.uint8))                           # nothing set


def test_face_adjacency_and_boundary_edges(cases):
    from nicer_slam_amd import mesh_topology as M
    f, V, _ = cases["mc torus"]
    adj = M.face_adjacency(torch.as_tensor(f).cuda(), V)
    assert adj.dtype == torch.int32 and np.array_equal(adj.cpu().numpy(), T.face_adjacency(f, V))
    assert adj.shape[0] == 1344
    got = M.face_adjacency(f, V)                                       # numpy in, numpy out
    assert isinstance(got, np.ndarray) and np.array_equal(got, adj.cpu().numpy())
    f, V, _ = cases["mc cut sphere"]
    t = T.edge_table(f, V)
    b = M.boundary_edges(torch.as_tensor(f).cuda(), V)
    assert np.array_equal(b.cpu().numpy(), t["edges"][t["edge_count"] == 1]) and b.shape[0] == 32


def test_bad_arguments_raise_without_a_launch():
    from nicer_slam_amd import mesh_topology as M
    f = torch.zeros(4, 3, dtype=torch.int32, device="cuda")
    for bad in (lambda: M.edge_table(f[:, :2], 4), lambda: M.edge_table(f.float(), 4), lambda: M.edge_table(f, -1),
                lambda: M.edge_table(f, 2 ** 31), lambda: M.edge_table(f, 4, torch.ones(5, dtype=torch.uint8, device="cuda")),
                lambda: M.face_components(f.long() + 2 ** 40, 4), lambda: M.face_adjacency(f.reshape(-1), 4),
                lambda: M.topology({"verts": torch.zeros(4, 2, device="cuda"), "faces": f}), lambda: M.topology({"verts": f})):
        with pytest.raises(ValueError):
            bad()


# ---- the device's own marching cubes ----------------------------------------------------------------------------------------------------

def _mc(vol, res):
    from nicer_slam_amd import inference
    ax = torch.linspace(-1, 1, res, dtype=torch.float64)
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol.float().cuda(), 0.0, (step,) * 3, (-1.0,) * 3)


def _grid(res):
    ax = torch.linspace(-1, 1, res, dtype=torch.float64)
    return torch.meshgrid(ax, ax, ax, indexing="ij")


def _sphere(X, Y, Z, c, r):
    return torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r


def _four_spheres():
    """the mesh of test_mesh_clean_gpu._four_spheres"""
    X, Y, Z = _grid(64)
    vol = None
    for c, r in (((-0.5, -0.5, -0.5), 0.30), ((0.5, 0.5, -0.4), 0.22), ((0.5, -0.5, 0.5), 0.15), ((-0.5, 0.6, 0.6), 0.08)):
        s = _sphere(X, Y, Z, c, r)
        vol = s if vol is None else torch.minimum(vol, s)
    return _mc(vol, 64)


def _blob_with_stray(res):
    """the mesh of test_mesh_clean_gpu._blob_with_stray"""
    X, Y, Z = _grid(res)
    s = lambda c, r: _sphere(X, Y, Z, c, r)
    blob = torch.minimum(torch.minimum(s((0.2, 0, 0), 0.4), s((-0.35, 0.25, 0.1), 0.25)), s((0, -0.3, 0.35), 0.2))
    return _mc(torch.minimum(blob, s((-0.75, -0.75, -0.75), 0.12)), res)


def test_marching_cubes_meshes_are_closed_and_oriented():
    from nicer_slam_amd import mesh_topology as M
    X, Y, Z = _grid(64)
    r = M.topology(_mc(_sphere(X, Y, Z, (0, 0, 0), 0.6), 64))
    assert r["is_oriented"] and r["euler"] == 2 and r["n_components"] == 1 and r["n_boundary_loops"] == 0
    r = M.topology(_mc(torch.sqrt((torch.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z) - 0.25, 64))
    assert r["is_oriented"] and r["euler"] == 0 and r["n_components"] == 1
    m = _four_spheres()
    from nicer_slam_amd.mesh_clean import components
    label, n = M.face_components(m["faces"], m["verts"].shape[0])
    _, fl, n_vertex, _ = components(m["faces"], m["verts"].shape[0])
    assert n == 4 and n_vertex == 4
    pairs = torch.unique(torch.stack([label.long(), fl.long()], 1), dim=0)
    assert pairs.shape[0] == 4                                         # the same partition of the faces
    r = M.topology(m)
    assert r["is_oriented"] and r["euler"] == 8 and r["n_components"] == 4
    _check(m["faces"].cpu().numpy(), m["verts"].shape[0])


# ---- keep_components(connectivity="edge") -----------------------------------------------------------------------------------------------

def test_keep_components_edge_connectivity_splits_at_a_pinch_vertex(cases):
    from nicer_slam_amd.mesh_clean import component_stats, keep_components
    f, V = T.two_tets_sharing_vertex()                                 # faces 0 .. 3 on vertices 0 .. 3, faces 4 .. 7 on 3 .. 6
    v = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [-2, 0, 0], [0, -2, 0], [0, 0, -2]], np.float32)    # the second is larger
    mesh = {"verts": v, "faces": f}
    both, st_v = keep_components(mesh, "largest")
    assert st_v["n_components"] == 1 and both["faces"].shape[0] == 8
    kept, st = keep_components(mesh, "largest", connectivity="edge")
    assert st["n_components"] == 2 and st["label"].tolist() == [0, 4]
    assert st["n_faces"].tolist() == [4, 4] and st["n_verts"].tolist() == [4, 4]                   # the pinch vertex counts twice
    assert st["kept"].tolist() == [False, True]
    assert np.array_equal(kept["faces"], T.TET) and np.array_equal(kept["verts"], v[3:])
    # the table is the one today's path gives on the mesh with vertex 3 listed once per component: slots 3 and 4
    split = np.concatenate([T.TET, T.TET + 4]).astype(np.int32)
    ref = component_stats(torch.from_numpy(v[[0, 1, 2, 3, 3, 4, 5, 6]]).cuda(), torch.from_numpy(split).cuda())
    for k in ("label", "n_faces", "n_verts", "area", "lo", "hi", "vertex_comp", "face_comp"):
        assert torch.equal(st[k].view(torch.uint8), ref[k].view(torch.uint8)), k
    # a larger closed mesh with a small tetrahedron hanging on its vertex 0
    sf, sV, _ = cases["mc sphere"]
    sv = T.mc_mesh("sphere")["verts"]
    tet = np.array([[0, sV, sV + 1], [0, sV + 1, sV + 2], [0, sV + 2, sV], [sV, sV + 2, sV + 1]], np.int32)
    extra = sv[0] + 0.05 * np.eye(3, dtype=np.float32)
    mesh = {"verts": np.concatenate([sv, extra]).astype(np.float32), "faces": np.concatenate([sf, tet]).astype(np.int32)}
    both, st_v = keep_components(mesh, "largest")
    assert st_v["n_components"] == 1 and both["faces"].shape[0] == len(sf) + 4
    kept, st = keep_components(mesh, "largest", connectivity="edge")
    assert st["n_components"] == 2 and int(st["n_verts"].sum()) == sV + 4
    assert np.array_equal(kept["faces"], sf) and np.array_equal(kept["verts"], sv)
    assert 0.99 < st["kept_area_fraction"] < 1.0
    lo, hi = extra[0] - 0.01, extra[0] + 0.01                          # a box around one corner of the tetrahedron
    assert not ((sv >= lo) & (sv <= hi)).all(1).any()
    kept, st = keep_components(mesh, "touching", (lo, hi), connectivity="edge")
    assert kept["faces"].shape[0] == 4 and kept["verts"].shape[0] == 4
    assert np.array_equal(kept["verts"], mesh["verts"][[0, sV, sV + 1, sV + 2]])


def test_keep_components_connectivities_agree_without_pinch_vertices():
    from nicer_slam_amd.mesh_clean import keep_components
    m = _blob_with_stray(48)
    kv, sv = keep_components(m, "largest")
    ke, se = keep_components(m, "largest", connectivity="edge")
    assert sv["n_components"] == se["n_components"] == 2
    for k in ("verts", "faces", "normals"):
        assert torch.equal(kv[k].view(torch.uint8), ke[k].view(torch.uint8)), k
    for k, x in sv.items():
        assert x == se[k] if not torch.is_tensor(x) else torch.equal(x.view(torch.uint8), se[k].view(torch.uint8)), k


# ---- sign="auto" ------------------------------------------------------------------------------------------------------------------------

def _seam_sphere():
    """a latitude-longitude sphere whose seam column is listed twice with the same coordinates"""
    v, f, _ = P.latlong_sphere(12, 24)
    v = v.reshape(13, 25, 3).copy()
    v[:, -1] = v[:, 0]
    return v.reshape(-1, 3), f


def test_sign_auto(cases):
    from nicer_slam_amd import mesh_sdf
    from nicer_slam_amd.mesh_eval import TriIndex
    g = np.random.default_rng(5)
    q = torch.from_numpy(g.uniform(-1, 1, (600, 3)).astype(np.float32)).cuda()
    for name, rule in (("mc sphere", "normal"), ("mc cut sphere", "winding")):
        f, V, _ = cases[name]
        m = T.mc_mesh("sphere", 16, (0.7, 0.0, 0.0) if "cut" in name else (0.0, 0.0, 0.0))
        assert np.array_equal(m["faces"], f)
        mesh = {"verts": m["verts"], "faces": f}
        assert mesh_sdf.resolve_sign(mesh, "auto") == rule and mesh_sdf.resolve_sign(mesh, "normal") == "normal"
        index = TriIndex(torch.from_numpy(m["verts"]).cuda(), torch.from_numpy(f).cuda())
        assert mesh_sdf.resolve_sign(index, "auto") == rule
        assert index.topology() == index.topology() and True in index._topology          # computed once, kept on the index
        auto = mesh_sdf.signed_distance(index, q, sign="auto")
        assert torch.equal(auto.view(torch.int64), mesh_sdf.signed_distance(index, q, sign=rule).view(torch.int64)), name
        assert torch.equal(mesh_sdf.contains(index, q, method="auto"), mesh_sdf.contains(index, q, method=rule))
        grid = mesh_sdf.mesh_sdf_grid(index, 12, band=0.3, sign="auto")
        assert torch.equal(grid.view(torch.int32), mesh_sdf.mesh_sdf_grid(index, 12, band=0.3, sign=rule).view(torch.int32))
    v, f = S.open_square()
    assert mesh_sdf.resolve_sign({"verts": v, "faces": f}, "auto") == "winding"
    v, f = _seam_sphere()
    mesh = {"verts": v, "faces": f}
    assert mesh_sdf.resolve_sign(mesh, "auto", weld=True) == "normal"
    assert mesh_sdf.resolve_sign(mesh, "auto", weld=False) == "winding"
    from nicer_slam_amd import mesh_topology as M
    welded, raw = M.topology(mesh, weld=True), M.topology(mesh, weld=False)
    ref = T.topology(S.weld_faces(v, f), len(v))
    assert welded["is_oriented"] and welded["euler"] == 2 and not raw["is_watertight"] and raw["n_boundary"] > 0
    assert (welded["n_edges"], welded["n_contributing"], welded["euler"]) == (ref["n_edges"], ref["n_contributing"], ref["euler"])
    with pytest.raises(ValueError):
        mesh_sdf.signed_distance(mesh, q, sign="nearest")


def test_weld_masks_out_faces_with_a_non_finite_vertex():
    from nicer_slam_amd import mesh_topology as M
    f, V = T.tetrahedron()
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [np.nan, 0, 0]], np.float32)
    f = np.concatenate([f, [[0, 1, 4]]]).astype(np.int32)
    assert M.topology({"verts": v, "faces": f}, weld=True)["is_oriented"]
    r = M.topology({"verts": v, "faces": f}, weld=False)
    assert r["n_contributing"] == 5 and r["n_nonmanifold"] == 1 and not r["is_watertight"]


def test_command_line_round_trips_the_report(tmp_path, capsys, cases):
    from nicer_slam_amd import inference, mesh_topology as M
    m = T.mc_mesh("sphere", 16, (0.7, 0.0, 0.0))
    path = str(tmp_path / "cut.ply")
    inference.write_ply(path, {k: torch.from_numpy(np.ascontiguousarray(m[k])) for k in ("verts", "normals", "faces")})
    r = M.main([path, "--json"])
    out = json.loads(capsys.readouterr().out)
    assert out == r == M.topology(inference.read_ply(path))
    assert T.row_of(out) == cases["mc cut sphere"][2] and list(out) == list(M.REPORT_KEYS)
    M.main([path, "--weld"])
    text = capsys.readouterr().out
    assert "watertight: no" in text and "boundary edges 32 in 1 loops" in text
