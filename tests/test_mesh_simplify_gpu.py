"""Mesh simplification on the device (csrc/mesh_simplify.hip, nicer_slam_amd/mesh_simplify.py; header Section 19) against
the numpy float64 oracle tests/simplify_ref.py.  The combinatorial half -- vertex_cluster, the surviving faces, face_origin, every
total -- element for element, each case run twice and compared bit for bit.  Positions, normals and colours component by component
within 1e-7 h + one float32 ulp of the reference: the first term is about a thousand times the rounding bound of the 3 x 3 solve
(condition <= ~1 / eps = 1e3, <= 4096 incidences per cluster here, float64 unit 1.1e-16) and a thousand times below the float32 ulp
of the coordinates used; the second is the rounding of two float64 values that close.  Every vertex is held.  The small cases come
first in the file.

The issue's example of a cluster with tr == 0, one fed only by repeated-index faces, has no output vertex (every face that feeds it
is collapsed), so the tr == 0 OUTPUT vertices here come from a zero-area face (three collinear vertices in three cells)."""
import json

import numpy as np
import pytest
import torch

import clean_ref as C
import simplify_ref as S
import topology_ref as T

pytestmark = pytest.mark.gpu

TOTALS = S.TOTALS[:8]


def _bytes_equal(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _check_cluster(v, f, origin, h):
    """device == oracle on the combinatorial half; a second run is bit-identical.  Returns the oracle's dict."""
    from nicer_slam_amd import mesh_simplify as M
    ref = S.cluster(v, f, origin, h)
    vt, ft = torch.as_tensor(np.asarray(v, np.float32)).cuda(), torch.as_tensor(np.asarray(f)).cuda()
    got = M.cluster(ft, vt, h, origin)
    for k in TOTALS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("vertex_cluster", "faces", "face_origin", "out_cluster"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        assert np.array_equal(g, ref[k]), k
    again = M.cluster(ft, vt, h, origin)
    for k in got:
        assert (again[k] == got[k]) if not torch.is_tensor(got[k]) else _bytes_equal(again[k], got[k]), k
    return ref


def _within(got, ref64, h, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.float32 and got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err = np.abs(got.astype(np.float64) - ref64.astype(np.float32).astype(np.float64))
    bound = S.position_bound(ref64, h)
    worst = float((err - bound).max()) if err.size else 0.0
    assert (err <= bound).all(), (what, worst, float(err.max()))


def _check_simplify(mesh, h, origin=None, placements=("quadric", "mean")):
    """device == oracle on the whole result for each placement; a second run is bit-identical.  Returns the quadric oracle result."""
    from nicer_slam_amd import mesh_simplify as M
    dev = {k: torch.as_tensor(np.asarray(x)).cuda() for k, x in mesh.items()}
    o = S.default_origin(mesh["verts"]) if origin is None else np.asarray(origin, np.float64)
    out = None
    for placement in placements:
        ref = S.simplify(mesh, cell=h, placement=placement, origin=origin)
        got = M.simplify(dev, cell=h, placement=placement, origin=origin, return_map=True)
        assert got["totals"] == {k: ref["totals"][k] for k in TOTALS} and got["cell"] == ref["cell"]
        for k in ("faces", "vertex_cluster", "face_origin", "vertex_cell"):
            assert np.array_equal(got[k].cpu().numpy(), ref[k]), (placement, k)
        for k in ("verts", "normals", "colors"):
            assert (k in got) == (k in ref)
            if k in ref:
                _within(got[k], ref[k], h, (placement, k))
        assert S.in_cell_box(got["verts"].cpu().numpy(), got["vertex_cell"].cpu().numpy(), o, h), placement      # the box theorem
        again = M.simplify(dev, cell=h, placement=placement, origin=origin, return_map=True)
        for k, x in got.items():
            assert _bytes_equal(again[k], x) if torch.is_tensor(x) else again[k] == x, (placement, k)
        out = out or ref
    return out


def _with_attributes(v, f, seed=0):
    g = np.random.default_rng(seed)
    n = g.normal(size=v.shape).astype(np.float32)
    return {"verts": v, "faces": f, "normals": n, "colors": g.uniform(0, 1, v.shape).astype(np.float32)}


def test_hand_derived_cases():
    from nicer_slam_amd import mesh_simplify as M
    for name, (v, f, o, h) in S.hand_cases().items():
        _check_cluster(v, f, o, h)
        if name == "faces that do not contribute":                     # a vertex at cell 2^21: the front refuses the grid
            for front in (S.simplify, M.simplify):
                with pytest.raises(ValueError):
                    front({"verts": v, "faces": f}, cell=h, origin=o)
            continue
        ref = _check_simplify(_with_attributes(v, f), h, o)
        if name == "zero-area face":
            assert ref["info"]["tr_zero"].sum() == 3 and ref["totals"]["n_faces"] == 1, name
        if name == "tetrahedron in one cell":
            assert ref["totals"]["n_collapsed"] == 4 and ref["totals"]["n_faces"] == 0


def test_no_faces_and_no_vertices():
    from nicer_slam_amd import mesh_simplify as M
    v, f = S.icosphere(0)
    for vv, ff in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), f), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        _check_cluster(vv, ff, np.zeros(3), 0.5)
        got = M.simplify({"verts": vv, "faces": ff, "normals": vv}, cell=0.5, return_map=True)
        assert got["verts"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["normals"].shape == (0, 3)
        assert set(got["totals"].values()) == {0} and (got["vertex_cluster"] == -1).all()
    got = M.simplify({"verts": np.full((3, 3), np.nan, np.float32), "faces": np.array([[0, 1, 2]], np.int32)}, cell=0.5, return_map=True)
    assert got["totals"]["n_contributing"] == 0 and got["faces"].shape == (0, 3)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_key_width(axis):
    """two clumps 2000 units apart at h = 1e-3: the far clump's cell index is about 2e6 > 2^20, so the top byte of the key's word for
    that axis decides the order; moved to 2100 units it lies past 2^21 cells: its faces do not contribute, its vertices count as outside"""
    v, f, o, h = S.key_width_case(axis)
    ref = _check_cluster(v, f, o, h)
    assert ref["n_faces"] == 8 and ref["n_outside"] == 0
    cell = S.cells(v, o, h)[0][:, axis]
    assert cell[:4].max() < 2 ** 20 < cell[4:].min() < 2 ** 21
    _check_simplify({"verts": v, "faces": f}, h, o)
    v, f, o, h = S.key_width_case(axis, beyond=True)
    ref = _check_cluster(v, f, o, h)
    assert ref["n_outside"] == 4 and ref["n_contributing"] == 4 and (ref["vertex_cluster"][4:] == -1).all()


def test_adversarial_face_lists():
    for name, (f, V) in C.adversarial_cases(2000).items():
        v = S.adversarial_mesh(f, V)
        o = S.default_origin(v)
        _check_cluster(v, f, o, 0.11)
        _check_cluster(v, f, o, 0.7)
        _check_simplify(_with_attributes(v, f, 1), 0.3, placements=("quadric",))


@pytest.mark.parametrize("a,b", [(32, 30), (31, 31), (24, 40), (7, 73), (16, 32), (19, 27), (1024, 1024)])
def test_sheets_at_the_seams_of_the_scans(a, b):
    """a flat a x b quad sheet (topology_ref.quad_sheet), one vertex to a cell, so nothing merges: V' = V, F' = F and the output faces
    are the input faces under the returned vertex map.  V = 1023, 1024, 1025 and F = 1022, 1024, 1026 sit just below, at and just
    above the 1024 lanes of a block of the three rank scans (csrc/block_scan.hpp); the 1024 x 1024 sheet (V = 1 050 625, F = 2 097 152)
    has more blocks than the one workgroup that scans the block counts has lanes"""
    from nicer_slam_amd import mesh_simplify as M
    f, V = T.quad_sheet(a, b)
    F = 2 * a * b
    i = torch.arange(V, device="cuda")
    v = torch.stack([i // (b + 1), i % (b + 1), torch.zeros_like(i)], 1).float() + 0.5          # the centre of cell (i, j, 0)
    got = M.cluster(f, v, 1.0, (0.0, 0.0, 0.0))
    assert [got[k] for k in TOTALS] == [V, F, V, 0, 0, 0, V, F]
    vmap = torch.empty(V, dtype=torch.int64, device="cuda")
    vmap[got["out_cluster"].long()] = torch.arange(V, device="cuda")                             # cluster -> output vertex
    vmap = vmap[got["vertex_cluster"].long()]                                                    # vertex -> output vertex
    assert torch.equal(got["faces"].long(), vmap[f.long()])                   # (every sheet face already starts at its smallest vertex)
    assert torch.equal(got["face_origin"].long(), torch.arange(F, device="cuda"))
    assert torch.equal(vmap, torch.arange(V, device="cuda"))                  # cell keys ascend with the row-major vertex index


def test_cube():
    v, f = S.cube(8)
    for h in (0.21, 0.3, 0.77):
        _check_cluster(v, f, np.array([-1.01, -1.013, -1.017]), h)
        _check_simplify(_with_attributes(v, f, 2), h, (-1.01, -1.013, -1.017))


@pytest.fixture(scope="module")
def spheres():
    return {3: S.icosphere(3), 5: S.icosphere(5)}


@pytest.mark.parametrize("h", [0.05, 0.2, 0.37])
@pytest.mark.parametrize("subdivisions", [3, 5])
def test_icosphere(spheres, subdivisions, h):
    """1280 faces, and 20 480 faces (more than one workgroup in every kernel, several scan blocks)"""
    v, f = spheres[subdivisions]
    ref = _check_simplify(_with_attributes(v, f, 3), h)
    assert ref["info"]["incidences"].max() <= 4096
    if subdivisions == 3 and h == 0.37:
        assert ref["info"]["clamped"].any()                             # the clamp acts on at least one axis of one vertex
    if h == 0.05 and subdivisions == 3:
        assert ref["totals"]["n_faces"] == 1280                         # finer than the mesh: nothing merges


def test_target_faces(spheres):
    from nicer_slam_amd import mesh_simplify as M
    v, f = spheres[5]
    mesh = {"verts": v, "faces": f}
    ref = S.simplify(mesh, target_faces=2000)
    got = M.simplify(mesh, target_faces=2000, return_map=True)
    assert got["cell"] == ref["cell"]                                   # the same float64, bit for bit
    assert got["totals"] == {k: ref["totals"][k] for k in TOTALS} and 0 < got["totals"]["n_faces"] <= 2000
    for k in ("faces", "vertex_cluster", "face_origin"):
        assert np.array_equal(got[k], ref[k]), k
    _within(got["verts"], ref["verts"], ref["cell"], "verts")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------

def test_kinds_in_kinds_out_and_return_map(spheres):
    from nicer_slam_amd import mesh_simplify as M
    v, f = spheres[3]
    mesh = _with_attributes(v, f)
    a = M.simplify(mesh, cell=0.2)
    assert set(a) == {"verts", "faces", "normals", "colors"} and all(isinstance(x, np.ndarray) for x in a.values())
    assert a["verts"].dtype == np.float32 and a["faces"].dtype == np.int32
    b = M.simplify({k: torch.from_numpy(x) for k, x in mesh.items()}, cell=0.2, return_map=True)
    assert all(x.device.type == "cpu" for x in b.values() if torch.is_tensor(x))
    c = M.simplify({k: torch.from_numpy(x).cuda() for k, x in mesh.items()}, cell=0.2)
    for k in a:
        assert np.array_equal(a[k], b[k].numpy()) and b[k].numpy().tobytes() == c[k].cpu().numpy().tobytes(), k
    assert c["verts"].is_cuda
    assert b["vertex_cluster"].shape == (len(v),) and b["face_origin"].shape == (len(a["faces"]),)
    assert b["vertex_cell"].shape == a["verts"].shape and b["totals"]["n_faces"] == len(a["faces"]) and b["cell"] == 0.2
    plain = M.simplify({"verts": v, "faces": f.astype(np.int64)}, cell=0.2)
    assert set(plain) == {"verts", "faces"} and np.array_equal(plain["verts"], a["verts"])
    only = M.cluster(f, v, 0.2)
    assert isinstance(only["faces"], np.ndarray) and np.array_equal(only["faces"], a["faces"])


def test_simplified_mesh_feeds_the_other_mesh_tools(spheres, tmp_path):
    from nicer_slam_amd import inference, mesh_clean, mesh_simplify as M, mesh_topology
    from nicer_slam_amd.mesh_eval import TriIndex
    v, f = spheres[5]
    mesh = {k: torch.from_numpy(x).cuda() for k, x in _with_attributes(v, f).items()}
    small = M.simplify(mesh, cell=0.2)
    ref = S.simplify({"verts": v, "faces": f}, cell=0.2)
    r = mesh_topology.topology(small)
    assert r == {k: x for k, x in T.topology(ref["faces"], len(ref["verts"])).items() if k in r} and r["is_oriented"]
    dist, face, _ = TriIndex(small["verts"], small["faces"]).query(mesh["verts"])
    assert torch.isfinite(dist).all() and (face >= 0).all() and float(dist.max()) < 0.2
    kept, stats = mesh_clean.keep_components(small, "largest")
    assert stats["n_components"] == 1 and kept["faces"].shape == small["faces"].shape
    path = str(tmp_path / "small.ply")
    inference.write_ply(path, small)
    back = inference.read_ply(path)
    assert np.array_equal(back["verts"], small["verts"].cpu().numpy()) and np.array_equal(back["faces"], small["faces"].cpu().numpy())
    assert np.array_equal(back["normals"], small["normals"].cpu().numpy())
    assert np.array_equal(back["colors"], np.rint(small["colors"].cpu().numpy().clip(0, 1) * 255).astype(np.uint8) / np.float32(255))


def test_command_line_writes_the_printed_face_count(spheres, tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_simplify as M
    v, f = spheres[3]
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    inference.write_ply(src, {k: torch.from_numpy(x) for k, x in _with_attributes(v, f).items()})
    r = M.main([src, "--out", dst, "--faces", "300", "--json"])
    out = json.loads(capsys.readouterr().out)
    assert out == r and 0 < out["n_faces"] <= 300
    assert inference.read_ply(dst)["faces"].shape[0] == out["n_faces"]
    M.main([src, "--out", dst, "--cell", "0.3", "--placement", "mean"])
    text = capsys.readouterr().out
    n = inference.read_ply(dst)["faces"].shape[0]
    assert f"-> {n} faces" in text and n == S.cluster(v, f, S.default_origin(v), 0.3)["n_faces"]


def test_bad_arguments_raise():
    from nicer_slam_amd import mesh_simplify as M
    v, f = S.icosphere(0)
    mesh = {"verts": torch.from_numpy(v).cuda(), "faces": torch.from_numpy(f).cuda()}
    wide = {"verts": np.array([[0, 0, 0], [3e6, 0, 0], [0, 5, 0]], np.float32), "faces": np.array([[0, 1, 2]], np.int32)}
    for bad in (lambda: M.simplify(mesh), lambda: M.simplify(mesh, cell=0.1, target_faces=10), lambda: M.simplify(mesh, cell=0.0),
                lambda: M.simplify(mesh, cell=-2.0), lambda: M.simplify(wide, cell=1.0), lambda: M.simplify(mesh, cell=0.1, placement="svd"),
                lambda: M.simplify({"verts": np.zeros((3, 3), np.float32), "faces": np.array([[0, 1, 2]], np.int32)}, target_faces=5)):
        with pytest.raises(ValueError):
            bad()
    assert M.simplify(wide, cell=3e6 / 2 ** 21 * 1.01)["faces"].shape == (1, 3)       # just inside 2^21 cells
