"""Mesh decimation on the device (header Section 22, csrc/mesh_decimate.hip) against the numpy statement of
tests/decimate_ref.py: the log, the faces, face_origin, vertex_map and every total element for element, the fp32 positions, colours
and area normals BYTE FOR BYTE -- the statement is + - * / on float64 in a stated order, so no tolerance takes part -- and a second
run bit-identical.  The angle normals go through atan2 and are held to one fp32 unit, as in test_mesh_smooth_gpu.py.  Then the public
interface, the extract_mesh keywords, a PLY round trip and the command line."""
import json

import numpy as np
import pytest
import torch

import clean_ref
import decimate_ref as D
import simplify_ref
import smooth_ref as S
import topology_ref as T

pytestmark = pytest.mark.gpu

KEYS = ("verts", "faces", "colors", "normals", "vertex_map", "face_origin", "log")


def _check(mesh, **kw):
    """the device against the oracle, twice; returns (device result, oracle result)"""
    from nicer_slam_amd import mesh_decimate as M
    got = M.decimate(mesh, normals="area", return_map=True, **kw)
    again = M.decimate(mesh, normals="area", return_map=True, **kw)
    ref = D.decimate(mesh, normals="area", **kw)
    print(f"F {len(mesh['faces'])} -> {got['totals']}")
    for k in KEYS:
        if k in ref:
            assert got[k].tobytes() == again[k].tobytes(), k                 # bit for bit, NaN or not
    assert got["totals"] == again["totals"]
    assert got["log"].shape == ref["log"].shape and (got["log"].astype(np.uint64) == ref["log"]).all()
    for k in ("faces", "face_origin", "vertex_map"):
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape and (got[k] == ref[k]).all(), k
    assert got["totals"] == ref["totals"]
    for k in ("verts", "colors", "normals"):
        assert (k in got) == (k in ref)
        if k in ref:
            assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape
            diff = (got[k].view(np.uint32) != ref[k].view(np.uint32)).any(1)
            assert not diff.any(), (k, int(diff.sum()), np.nonzero(diff)[0][:5], got[k][diff][:3], ref[k][diff][:3])
    return got, ref


@pytest.fixture(scope="module")
def sphere3():
    return D.mesh_of(*simplify_ref.icosphere(3), colors=True)


@pytest.fixture(scope="module")
def holed_grid():
    return D.mesh_of(*S.grid_mesh(17, (5, 6, 4), 0.3), colors=True)


# ---- the hand cases ------------------------------------------------------------------------------------------------------------------

def test_hand_cases():
    got, _ = _check(D.mesh_of(simplify_ref.TET_V, simplify_ref.TET_F), target_faces=2)
    assert got["verts"].tobytes() == simplify_ref.TET_V.tobytes() and (got["faces"] == simplify_ref.TET_F).all()
    quad = D.mesh_of(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), [[0, 1, 2], [0, 2, 3]])
    got, _ = _check(quad, max_error=1e-6)
    assert got["totals"]["collapses"] == 0 and len(got["faces"]) == 2
    v, f = S.grid_mesh(9)
    got, _ = _check(D.mesh_of(v, f), max_error=1e-6)
    assert len(got["faces"]) < 16 and abs(D.area(got["verts"], got["faces"]) - 64.0) < 1e-9
    f2, V2 = T.two_tets_sharing_edge()
    v2 = S.index_only_mesh(f2, V2)
    got, _ = _check(D.mesh_of(v2, f2), target_faces=2, min_cos=0.0)
    assert (got["vertex_map"][:2] >= 0).all() and got["verts"][got["vertex_map"][:2]].tobytes() == v2[:2].tobytes()


def test_no_faces_no_vertices_bad_indices_and_a_nan():
    from nicer_slam_amd import mesh_decimate as M
    none = M.decimate(D.mesh_of(np.zeros((0, 3)), np.zeros((0, 3))), target_faces=4, return_map=True)
    assert none["verts"].shape == (0, 3) and none["faces"].shape == (0, 3) and none["totals"]["rounds"] == 0
    v = simplify_ref.icosphere(1)[0]
    _check(D.mesh_of(v, np.zeros((0, 3))), target_faces=4)
    _check(D.mesh_of(np.zeros((0, 3)), simplify_ref.TET_F), target_faces=1)
    v, f = simplify_ref.icosphere(2)
    f = f.copy()
    f[3, 1], f[40, 0] = -1, len(v)                                               # the indices -1 and V: the faces are dropped
    v = v.copy()
    v[17, 2] = np.nan
    got, ref = _check(D.mesh_of(v, f, colors=True), target_faces=100)
    assert len(got["faces"]) in (99, 100) and np.isnan(got["verts"]).sum() == 1
    st = ref["state"]
    assert st.locked[17] and st.locked[st.faces[(st.faces == 17).any(1)]].all() and not st.moved[st.locked].any()


# ---- the icosphere, the cube ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", [1000, 300, 20])
def test_icosphere_to_a_face_count(sphere3, target):
    got, _ = _check(sphere3, target_faces=target)
    assert len(got["faces"]) in (target, target - 1)
    r = T.topology(got["faces"], len(got["verts"]))
    assert r["is_watertight"] and r["euler"] == 2 and r["n_components"] == 1


def test_icosphere_to_an_error(sphere3):
    got, _ = _check(sphere3, max_error=0.01)
    assert 20 < len(got["faces"]) < 1280 and got["totals"]["n_candidates"] == 0 and got["totals"]["rej_error"] > 0
    both, _ = _check(sphere3, max_error=0.01, target_faces=800)
    assert len(both["faces"]) in (799, 800)


def test_cube_with_a_tiny_error():
    v, f = simplify_ref.cube(8)
    got, _ = _check(D.mesh_of(v, f), max_error=1e-6, max_rounds=40)
    assert len(got["faces"]) < len(f) and abs(simplify_ref.volume(got["verts"], got["faces"]) - simplify_ref.volume(v, f)) < 1e-9
    assert T.topology(got["faces"], len(got["verts"]))["is_watertight"]


# ---- long rows, many blocks, odd lists -----------------------------------------------------------------------------------------------

def test_fan_with_one_row_of_300():
    v, f = S.fan_mesh(300)
    got, _ = _check(D.mesh_of(v, f), target_faces=10, min_cos=0.0)
    assert got["totals"]["collapses"] == 0 and got["totals"]["rej_lock"] == 601       # both hub vertices lie on the non-manifold edge


def test_strip_of_5000():
    f, V = T.strip(5000)
    got, _ = _check(D.mesh_of(S.index_only_mesh(f, V), f), target_faces=4000, min_cos=0.0, max_rounds=6)
    assert got["totals"]["collapses"] > 0


def test_moebius():
    f, V = T.moebius(24)
    a = np.linspace(0.0, 2.0 * np.pi, 24, endpoint=False)
    ring = np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], 1)
    off = 0.2 * np.stack([np.cos(a / 2) * np.cos(a), np.cos(a / 2) * np.sin(a), np.sin(a / 2)], 1)
    v = np.empty((V, 3))
    v[0::2], v[1::2] = ring + off, ring - off
    got, _ = _check(D.mesh_of(v, f, colors=True), target_faces=24)
    t0, t1 = T.topology(f, V), T.topology(got["faces"], len(got["verts"]))
    assert t1["n_boundary_loops"] == t0["n_boundary_loops"] == 1 and t1["euler"] == t0["euler"] == 0


def test_adversarial_face_lists_and_non_finite_vertices():
    for name, (f, V) in clean_ref.adversarial_cases(2000).items():
        v = simplify_ref.adversarial_mesh(f, V)
        got, ref = _check(D.mesh_of(v, f, colors=True), target_faces=len(f) // 4, min_cos=0.0, max_rounds=5)
        assert np.isfinite(ref["state"].X[ref["state"].moved]).all(), name


# ---- boundaries, masks, the round limit ------------------------------------------------------------------------------------------------

def test_boundary_fixed_and_a_fixed_mask(holed_grid):
    V = len(holed_grid["verts"])
    fixed = np.random.default_rng(4).random(V) < 0.15
    free, _ = _check(holed_grid, target_faces=150)
    held, ref = _check(holed_grid, target_faces=150, boundary="fixed", fixed=fixed)
    st = ref["state"]
    assert not st.moved[fixed].any() and (held["vertex_map"][fixed] >= 0).all()
    assert held["verts"][held["vertex_map"][fixed]].tobytes() == holed_grid["verts"][fixed].tobytes()
    for out in (free, held):
        t = T.topology(out["faces"], len(out["verts"]))
        assert t["n_boundary_loops"] == 2 and t["euler"] == 0 and t["n_nonmanifold"] == 0
    _check(holed_grid, max_error=0.05, boundary_weight=100.0)


def test_one_round(sphere3):
    got, _ = _check(sphere3, target_faces=20, max_rounds=1)
    assert got["totals"]["rounds"] == 1 and 0 < got["totals"]["collapses"] == len(got["log"]) and (got["log"][:, 0] == 0).all()
    cost = got["log"][:, 3].astype(np.uint64)
    assert (cost[1:] >= cost[:-1]).all()                                         # the log is in key order


# ---- the public interface ----------------------------------------------------------------------------------------------------------------

def test_kinds_in_kinds_out_and_angle_normals(sphere3):
    from nicer_slam_amd import mesh_decimate as M
    ref = D.decimate(sphere3, target_faces=400)
    a = M.decimate(sphere3, target_faces=400)
    assert set(a) == {"verts", "faces", "colors", "normals"} and all(isinstance(x, np.ndarray) for x in a.values())
    assert a["verts"].tobytes() == ref["verts"].tobytes() and (a["faces"] == ref["faces"]).all()
    err = np.abs(a["normals"].astype(np.float64) - ref["normals"].astype(np.float64)).max()
    print(f"angle normals: max |device - oracle| {err:.3e}")
    assert err <= 2.0 ** -23                                                     # test_mesh_smooth_gpu.py's bound for the angle form
    assert "normals" not in M.decimate(sphere3, target_faces=400, normals=None)
    cpu = {k: torch.from_numpy(x) for k, x in sphere3.items()}
    b = M.decimate(cpu, target_faces=400, return_map=True)
    assert all(torch.is_tensor(b[k]) and not b[k].is_cuda for k in KEYS) and b["verts"].numpy().tobytes() == ref["verts"].tobytes()
    gpu = {k: x.cuda() for k, x in cpu.items()}
    gpu["faces"] = gpu["faces"].long()
    c = M.decimate(gpu, target_faces=400, return_map=True)
    assert all(c[k].is_cuda for k in KEYS) and c["faces"].dtype == torch.int32 and c["verts"].cpu().numpy().tobytes() == ref["verts"].tobytes()
    assert c["totals"] == ref["totals"] and (c["vertex_map"].cpu().numpy() == ref["vertex_map"]).all()
    assert (c["log"].cpu().numpy().astype(np.uint64) == ref["log"]).all()


def test_other_tools_take_the_result_and_ply_round_trip(sphere3, tmp_path):
    from nicer_slam_amd import inference, mesh_decimate as M, mesh_smooth, mesh_topology
    from nicer_slam_amd.mesh_eval import TriIndex
    out = M.decimate({k: torch.from_numpy(x).cuda() for k, x in sphere3.items()}, target_faces=300)
    r = mesh_topology.topology(out)
    assert r["is_oriented"] and r["euler"] == 2 and r["n_faces"] in (299, 300)
    q = torch.from_numpy(sphere3["verts"]).cuda()
    d = TriIndex(out["verts"], out["faces"]).query(q)[0]
    assert float(d.max()) < 0.1                                                  # the unit sphere at 300 faces: sag below 0.1
    sm = mesh_smooth.smooth(out, iterations=2)
    assert sm["verts"].shape == out["verts"].shape and bool(torch.isfinite(sm["verts"]).all())
    path = str(tmp_path / "decimated.ply")
    inference.write_ply(path, out)
    back = inference.read_ply(path)
    assert back["verts"].tobytes() == out["verts"].cpu().numpy().tobytes() and np.array_equal(back["faces"], out["faces"].cpu().numpy())


def test_command_line(sphere3, tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_decimate as M
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    mesh = dict(sphere3, normals=S.vertex_normals(sphere3["verts"], sphere3["faces"], "area"))
    inference.write_ply(src, {k: torch.from_numpy(x) for k, x in mesh.items()})
    r = M.main([src, "--out", dst, "--faces", "300", "--json"])
    assert json.loads(capsys.readouterr().out) == r and r["n_faces"] == 300
    assert len(inference.read_ply(dst)["faces"]) == 300
    M.main([src, "--out", dst, "--max-error", "0.01", "--boundary", "fixed", "--min-cos", "0.3", "--normals", "area"])
    n = len(inference.read_ply(dst)["faces"])
    assert f"-> {n} faces" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        M.main([src, "--out", dst])
    capsys.readouterr()


def test_extract_mesh_keywords():
    """decimate=dict(...) equals the call made by hand after simplify; decimate=None is today's result bit for bit"""
    from nicer_slam_amd import inference, mesh_decimate as M
    from nicer_slam_amd.mesh_simplify import simplify
    from nicer_slam_amd.tsdf import TSDFVolume
    from test_mesh_gpu import _model
    import tsdf_ref
    m = _model()
    kw = dict(target_faces=500, normals="area")
    plain = inference.extract_mesh(m, 32, (-1.0, 1.0))
    same = inference.extract_mesh(m, 32, (-1.0, 1.0), decimate=None)
    assert plain["faces"].shape[0] > 500 and all(torch.equal(plain[k], same[k]) for k in plain) and set(plain) == set(same)
    by_hand = M.decimate(plain, **kw)
    fused = inference.extract_mesh(m, 32, (-1.0, 1.0), decimate=kw)
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)
    assert fused["faces"].shape[0] in (499, 500) and fused["colors"].shape == fused["verts"].shape
    both = inference.extract_mesh(m, 32, (-1.0, 1.0), simplify=dict(cell=0.1), decimate=dict(target_faces=200))
    want = M.decimate(simplify(plain, cell=0.1), target_faces=200)                # simplified first, then decimated
    assert set(both) == set(want) and all(torch.equal(both[k], want[k]) for k in both)
    poses = tsdf_ref.ring_poses(4)
    depth, rgb = tsdf_ref.room_frames(poses, 60, 80, 50.0)
    vl = 0.03
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl, True)
    vol.integrate(depth, rgb, poses, tsdf_ref.pinhole(60, 80, 50.0))
    plain = vol.extract_mesh()
    fused = vol.extract_mesh(decimate=dict(max_error=0.002, max_rounds=4))
    by_hand = M.decimate(plain, max_error=0.002, max_rounds=4)
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)
    assert 0 < fused["faces"].shape[0] < plain["faces"].shape[0]
    with pytest.raises(ValueError):
        vol.extract_mesh(decimate="quadric")
