"""Mesh smoothing on the device (header Section 21, csrc/mesh_smooth.hip) against the numpy statement of
tests/smooth_ref.py: the ring element for element, the smoothed positions and the area normals BYTE FOR BYTE -- the statement is
+ - * / and sqrt on float64 in a stated order, so no tolerance takes part -- and a second run bit-identical.  The angle normals go
through atan2 and are held to one fp32 unit.  Then the public interface, the two extract_mesh keywords, a PLY round trip and the
command line."""
import json

import numpy as np
import pytest
import torch

import clean_ref
import simplify_ref
import smooth_ref as S
import topology_ref as T

pytestmark = pytest.mark.gpu

ODD = [0.5, -0.53, 0.5]                                    # an odd count ends in the other ping-pong buffer


def _device(verts, faces, factors, boundary="curve", fixed=None, max_move=None):
    """the three entry points through the module's own device helpers: dict of numpy arrays"""
    from nicer_slam_amd import mesh_smooth as M
    from nicer_slam_amd import mesh_topology as MT
    v32 = np.ascontiguousarray(verts, np.float32)
    V = len(v32)
    f, V, F, _, _ = MT._checked(np.asarray(faces).reshape(-1, 3), V, None, "test")
    v = torch.from_numpy(v32).cuda()
    t, totals = MT._edge_table(f, V, F, None)
    rings = M._ring(t, V, F, f.device)
    n = 2 * totals["n_edges"]
    mask = None if fixed is None else torch.from_numpy((np.asarray(fixed).reshape(-1) != 0).astype(np.uint8)).cuda()
    out, state = M._smooth(v, V, F, t, rings, list(factors), boundary, mask, max_move)
    return dict(ring_start=rings[0].cpu().numpy(), ring=rings[1][:n].cpu().numpy(), ring_edge=rings[2][:n].cpu().numpy(),
                out=out.cpu().numpy(), state=state.cpu().numpy(), normals=M._vertex_normals(v, f, V, F, "area").cpu().numpy())


def _check(verts, faces, factors=ODD, boundary="curve", fixed=None, max_move=None, ring=None):
    """the device against the oracle, twice; returns (device result, oracle output)"""
    v32 = np.ascontiguousarray(verts, np.float32)
    got = _device(v32, faces, factors, boundary, fixed, max_move)
    again = _device(v32, faces, factors, boundary, fixed, max_move)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k                     # bit for bit, NaN or not
    ring = ring or S.vertex_ring(faces, len(v32))
    for k in ("ring_start", "ring", "ring_edge"):
        assert got[k].shape == ring[k].shape and (got[k] == ring[k]).all(), k
    out, state = S.smooth_steps(v32, faces, factors, boundary, fixed, max_move, ring=ring)
    assert (got["state"] == state).all()
    diff = (got["out"].view(np.uint32) != out.view(np.uint32)).any(1)
    assert not diff.any(), (int(diff.sum()), np.nonzero(diff)[0][:5], got["out"][diff][:3], out[diff][:3])
    assert got["normals"].tobytes() == S.vertex_normals(v32, faces, "area").tobytes()
    return got, out


@pytest.fixture(scope="module")
def spheres():
    return {s: S.noisy_icosphere(s)[:2] for s in (3, 5)}


@pytest.fixture(scope="module")
def holed_grid():
    v, f = S.grid_mesh(17, (6, 6, 3), 0.5)
    return v, f, S.vertex_ring(f, len(v))


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------

def test_no_faces_no_vertices_one_face():
    v = np.random.default_rng(0).uniform(-1, 1, (5, 3)).astype(np.float32)
    got, _ = _check(v, np.zeros((0, 3), np.int32))
    assert got["out"].tobytes() == v.tobytes() and (got["state"] == 0).all() and (got["normals"] == 0).all()
    assert got["ring_start"].tolist() == [0] * 6 and got["ring"].size == 0
    _check(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    _check(np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))      # faces over no vertices: nothing contributes
    got, out = _check(v, np.array([[3, 0, 4]], np.int32), boundary="free")
    assert got["ring"].tolist() == [3, 4, 0, 4, 0, 3] and (out[[1, 2]] == v[[1, 2]]).all() and (out[[0, 3, 4]] != v[[0, 3, 4]]).any()
    for boundary in ("fixed", "curve"):                                        # every edge of a single face is a boundary edge
        _check(v, np.array([[3, 0, 4]], np.int32), boundary=boundary)


def test_n_steps_zero_returns_the_input_bits(spheres):
    v, f = spheres[3]
    v = v.copy()
    v.view(np.uint32)[7, 1] = 0x7FC00ABC                                       # a NaN with a payload
    got, _ = _check(v, f, factors=[])
    assert got["out"].tobytes() == v.tobytes() and got["state"][7] == 0 and got["state"][8] == S.LIVE | S.MOVES | S.STEPS


# ---- rows, keys, names ------------------------------------------------------------------------------------------------------------------

def test_high_valence_rows():
    """two rows of 301 entries, longer than a wave; every other row has 2; every edge but one is a boundary edge and that one is
    non-manifold, an ordinary edge for smoothing"""
    v, f = S.fan_mesh(300)
    for boundary in S.BOUNDARY:
        got, _ = _check(v, f, boundary=boundary)
    assert np.diff(got["ring_start"]).tolist() == [301, 301] + [2] * 300


def test_key_width_and_empty_rows():
    """V = 70000 needs three 8-bit passes of the sort; 69 996 rows are empty"""
    f, V = T.high_index_faces(70000)
    v = S.index_only_mesh(f, V)
    got, out = _check(v, f, boundary="free")
    assert (np.diff(got["ring_start"])[:-4] == 0).all() and (out[:-4] == v[:-4]).all() and (out[-4:] != v[-4:]).any(1).all()


def test_permuted_vertex_names():
    f, V = T.strip(5000)
    _check(S.index_only_mesh(f, V), f)
    _check(S.index_only_mesh(f, V), f, boundary="free", factors=[1.0, -1.0])


def test_adversarial_face_lists_and_non_finite_vertices():
    """invalid indices, repeated indices, non-finite vertices: those come back with their input bits and poison no neighbour"""
    for name, (f, V) in clean_ref.adversarial_cases(2000).items():
        v = simplify_ref.adversarial_mesh(f, V)
        got, out = _check(v, f)
        bad = ~np.isfinite(v).all(1)
        assert got["out"][bad].tobytes() == v[bad].tobytes() and np.isfinite(got["out"][~bad]).all(), name
        assert np.isfinite(got["normals"]).all(), name


# ---- block tails, step counts, the clamp ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("factors", [[0.5], [0.5] * 2, [0.5] * 3, S.factors_of("taubin", 10)], ids=["1", "2", "3", "taubin 10"])
def test_step_counts(spheres, factors):
    """642 vertices, no multiple of 256; 1, 2 and 3 steps end in different ping-pong buffers"""
    v, f = spheres[3]
    _check(v, f, factors=factors)


def test_ten_thousand_vertices(spheres):
    v, f = spheres[5]
    assert len(v) == 10242
    _check(v, f, factors=S.factors_of("taubin", 3))


def test_clamp(spheres):
    v, f = spheres[3]
    got, out = _check(v, f, factors=S.factors_of("taubin", 10), max_move=0.01)
    x0 = v.astype(np.float64)                                                # from the oracle: some vertices end on the clamp, not all
    clamped = ((out == (x0 + 0.01).astype(np.float32)) | (out == (x0 - 0.01).astype(np.float32))).any(1)
    assert clamped.sum() == 204 and len(v) == 642
    assert (np.abs(got["out"].astype(np.float64) - v.astype(np.float64)) <= 0.01 + 2.0 ** -24).all()


@pytest.mark.parametrize("boundary", S.BOUNDARY)
def test_boundary_modes(holed_grid, boundary):
    """76 boundary edges in two loops and four unused vertices"""
    v, f, ring = holed_grid
    got, out = _check(v, f, factors=S.factors_of("taubin", 10), boundary=boundary, ring=ring)
    unused = np.diff(ring["ring_start"]) == 0
    assert unused.sum() == 4 and (out[unused] == v[unused]).all() and ((got["state"] & S.ON_BOUNDARY) != 0).sum() == 76
    fixed = np.random.default_rng(12).random(len(v)) < 0.3
    got, out = _check(v, f, factors=ODD, boundary=boundary, fixed=fixed, ring=ring)
    assert (out[fixed] == v[fixed]).all() and (out[~fixed & ~unused] != v[~fixed & ~unused]).any()


def test_boundary_modes_differ(holed_grid):
    v, f, ring = holed_grid
    out = {b: _device(v, f, S.factors_of("taubin", 10), b)["out"] for b in S.BOUNDARY}
    assert min(np.abs(out[a] - out[b]).max() for a, b in (("free", "fixed"), ("free", "curve"), ("fixed", "curve"))) > 0.2


# ---- angle normals -----------------------------------------------------------------------------------------------------------------------

def test_angle_normals(spheres):
    """Per component within 2^-23, one fp32 unit at unit length.  The statement differs from the oracle only in atan2, which the
    device's math library computes to a few float64 units (its reference documentation is not part of the ROCm tree here, so no
    figure is quoted; a thousand units would do).  Rows have at most 9 corners and |N| >= 0.33 sum(theta) on these inputs -- 0.97 on the two
    marching-cubes meshes, 0.85 and 0.34 on the noisy icospheres, from the oracle -- so the float64 normals disagree by less
    than 1e-13, seven orders under half an fp32 unit: only a rounding near-tie can flip the last bit.  A vertex with
    |N| < 1e-3 sum(theta) would be held to "finite and unit or zero" only; none is on these inputs, which the test asserts."""
    from nicer_slam_amd import mesh_smooth as M
    meshes = [spheres[3], spheres[5]] + [(m["verts"], m["faces"]) for m in (T.mc_mesh("sphere", 16), T.mc_mesh("torus", 24))]
    for v, f in meshes:
        ref, N, W, count = S.vertex_normals(v, f, "angle", return_sums=True)
        assert count.max() <= 9 and (np.linalg.norm(N, axis=1) >= 1e-3 * W).all()      # the guard leaves out no vertex
        got = M.vertex_normals({"verts": v, "faces": f}, "angle")
        assert got.dtype == np.float32 and got.shape == ref.shape
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
        print(f"angle normals: V {len(v)}  max |device - oracle| {err:.3e}  differing components {(got != ref).sum()}")
        assert err <= 2.0 ** -23
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        assert got.tobytes() == M.vertex_normals({"verts": v, "faces": f}, "angle").tobytes()


# ---- the public interface ----------------------------------------------------------------------------------------------------------------

def _with_attributes(v, f):
    g = np.random.default_rng(21)
    return {"verts": v, "faces": f, "normals": S.vertex_normals(v, f, "area"), "colors": g.random((len(v), 3)).astype(np.float32)}


def test_kinds_in_kinds_out(spheres):
    from nicer_slam_amd import mesh_smooth as M
    v, f = spheres[3]
    mesh = _with_attributes(v, f)
    ref, state = S.smooth_steps(v, f, S.factors_of("taubin", 10))
    a, rep = M.smooth(mesh, return_report=True)
    assert isinstance(a["verts"], np.ndarray) and a["verts"].tobytes() == ref.tobytes() and a["faces"] is mesh["faces"]
    assert a["colors"] is mesh["colors"] and a["normals"].tobytes() == M.vertex_normals({"verts": ref, "faces": f}, "angle").tobytes()
    assert rep == dict(n_verts=642, n_steps=20, n_live=642, n_moving=642, n_boundary=0, n_held=0,
                       max_move=float(np.abs(ref - v).max()))
    assert M.smooth(mesh, normals="area")["normals"].tobytes() == S.vertex_normals(ref, f, "area").tobytes()
    assert M.smooth(mesh, normals="keep")["normals"] is mesh["normals"] and "normals" not in M.smooth(mesh, normals=None)
    lap = M.smooth(mesh, "laplacian", 3, 0.25, mu=7.0)                           # laplacian ignores mu
    assert lap["verts"].tobytes() == S.smooth_steps(v, f, [0.25] * 3)[0].tobytes()
    fixed = np.arange(len(v)) % 3 == 0
    held, rep = M.smooth(mesh, fixed=fixed, max_move=0.01, boundary="free", return_report=True)
    assert held["verts"].tobytes() == S.smooth_steps(v, f, S.factors_of("taubin", 10), "free", fixed, 0.01)[0].tobytes()
    assert rep["n_held"] == int(fixed.sum()) and rep["n_moving"] == int((~fixed).sum()) and rep["max_move"] <= 0.01 + 2.0 ** -24
    cpu = {k: torch.from_numpy(x) for k, x in mesh.items()}
    b = M.smooth(cpu)
    assert all(torch.is_tensor(b[k]) and not b[k].is_cuda for k in b) and b["verts"].numpy().tobytes() == ref.tobytes()
    gpu = {k: x.cuda() for k, x in cpu.items()}
    c = M.smooth(gpu)
    assert all(c[k].is_cuda for k in c) and c["verts"].cpu().numpy().tobytes() == ref.tobytes() and c["faces"].dtype == torch.int32
    assert torch.equal(c["normals"], M.vertex_normals(c, "angle")) and M.vertex_normals(cpu, "area").device.type == "cpu"
    ring = M.vertex_ring(f, len(v))
    r = S.vertex_ring(f, len(v))
    assert all(isinstance(ring[k], np.ndarray) and (ring[k] == r[k]).all() for k in ("ring_start", "ring", "ring_edge"))
    assert ring["n_edges"] == 1920 and ring["n_boundary"] == 0               # F = 1280 faces, 3 F / 2 edges
    tr = M.vertex_ring(torch.from_numpy(f.astype(np.int64)).cuda(), len(v))
    assert tr["ring"].is_cuda and tr["ring"].dtype == torch.int32 and (tr["ring"].cpu().numpy() == r["ring"]).all()


def test_topology_is_unchanged_and_ply_round_trip(spheres, tmp_path):
    from nicer_slam_amd import inference, mesh_smooth as M, mesh_topology
    v, f = spheres[3]
    mesh = {k: torch.from_numpy(x).cuda() for k, x in _with_attributes(v, f).items()}
    out = M.smooth(mesh)
    assert mesh_topology.topology(out) == mesh_topology.topology(mesh) and mesh_topology.topology(out)["is_oriented"]
    path = str(tmp_path / "smooth.ply")
    inference.write_ply(path, out)
    back = inference.read_ply(path)
    assert back["verts"].tobytes() == out["verts"].cpu().numpy().tobytes() and np.array_equal(back["faces"], f)
    assert back["normals"].tobytes() == out["normals"].cpu().numpy().tobytes()
    del back["normals"]                                                          # a PLY without normals gets them from its faces
    assert M.vertex_normals(back).tobytes() == out["normals"].cpu().numpy().tobytes()


def test_command_line(spheres, tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_smooth as M
    v, f = spheres[3]
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    inference.write_ply(src, {k: torch.from_numpy(x) for k, x in _with_attributes(v, f).items()})
    colours = inference.read_ply(src)["colors"]
    r = M.main([src, "--out", dst, "--json"])
    assert json.loads(capsys.readouterr().out) == r and r["n_steps"] == 20 and r["n_moving"] == 642
    back = inference.read_ply(dst)
    assert back["verts"].tobytes() == S.smooth_steps(v, f, S.factors_of("taubin", 10))[0].tobytes()
    assert np.array_equal(back["colors"], colours)
    M.main([src, "--out", dst, "--method", "laplacian", "--iterations", "2", "--lam", "0.25", "--boundary", "free", "--max-move", "0.005",
            "--normals", "keep"])
    assert f"-> {dst}" in capsys.readouterr().out
    back = inference.read_ply(dst)
    assert back["verts"].tobytes() == S.smooth_steps(v, f, [0.25] * 2, "free", None, 0.005)[0].tobytes()
    assert back["normals"].tobytes() == S.vertex_normals(v, f, "area").tobytes()
    with pytest.raises(SystemExit):
        M.main([src, "--out", dst, "--lam", "2"])
    capsys.readouterr()


def test_extract_mesh_keywords():
    """smooth=dict(...) equals the two calls made by hand; smooth=None is today's result bit for bit"""
    from nicer_slam_amd import inference, mesh_smooth as M
    from nicer_slam_amd.tsdf import TSDFVolume
    from test_mesh_gpu import _model
    import tsdf_ref
    m = _model()
    kw = dict(method="taubin", iterations=3, normals="area")
    plain = inference.extract_mesh(m, 32, (-1.0, 1.0))
    same = inference.extract_mesh(m, 32, (-1.0, 1.0), smooth=None)
    assert plain["verts"].shape[0] > 0 and all(torch.equal(plain[k], same[k]) for k in plain) and set(plain) == set(same)
    by_hand = M.smooth(plain, **kw)
    fused = inference.extract_mesh(m, 32, (-1.0, 1.0), smooth=kw)
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)
    assert torch.equal(fused["colors"], plain["colors"]) and not torch.equal(fused["verts"], plain["verts"])
    both = inference.extract_mesh(m, 32, (-1.0, 1.0), smooth=kw, simplify=dict(cell=0.2))
    from nicer_slam_amd.mesh_simplify import simplify
    assert all(torch.equal(both[k], x) for k, x in simplify(by_hand, cell=0.2).items())      # smoothed first, then simplified
    poses = tsdf_ref.ring_poses(4)
    depth, rgb = tsdf_ref.room_frames(poses, 60, 80, 50.0)
    vl = 0.03
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl, True)
    vol.integrate(depth, rgb, poses, tsdf_ref.pinhole(60, 80, 50.0))
    plain = vol.extract_mesh()
    same = vol.extract_mesh(min_weight=1, smooth=None)
    assert plain["verts"].shape[0] > 0 and all(torch.equal(plain[k], same[k]) for k in plain) and set(plain) == set(same)
    by_hand = M.smooth(plain, **kw)
    fused = vol.extract_mesh(smooth=kw)
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)
    assert torch.equal(fused["colors"], plain["colors"])
    with pytest.raises(ValueError):
        vol.extract_mesh(smooth="taubin")
