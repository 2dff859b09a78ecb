"""Self-intersections on the device (header Section 25, csrc/mesh_intersect.hip) against the rational statement of
tests/intersect_ref.py: pairs, codes, flags, the candidate count and its split by shared positions element for element; the tree walk
equal to the on-device brute force; a second run byte-identical.  Then the public interface, the other tools' opt-in keywords, the
command line with a PLY round trip and the argument checks.  No tolerance takes part anywhere."""
import functools
import json

import numpy as np
import pytest
import torch

import intersect_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    """(mesh, reference answer), computed once per module"""
    if name == "known":
        mesh = R.known_mesh()
    elif name == "lattice":
        mesh = R.lattice_soup()
    elif name == "lattice, offset":
        mesh = R.lattice_soup(40, 5, (3.25, -1.5, 100.0))
    elif name == "random 600":
        mesh = R.random_soup(600, 7)
    elif name == "spheres":
        mesh = R.two_spheres(10)[0]
    elif name.startswith("count "):
        mesh = R.random_soup(int(name.split()[1]), 21)
    elif name == "coincident centroids":
        rng = np.random.default_rng(5)
        d = rng.integers(-8, 9, (40, 2, 3)).astype(np.float32) / 8
        mesh = R.concat([np.stack([u, w, -u - w]) for u, w in d if np.any(np.cross(u, w) != 0)])
    elif name == "unusable faces":
        soup = R.random_soup(30, 9)
        v = np.concatenate([soup["verts"], R.collinear_case(), [[np.nan, 0, 0], [np.inf, 1, 1], [2.0 ** -120, 0, 0], [1, 0, 0], [0, 1, 0]]])
        v = v.astype(np.float32)
        n = len(soup["verts"])
        extra = [[n, n + 1, n + 2], [0, 1, n + 3], [2, n + 4, 3], [0, 1, 500], [-1, 2, 3], [4, 4, 5], [0, 1, 1],
                 [n + 5, n + 6, n + 7], [6, 7, 8]]                           # the last but one spans 120 binades: state 5
        mesh = dict(verts=v, faces=np.concatenate([soup["faces"][:10], extra, soup["faces"][10:]]).astype(np.int32))
    else:
        raise KeyError(name)
    return mesh, R.self_intersections(mesh["verts"], mesh["faces"])


def _run(mesh, **kw):
    from nicer_slam_amd import mesh_intersect as M
    out = M.self_intersections(mesh, return_report=True, **kw)
    torch.cuda.synchronize()
    return out


def _check(name, between=None):
    mesh, ref = _case(name)
    if between is not None:
        ref = R.self_intersections(mesh["verts"], mesh["faces"], between=between)
    pairs, code, flags, rep = _run(mesh, between=between)
    print(f"{name}: F {len(mesh['faces'])} {rep}")
    assert pairs.dtype == np.int64 and code.dtype == np.uint8 and flags.dtype == np.uint8 and flags.shape == (len(mesh["faces"]),)
    assert pairs.tolist() == ref["pairs"].tolist()
    assert code.tolist() == ref["code"].tolist()
    assert flags.tolist() == ref["flags"].tolist()
    assert rep["n_candidates"] == ref["n_candidates"] and rep["n_candidates_s"] == ref["n_candidates_s"]
    assert list(rep["n_skipped"].values()) == ref["n_skipped"]
    assert (rep["n_proper"], rep["n_touch"]) == (ref["n_proper"], ref["n_touch"])
    assert rep["n_stage1"] + rep["n_exact"] + rep["n_host"] == rep["n_candidates"]
    again = _run(mesh, between=between)
    brute = _run(mesh, between=between, brute=True)
    for other in (again, brute):
        assert all(x.tobytes() == y.tobytes() for x, y in zip((pairs, code, flags), other[:3])) and other[3] == rep
    return rep, ref


@pytest.mark.parametrize("name", ["known", "lattice", "lattice, offset", "coincident centroids", "unusable faces"])
def test_degenerate_meshes_equal_the_reference(name):
    rep, ref = _check(name)
    if name == "known":
        assert rep["n_host"] >= 1 and rep["n_exact"] > 10
    if name == "unusable faces":
        assert ref["n_skipped"] == [2, 2, 2, 1] and rep["n_host"] >= 1
    if name == "coincident centroids":
        assert rep["n_candidates"] > 500


def test_random_soup_is_decided_by_the_filter_alone():
    """generic position: a filter that gives up too often, or an exact stage that hides a broken filter, shows here"""
    rep, ref = _check("random 600")
    assert rep["n_exact"] == 0 and rep["n_host"] == 0 and rep["n_stage1"] == rep["n_candidates"] > 1500 and ref["n_proper"] > 100


def test_two_marching_cubes_spheres():
    mesh, ref = _case("spheres")
    rep, _ = _check("spheres")
    assert rep["n_host"] == 0 and ref["n_proper"] > 20 and min(rep["n_candidates_s"][:3]) > 100
    # the share of candidates that reach the exact stage (recorded in DESIGN 4x, not capped)
    print(f"spheres: {rep['n_exact']} of {rep['n_candidates']} candidates went to the exact stage")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 513])
def test_face_counts(n):
    _check(f"count {n}")


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_face_counts_at_the_seams_of_the_scans(n):
    """F just below, at and just above the 1024 lanes of the one workgroup that scans the tree's node counts (F + 1 items) and the
    records per face (F items; csrc/block_scan.hpp): the walk over the tree against the on-device brute force, byte for byte"""
    mesh = R.random_soup(n, 21)
    pairs, code, flags, rep = _run(mesh)
    brute = _run(mesh, brute=True)
    assert rep["n_candidates"] > n and len(pairs) > 100 and len(np.unique(pairs, axis=0)) == len(pairs)
    assert (pairs[:, 0] < pairs[:, 1]).all() and pairs.min() >= 0 and pairs.max() < n and (code != 0).all()
    assert all(x.tobytes() == y.tobytes() for x, y in zip((pairs, code, flags), brute[:3])) and brute[3] == rep


def test_between():
    mesh, _ = _case("lattice")
    mask = np.arange(len(mesh["faces"])) % 3 == 0
    rep, ref = _check("lattice", between=mask)
    assert 0 < ref["n_candidates"] < _case("lattice")[1]["n_candidates"]
    spheres, n_first = R.two_spheres(10)
    mask = np.arange(len(spheres["faces"])) < n_first
    from nicer_slam_amd import mesh_intersect as M
    pairs, code, _ = M.self_intersections({k: torch.from_numpy(x).cuda() for k, x in spheres.items()}, between=torch.from_numpy(mask).cuda())
    full = _case("spheres")[1]
    keep = mask[full["pairs"][:, 0]] != mask[full["pairs"][:, 1]]
    assert pairs.is_cuda and pairs.cpu().tolist() == full["pairs"][keep].tolist() and code.cpu().tolist() == full["code"][keep].tolist()


def test_kinds_index_and_is_embedded():
    from nicer_slam_amd import mesh_intersect as M
    from nicer_slam_amd.mesh_eval import TriIndex
    mesh, ref = _case("lattice")
    kind = ref["code"] & 3
    for kinds, k in ((("proper",), R.PROPER), ("touch", R.TOUCH)):
        pairs, code, flags = M.self_intersections(mesh, kinds=kinds)
        assert pairs.tolist() == ref["pairs"][kind == k].tolist() and code.tolist() == ref["code"][kind == k].tolist()
        want = np.zeros(len(flags), np.uint8)
        want[ref["pairs"][kind == k].reshape(-1)] = k
        assert flags.tolist() == want.tolist()
    ix = TriIndex(torch.from_numpy(mesh["verts"]).cuda(), torch.from_numpy(mesh["faces"]).cuda())
    pairs, code, flags, rep = ix.self_intersections(return_report=True)
    assert pairs.is_cuda and pairs.cpu().tolist() == ref["pairs"].tolist() and rep["n_candidates"] == ref["n_candidates"]
    assert not M.is_embedded(mesh) and not M.is_embedded(ix)
    tetra = dict(verts=np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32),
                 faces=np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], np.int32))
    assert M.is_embedded(tetra)
    empty = M.self_intersections(dict(verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32)), return_report=True)
    assert empty[0].shape == (0, 2) and empty[3]["n_candidates"] == 0


def _sphere(n):
    from nicer_slam_amd import inference
    g = torch.linspace(-1, 1, n, device="cuda")
    X, Y, Z = torch.meshgrid(g, g, g, indexing="ij")
    h = 2.0 / (n - 1)
    return inference.marching_cubes((torch.sqrt(X * X + Y * Y + Z * Z) - 0.8173).float().contiguous(), 0.0, (h, h, h), (-1.0, -1.0, -1.0))


def test_sphere_before_and_after_decimate_and_smooth():
    """whatever the tools do to embeddedness is a finding; the assertion is agreement with the reference on a sub-mesh"""
    from nicer_slam_amd import mesh_decimate, mesh_intersect as M, mesh_smooth
    m0 = _sphere(32)
    m1 = mesh_decimate.decimate(m0, target_faces=m0["faces"].shape[0] // 2)     # (a target is required; the rest are the defaults)
    m2 = mesh_smooth.smooth(m1)
    for name, m in (("sphere 32^3", m0), ("decimated", m1), ("decimated and smoothed", m2)):
        pairs, code, flags, rep = M.self_intersections(m, return_report=True)
        print(f"{name}: faces {m['faces'].shape[0]} embedded {rep['n_proper'] == 0} {rep}")
        assert M.is_embedded(m) == (rep["n_proper"] == 0)
        sub = dict(verts=m["verts"].cpu().numpy(), faces=m["faces"][:260].cpu().numpy())
        ref = R.self_intersections(sub["verts"], sub["faces"])
        p, c, _, r = M.self_intersections(sub, return_report=True)
        assert p.tolist() == ref["pairs"].tolist() and c.tolist() == ref["code"].tolist() and r["n_candidates_s"] == ref["n_candidates_s"]
        inside = (pairs < 260).all(1).cpu().numpy()
        assert pairs.cpu().numpy()[inside].tolist() == ref["pairs"].tolist()


def _cut_box():
    """a unit box with the corner (1, 1, 1) cut off, the cut left open, and a lone triangle through the opening"""
    v = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (0.5, 1, 1), (1, 0.5, 1), (1, 1, 0.5),
         (0.9, 0.9, 0.6), (0.8, 0.8, 1.4), (1.3, 1.2, 1.3)]
    f = [(0, 2, 3), (0, 3, 1), (0, 1, 5), (0, 5, 4), (0, 4, 6), (0, 6, 2),
         (4, 5, 8), (4, 8, 7), (4, 7, 6), (1, 3, 9), (1, 9, 8), (1, 8, 5), (2, 6, 7), (2, 7, 9), (2, 9, 3), (10, 11, 12)]
    return dict(verts=np.array(v, np.float32), faces=np.array(f, np.int32))


def test_fill_holes_reports_patches_that_cross_the_mesh():
    from nicer_slam_amd import mesh_fill
    mesh = _cut_box()
    plain = mesh_fill.fill_holes(mesh, method="min_area", normals="none")
    out, rep = mesh_fill.fill_holes(mesh, method="min_area", normals="none", return_report=True, intersections="report")
    assert all(out[k].tobytes() == plain[k].tobytes() for k in ("verts", "faces"))      # the mesh is not changed by it
    ref = R.self_intersections(out["verts"], out["faces"])
    F = len(mesh["faces"])
    assert len(out["faces"]) == F + 2 and len(rep["proper_pairs"]) == len(rep["n"]) == 2
    proper = ref["pairs"][(ref["code"] & 3) == R.PROPER]
    want = []
    for l in range(2):
        face = F + rep["area_face_offset"][l]
        want.append(int((proper == face).any(1).sum()))                      # a patch of one face: every pair that names it
    print("cut box:", rep["proper_pairs"], proper.tolist())
    assert rep["proper_pairs"] == want and sum(want) >= 2
    with pytest.raises(ValueError):
        mesh_fill.fill_holes(mesh, intersections="report")
    with pytest.raises(ValueError):
        mesh_fill.fill_holes(mesh, intersections="yes", return_report=True)


def test_topology_keyword_and_command_lines(tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_intersect as M, mesh_topology
    mesh, ref = _case("lattice")
    plain = mesh_topology.topology(mesh)
    r = mesh_topology.topology(mesh, intersections=True)
    assert {k: r[k] for k in plain} == plain and r["n_proper_pairs"] == ref["n_proper"] and r["embedded"] is False
    src, dst, npy = str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), str(tmp_path / "pairs.npy")
    inference.write_ply(src, dict(verts=torch.from_numpy(mesh["verts"]), faces=torch.from_numpy(mesh["faces"]),
                                  normals=torch.zeros(len(mesh["verts"]), 3)))
    t = M.main([src, "--json", "--out", dst, "--pairs", npy])
    assert json.loads(capsys.readouterr().out) == t
    assert (t["n_proper"], t["n_touch"], t["n_candidates"], t["embedded"]) == (ref["n_proper"], ref["n_touch"], ref["n_candidates"], False)
    saved = np.load(npy)
    assert saved[:, :2].tolist() == ref["pairs"].tolist() and saved[:, 2].tolist() == ref["code"].tolist()
    back = inference.read_ply(dst)
    assert (back["verts"] == mesh["verts"]).all() and (back["faces"] == mesh["faces"]).all()
    red = (back["colors"] == np.array([1, 0, 0], np.float32)).all(1)
    assert red[mesh["faces"][(ref["flags"] & 1) != 0].reshape(-1)].all() and red.sum() == 3 * int(((ref["flags"] & 1) != 0).sum())
    t = M.main([src, "--kinds", "touch", "--brute"])
    assert "NOT embedded" in capsys.readouterr().out and t["n_returned"] == ref["n_touch"]
    r = mesh_topology.main([src, "--intersections", "--json"])
    assert json.loads(capsys.readouterr().out)["n_proper_pairs"] == ref["n_proper"] == r["n_proper_pairs"]
    with pytest.raises(SystemExit):
        M.main([src, "--kinds", "some"])
    capsys.readouterr()


def test_argument_checks():
    from nicer_slam_amd import mesh_intersect as M
    from nicer_slam_amd._native import lib
    mesh, _ = _case("lattice")
    F = len(mesh["faces"])
    for bad in (np.zeros(F - 1, bool), np.zeros((F, 1), bool), np.zeros(F, np.float32)):
        with pytest.raises(ValueError):
            M.self_intersections(mesh, between=bad)
    with pytest.raises(ValueError):
        M.self_intersections(mesh, kinds=("crossing",))
    x = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = x.data_ptr()
    assert lib.nsa_tri_isect_workspace(0) == 0 and lib.nsa_tri_isect_workspace(1 << 31) == 0 and lib.nsa_tri_isect_workspace(7) > 0
    assert lib.nsa_tri_isect_count(None, None, 0, None, 0, None, 0, None, None, None, None) == 0           # no faces: nothing to do
    assert lib.nsa_tri_isect_emit(None, None, 0, None, 0, None, 0, None, None, 0, None, None, None) == 0
    assert lib.nsa_tri_isect_count(None, p, 3, p, 1, None, 0, p, p, p, None) != 0                             # no tree
    assert lib.nsa_tri_isect_count(p, p, 3, p, 1, None, 2, p, p, p, None) != 0                                # an unknown flag
    assert lib.nsa_tri_isect_count(p, p, 3, p, 1, None, 0, None, p, p, None) != 0                             # no workspace
    assert lib.nsa_tri_isect_count(p, p, 3, p, 1, None, 0, p, None, p, None) != 0
    assert lib.nsa_tri_isect_count(p, p, 0, p, 1, None, 0, p, p, p, None) != 0                                # no vertices
    assert lib.nsa_tri_isect_count(p, p, 3, p, 1 << 31, None, 0, p, p, p, None) != 0
    assert lib.nsa_tri_isect_emit(p, p, 3, p, 1, None, 0, p, p, 1, None, p, None) != 0                        # no pairs array
    assert lib.nsa_tri_isect_emit(p, p, 3, p, 1, None, 0, p, p, 0, None, None, None) == 0                     # nothing to emit
    torch.cuda.synchronize()
    assert int(x.sum()) == 0                                                   # nothing was launched on them
