"""k nearest neighbours and cloud normals on the device (csrc/mesh_eval.hip k_nn_query_k, csrc/cloud_normals.hip,
nicer_slam_amd/cloud_normals.py) against the numpy statement in tests/normals_ref.py: idx, dist and count bit for bit at every
list capacity and its edges, normals, eigenvalues and validity bit for bit, and point-to-plane ICP on estimated normals without a
tolerance.  Above 4096 queries the brute reference answers a strided subset."""
import functools
import math

import numpy as np
import pytest
import torch

import eval_ref as E
import normals_ref as N
import register_ref as R

pytestmark = pytest.mark.gpu

KS = [1, 2, 8, 9, 30, 63, 64]                            # the capacities 8 / 16 / 32 / 64 and their edges


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _assert_knn(got, ref, what, rows=None):
    dist, idx, count = (x.cpu().numpy() for x in got)
    if rows is not None:
        dist, idx, count = dist[rows], idx[rows], count[rows]
    assert dist.dtype == np.float32 and idx.dtype == np.int64 and count.dtype == np.int64
    assert np.array_equal(count, ref[2]), (what, np.nonzero(count != ref[2])[0][:5])
    assert np.array_equal(idx, ref[1]), (what, np.nonzero((idx != ref[1]).any(1))[0][:5])
    nan = np.isnan(ref[0])
    assert np.array_equal(np.isnan(dist), nan) and np.array_equal(dist.view(np.uint32)[~nan], ref[0].view(np.uint32)[~nan]), what


@functools.lru_cache(maxsize=None)
def _uniform(n):
    from nicer_slam_amd.mesh_eval import NNIndex
    t, q = N.uniform(n, seed=n), N.uniform_queries(n, seed=n)
    rows = np.arange(0, len(q), -(-len(q) // 4096))
    return NNIndex(_cuda(t)), _cuda(q), rows, N.knn_brute(q[rows], t, 64)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [1, 7, 1000, 20000])
def test_knn_on_uniform_clouds(n, k):
    """queries: the cloud itself and 300 points of a larger box; k > n pads"""
    index, q, rows, ref64 = _uniform(n)
    _assert_knn(index.knn(q, k), N.knn_prefix(ref64, k), (n, k), rows)


def test_knn_on_the_lattice_breaks_every_tie_to_the_lower_index():
    from nicer_slam_amd.mesh_eval import NNIndex
    t, q = N.lattice_case()
    index, ref64 = NNIndex(_cuda(t)), N.knn_brute(q, t, 64)
    assert (np.diff(ref64[0], axis=1) == 0).mean() > 0.5                                # ties everywhere
    for k in KS:
        _assert_knn(index.knn(_cuda(q), k), N.knn_prefix(ref64, k), k)
        assert (ref64[0][:, k - 1] == ref64[0][:, min(k, 63)]).any()                    # and across the k-th place


def test_knn_of_identical_targets():
    """the grid's worst case: every target in one cell"""
    from nicer_slam_amd.mesh_eval import nearest_k
    t = np.tile(np.float32([[0.25, -0.5, 0.125]]), (300, 1))
    q = np.float32([[0.25, -0.5, 0.125], [1, 1, 1]])
    dist, idx, count = nearest_k(_cuda(q), _cuda(t), 64)
    assert idx.cpu().tolist() == [list(range(64))] * 2 and count.cpu().tolist() == [64, 64]
    _assert_knn((dist, idx, count), N.knn_brute(q, t, 64), "identical")


def test_knn_ring_walk_ends_with_an_outlier_and_far_queries():
    from nicer_slam_amd.mesh_eval import NNIndex
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.normal(0, 1e-3, (500, 3)), [[40.0, -30.0, 25.0]]]).astype(np.float32)
    q = np.concatenate([t[::50], rng.uniform(-100, 100, (60, 3)), [[1e6, 1e6, -1e6], [40, -30, 25.001]]]).astype(np.float32)
    index = NNIndex(_cuda(t))
    for k in (1, 8, 30, 64):
        _assert_knn(index.knn(_cuda(q), k), N.knn_brute(q, t, k), k)
    few = np.float32([[0, 0, 0], [5, 5, 5], [np.nan, 0, 0], [0, 1, 0]])                # fewer than k finite targets in total
    _assert_knn(NNIndex(_cuda(few)).knn(_cuda(q), 9), N.knn_brute(q, few, 9), "few")


def test_knn_with_non_finite_targets_and_queries():
    from nicer_slam_amd.mesh_eval import NNIndex
    t, q = N.uniform(1000, seed=5).copy(), N.uniform_queries(1000, seed=5).copy()
    t[::7, 1] = np.nan
    t[3::11, 0] = np.inf
    t[5::13, 2] = -np.inf
    q[::9, 2] = np.nan
    q[4::17, 0] = np.inf
    index = NNIndex(_cuda(t))
    for k in (1, 9, 64):
        ref = N.knn_brute(q, t, k)
        got = index.knn(_cuda(q), k)
        _assert_knn(got, ref, k)
        assert np.isfinite(t[ref[1][ref[1] >= 0]]).all() and (ref[2][::9] == 0).all()
    none = NNIndex(_cuda(np.full((5, 3), np.nan, np.float32))).knn(_cuda(q), 4)
    assert (none[1] == -1).all() and (none[2] == 0).all() and torch.isinf(none[0][1]).all() and torch.isnan(none[0][0]).all()


def test_knn_within_a_radius():
    """most queries find fewer than k; a target at exactly d2 == fp32(max_dist^2) is not accepted"""
    from nicer_slam_amd.mesh_eval import NNIndex
    t = np.concatenate([N.uniform(1000, seed=8), np.float32([[0.25, 0, 0], [0, 0, 0.125]])])
    q = np.concatenate([N.uniform_queries(1000, seed=8), np.float32([[0, 0, 0]])])
    index = NNIndex(_cuda(t))
    for k in (1, 8, 30, 64):
        ref = N.knn_brute(q, t, k, 0.25)
        _assert_knn(index.knn(_cuda(q), k, 0.25), ref, k)
    assert (ref[2] < 64).mean() > 0.9 and (ref[2] == 0).any()
    assert 1001 in ref[1][-1] and 1000 not in ref[1][-1]


def test_knn_k_1_is_query_and_answers_are_repeatable():
    from nicer_slam_amd.mesh_eval import NNIndex
    t, q = N.lattice_case()
    t = np.concatenate([t, N.uniform(3000, seed=2) * 4 + 4])
    q = np.concatenate([q, N.uniform_queries(3000, seed=2) * 4 + 4])
    q[5] = np.nan
    index = NNIndex(_cuda(t))
    for radius in (math.inf, 0.3):
        d1, i1 = index.query(_cuda(q), radius)
        dk, ik, ck = index.knn(_cuda(q), 1, radius)
        assert torch.equal(ik[:, 0], i1) and torch.equal(dk[:, 0].view(torch.int32), d1.view(torch.int32)) and torch.equal(ck, (i1 >= 0).long())
    a, b, c = index.knn(_cuda(q), 30), index.knn(_cuda(q), 30), NNIndex(_cuda(t)).knn(_cuda(q), 30)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, z.view(torch.int32) if z.dtype == torch.float32 else z)


def test_knn_arguments():
    from nicer_slam_amd.mesh_eval import NNIndex
    index = NNIndex(_cuda(N.uniform(10)))
    q = _cuda(N.uniform(4))
    for k in (0, 65, 2.0):
        with pytest.raises(ValueError):
            index.knn(q, k)
    with pytest.raises(ValueError):
        index.knn(q, 3, max_dist=0.0)
    with pytest.raises(ValueError):
        index.knn(q.cpu(), 3)
    dist, idx, count = index.knn(q[:0], 3)
    assert dist.shape == (0, 3) and idx.shape == (0, 3) and count.shape == (0,)


# ---- normals ------------------------------------------------------------------------------------------------------------------------

def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_normals(points, k=30, max_dist=math.inf, viewpoint=None, queries=None, subset=4096):
    """device against reference; returns the reference's (normals, info) for further conditions"""
    from nicer_slam_amd.cloud_normals import estimate_normals
    got, info = estimate_normals(_cuda(points), k, max_dist, None if viewpoint is None else _cuda(np.asarray(viewpoint, np.float32)),
                                 None if queries is None else _cuda(queries), info=True)
    ref, ref_info = N.estimate_normals(points, k, max_dist, viewpoint, queries)
    got = got.cpu().numpy()
    info = {key: v.cpu().numpy() for key, v in info.items()}
    assert got.dtype == np.float32 and info["eigenvalues"].dtype == np.float64 and info["valid"].dtype == bool
    assert np.array_equal(info["idx"], ref_info["idx"]) and np.array_equal(info["count"], ref_info["count"])
    q = points if queries is None else queries
    own = N.normals_from(points, info["idx"], info["count"], q, viewpoint)              # the reference fed the device's own idx
    for r_n, r_w, r_v in ((ref, ref_info["eigenvalues"], ref_info["valid"]), (own["normals"], own["eigenvalues"], own["valid"])):
        assert np.array_equal(info["valid"], r_v)
        assert _bits_equal(got, r_n), np.nonzero((got.view(np.uint32) != r_n.view(np.uint32)).any(1))[0][:5]
        assert _bits_equal(info["eigenvalues"], r_w), np.nonzero((info["eigenvalues"].view(np.uint64) != r_w.view(np.uint64)).any(1))[0][:5]
    nan = np.isnan(ref_info["variation"])                                                # (0 / 0: the sign of that NaN is the platform's)
    assert np.array_equal(np.isnan(info["variation"]), nan) and _bits_equal(info["variation"][~nan], ref_info["variation"][~nan])
    return ref, ref_info


def test_normals_of_a_noisy_plane_and_the_plane_at_1000():
    for offset in (0.0, 1000.0):
        p = N.noisy_plane(2000, offset=offset)
        ref, info = _check_normals(p)
        assert info["valid"].all() and (np.abs(ref.astype(np.float64) @ ref[0].astype(np.float64)) > 0.99).all()
        assert np.median(info["variation"]) < (1e-3 if offset == 0.0 else 2e-3)
        lengths = np.linalg.norm(ref.astype(np.float64), axis=1)
        assert np.abs(lengths - 1).max() < 2e-7


def test_normals_of_a_sphere_with_and_without_viewpoints():
    p = N.sphere(2000)
    centre = np.float32([0.2, -0.1, 0.3])
    radial = (p - centre).astype(np.float64)
    ref, info = _check_normals(p, 16)
    assert info["valid"].all() and (np.abs((ref * radial).sum(1)) > 0.97).all()
    big = np.abs(ref).argmax(1)
    assert (np.take_along_axis(ref, big[:, None], 1) > 0).all()                         # without a viewpoint: the largest component positive
    ref, info = _check_normals(p, 16, viewpoint=centre + np.float32([0.1, 0.2, -0.1]))   # one viewpoint inside the sphere: all inward
    w = (centre + np.float32([0.1, 0.2, -0.1])).astype(np.float64)
    assert ((ref.astype(np.float64) * (w - p.astype(np.float64))).sum(1) >= 0).all() and ((ref * radial).sum(1) < 0).all()
    per_point = (p.astype(np.float64) + 0.5 * radial).astype(np.float32)                 # per-point viewpoints outside: all outward
    ref, info = _check_normals(p, 16, viewpoint=per_point)
    assert ((ref * radial).sum(1) > 0).all()


def test_normals_of_exact_planes_lines_and_duplicates():
    g = np.arange(12, dtype=np.float32)
    plane = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    plane = np.concatenate([plane * np.float32(0.25), np.full((144, 1), np.float32(3.5))], 1)       # an exactly planar lattice
    ref, info = _check_normals(plane, 9)
    assert info["valid"].all() and (info["eigenvalues"][:, 0] == 0.0).all() and (ref == np.float32([0, 0, 1])).all()
    line = np.float32([0.5, -0.25, 0.125]) + np.outer(np.arange(40, dtype=np.float32), np.float32([0.25, 0, 0]))
    ref, info = _check_normals(line, 8)                                                  # collinear along an axis: w1 == 0 exactly
    assert not info["valid"].any() and not ref.any() and (info["eigenvalues"][:, 1] == 0.0).all()
    skew = (np.float32([0.5, -0.25, 0.125]) + np.outer(np.arange(40, dtype=np.float32), np.float32([0.25, 0.5, -0.125]))).astype(np.float32)
    _check_normals(skew, 8)                                                              # a general line: whatever the reference says
    dup = np.concatenate([np.tile(np.float32([[1, 2, 3]]), (40, 1)), N.uniform(50, seed=4)])
    ref, info = _check_normals(dup, 16)
    assert not info["valid"][:40].any() and not ref[:40].any() and (info["eigenvalues"][:40] == 0.0).all()


def test_normals_under_a_radius_and_off_the_cloud():
    p = N.uniform(1500, seed=6)
    ref, info = _check_normals(p, 30, max_dist=0.12)
    few = info["count"] < 3
    assert few.any() and (~few).any() and not info["valid"][few].any() and not ref[few].any()
    q = np.concatenate([N.uniform(300, seed=7) * np.float32(1.5), [[np.nan, 0, 0], [50, 50, 50]]]).astype(np.float32)
    ref, info = _check_normals(N.sphere(1500, seed=2), 12, queries=q, viewpoint=np.float32([0.2, -0.1, 0.3]))
    assert info["count"][-2] == 0 and not info["valid"][-2] and np.isnan(info["eigenvalues"][-2]).all()
    ref, info = _check_normals(N.noisy_plane(300), 64, queries=q)
    ref, info = _check_normals(N.uniform(2, seed=1), 5)                                  # a cloud smaller than 3 points
    assert not info["valid"].any()


def test_normals_arguments_and_a_prebuilt_index():
    from nicer_slam_amd.cloud_normals import estimate_normals
    from nicer_slam_amd.mesh_eval import NNIndex
    p = _cuda(N.sphere(500))
    a = estimate_normals(p, 10)
    b = estimate_normals(p.cpu().numpy(), 10, index=NNIndex(p))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        estimate_normals(p, 0)
    with pytest.raises(ValueError):
        estimate_normals(p, 10, viewpoint=torch.zeros(7, 3))
    with pytest.raises(ValueError):
        estimate_normals(p, 10, index=NNIndex(p[:100]))
    with pytest.raises(ValueError):
        estimate_normals(p[:0], 10)


# ---- where it plugs in --------------------------------------------------------------------------------------------------------------

def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_icp_on_estimated_normals_equals_the_reference_and_stays_near_the_true_normals():
    """register_ref.box_case(), max_corr 0.1, k = 30 (the default; not tuned).  Measured with the two references alone, max |T - truth|:
    5.46e-4 with the box's true face normals (4 iterations), 8.23e-4 with estimated normals (5 iterations): 32 % of the 4000 targets have
    a neighbourhood that straddles an edge of the box and a normal more than 8 degrees off the face's.  Margin: twice the error of the run
    with true normals (the measured ratio is 1.51)."""
    from nicer_slam_amd.mesh_register import icp_point_to_plane
    c = R.box_case()
    est, _ = N.estimate_normals(c["target"], 30)
    ref = R.icp_point_to_plane(c["source"], c["target"], est, 0.1)
    true = R.icp_point_to_plane(c["source"], c["target"], c["normals"], 0.1)
    got = icp_point_to_plane(_cuda(c["source"]), _cuda(c["target"]), "estimate", 0.1)
    for key in ("iterations", "fitness", "inlier_rmse", "residual_rmse", "used", "degenerate"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert np.array_equal(_bits(got["transformation"]), _bits(ref["transformation"]))
    err = lambda r: np.abs(r["transformation"] - c["truth"]).max()
    print("max |T - truth|: true normals", err(true), "estimated", err(ref), "device", err(got))
    assert err(got) <= 2 * err(true)
    # the dict form, a viewpoint (the sums do not depend on the normals' side) and a prebuilt index
    from nicer_slam_amd.mesh_eval import NNIndex
    again = icp_point_to_plane(_cuda(c["source"]), _cuda(c["target"]), dict(k=30, viewpoint=[0.0, 0.0, 0.0]), 0.1, index=NNIndex(_cuda(c["target"])))
    assert np.array_equal(_bits(again["transformation"]), _bits(ref["transformation"]))
    other = icp_point_to_plane(_cuda(c["source"]), _cuda(c["target"]), dict(k=12, max_dist=0.2), 0.1)
    est12, _ = N.estimate_normals(c["target"], 12, 0.2)
    assert np.array_equal(_bits(other["transformation"]), _bits(R.icp_point_to_plane(c["source"], c["target"], est12, 0.1)["transformation"]))
    # the paths that were there stay as they were
    given = icp_point_to_plane(_cuda(c["source"]), _cuda(c["target"]), _cuda(c["normals"]), 0.1)
    assert np.array_equal(_bits(given["transformation"]), _bits(true["transformation"]))
    with pytest.raises(ValueError, match="needs normals"):
        icp_point_to_plane(_cuda(c["source"]), _cuda(c["target"]), None, 0.1)
    with pytest.raises(ValueError):
        icp_point_to_plane(_cuda(c["source"]), _cuda(c["target"]), "guess", 0.1)
    with pytest.raises(ValueError):
        icp_point_to_plane(_cuda(c["source"]), _cuda(c["target"]), dict(neighbours=3), 0.1)


def _write_cloud(path, points):
    """a PLY that is only points: no face element"""
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(points)}", "property float x", "property float y",
            "property float z", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(np.ascontiguousarray(points, "<f4").tobytes())


def test_command_lines_round_trip_a_faceless_ply(tmp_path, capsys):
    import json
    from nicer_slam_amd import cloud_normals, inference, mesh_register
    c = R.box_case()
    _write_cloud(tmp_path / "cloud.ply", c["target"])
    r = cloud_normals.main([str(tmp_path / "cloud.ply"), "--out", str(tmp_path / "out.ply"), "--k", "12", "--viewpoint", "0", "0", "0", "--json"])
    printed = json.loads(capsys.readouterr().out)
    assert printed == r and r["points"] == 4000 and r["valid"] == 4000 and r["k"] == 12
    back = inference.read_ply(str(tmp_path / "out.ply"))
    ref, _ = N.estimate_normals(c["target"], 12, viewpoint=np.zeros(3, np.float32))
    assert _bits_equal(back["verts"], c["target"]) and _bits_equal(back["normals"], ref) and back["faces"].shape == (0, 3)
    _write_cloud(tmp_path / "src.ply", c["source"])
    out = mesh_register.main([str(tmp_path / "src.ply"), str(tmp_path / "cloud.ply"), "--estimate-normals", "--json"])
    printed = json.loads(capsys.readouterr().out)
    est, _ = N.estimate_normals(c["target"], 30)
    assert np.array_equal(_bits(out["transformation"]), _bits(R.icp_point_to_plane(c["source"], c["target"], est, 0.1)["transformation"]))
    assert printed["iterations"] == out["iterations"]
    with pytest.raises(SystemExit):
        cloud_normals.main([str(tmp_path / "cloud.ply"), "--out", str(tmp_path / "bad.ply"), "--k", "65"])
