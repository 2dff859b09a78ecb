"""tests/register_ref.py, the numpy statement of point-to-plane registration, pinned on the CPU: its ordered sums against an
exact sum, mutants that the bit tests must notice, the 6x6 solve, degenerate inputs, convergence on the box case and the robust
kernels -- and the argument checks of the C ABI's Section 27, which need no GPU."""
import functools
import math

import numpy as np
import pytest

import eval_ref as E
import p2m_ref as P
import register_ref as R

U = 2.0 ** -53


def _err(T, truth):
    return float(np.abs(T - truth).max())


@functools.lru_cache(maxsize=None)
def _box(outliers=0):
    return R.box_case(outliers)


@functools.lru_cache(maxsize=None)
def _run(mode, max_corr=0.1, kernel="l2", outliers=0):
    c = _box(outliers)
    if mode == "point":
        return E.icp(c["source"], c["target"], max_corr)
    if mode == "cloud":
        return R.icp_point_to_plane(c["source"], c["target"], c["normals"], max_corr, kernel=kernel)
    return R.icp_point_to_plane(c["source"], (c["verts"], c["faces"]), None, max_corr, kernel=kernel)


# ---- the sums ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 257, 4097, 3 * 4096 + 5])
def test_ordered_sums_are_within_the_bound_of_an_exact_sum(n):
    """|ordered - exact| <= m u sum |terms|, m the additions on the longest path: the standard bound of any summation tree"""
    m = R.path_additions(n)
    assert m == 24 + (8 if n > 4096 else 0)
    for args, kernel in ((R.synthetic_cloud(n, seed=1), ("huber", R.K_EXACT)), (R.synthetic_surface(n, seed=2), "l2"),
                         (R.large_coordinate_cloud(n), ("tukey", 1e-5))):
        s = R.plane_system(kernel=kernel, **args)
        for slot in range(30):
            t = s["terms"][:, slot]
            exact = math.fsum(t.tolist())
            assert abs(float(s["sums"][slot]) - exact) <= m * U * math.fsum(np.abs(t).tolist()), (slot, n)


def test_path_additions_of_three_levels():
    assert R.path_additions(4096 * 256 + 1) == 40 and R.path_additions(4096 * 256) == 32


def test_the_order_and_the_rounding_of_r_show_in_the_bits():
    """On rows with coordinates near 1e3 and residuals near 1e-6 a reference that summed in numpy's order, or whose r took one fused
    multiply-add, differs from the stated one in at least one bit: the bit-for-bit tests can notice either."""
    args = R.large_coordinate_cloud(4097)
    rows = R.cloud_rows(**args)
    ref = R.system_from_rows(*rows, "l2")

    def fused(p, q, nrm):
        d = p - q
        two = nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]
        return (two.astype(np.longdouble) + nrm[:, 2].astype(np.longdouble) * d[:, 2].astype(np.longdouble)).astype(np.float64)

    by_np_sum = R.system_from_rows(*rows, "l2", reduce=lambda t: t.sum(0))
    by_fma = R.system_from_rows(*rows, "l2", residual=fused)
    bits = lambda s: s["sums"].view(np.uint64)
    assert (bits(by_np_sum) != bits(ref)).any()
    assert (bits(by_fma) != bits(ref)).any()
    # and neither mutant is far: both are sums of the same rows
    np.testing.assert_allclose(by_np_sum["sums"], ref["sums"], rtol=1e-9, atol=1e-12)


def test_unused_rows_add_plus_zero_and_counts():
    args = R.synthetic_cloud(1000, seed=3)
    s = R.plane_system(kernel="l2", **args)
    idx = args["idx"]
    assert s["k_corr"] == int((idx >= 0).sum())
    assert s["k_used"] == int(((idx >= 0) & (idx != 1) & (idx != 2)).sum())         # targets 1 and 2 carry a zero and a NaN normal
    rows = np.nonzero((idx == 1) | (idx == 2))[0]
    assert len(rows) and not s["terms"][rows, :29].any() and (s["terms"][rows, 29] > 0).all()
    assert not s["terms"][idx < 0].any() and not np.signbit(s["terms"][idx < 0]).any()
    none = R.plane_system(kernel="l2", **R.synthetic_cloud(100, drop="all"))
    assert none["k_corr"] == 0 and not none["sums"].any()


def test_rows_with_r_exactly_k_take_the_inner_branch():
    for args in (R.synthetic_cloud(600, seed=4, drop=None), R.synthetic_surface(600, seed=4, drop=None)):
        rows = R.cloud_rows(**args) if "idx" in args else R.surface_rows(**args)
        r = R.residuals(*rows[:3])
        exact = np.arange(5, 600, 6)
        assert (np.abs(r[exact]) == R.K_EXACT).all() and (r[exact] > 0).any() and (r[exact] < 0).any()
        assert (R.weights(r[exact], ("huber", R.K_EXACT)) == 1.0).all()
        assert (R.weights(r[exact], ("tukey", R.K_EXACT)) == 0.0).all()             # (1 - 1)^2: the inner branch's value at the edge
        assert (np.abs(r) > R.K_EXACT).any() and (np.abs(r) < R.K_EXACT).any()


def test_the_sums_do_not_depend_on_the_side_of_the_normals():
    args = R.synthetic_cloud(500, seed=6)
    flipped = dict(args, normals=-args["normals"])
    a, b = R.plane_system(kernel=("huber", R.K_EXACT), **args), R.plane_system(kernel=("huber", R.K_EXACT), **flipped)
    assert (a["sums"].view(np.uint64) == b["sums"].view(np.uint64)).all()


# ---- the solve --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["cloud", "surface"])
def test_solve_residual_on_the_first_system_of_the_box_case(mode):
    c = _box()
    p = c["source"].astype(np.float64)
    if mode == "cloud":
        d, i = E.nn_brute(c["source"], c["target"], 0.1)
        s = R.plane_system(p, idx=i, dist=d, targets=c["target"], normals=c["normals"])
    else:
        face, d2, closest, _ = P.closest_brute(c["source"], c["verts"], c["faces"])
        s = R.plane_system(p, face_idx=np.where(d2 <= 0.1 * 0.1, face, -1), d2=d2, closest=closest, verts=c["verts"], faces=c["faces"])
    x = R.ldlt_solve(s["A"], s["b"])
    assert x is not None
    A, b, x = s["A"], s["b"], np.array(x)
    exact = [math.fsum([A[i, j] * x[j] for j in range(6)] + [-b[i]]) for i in range(6)]       # (products rounded: 6 u |A||x| more)
    bound = 256 * U * (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max())
    assert max(abs(e) for e in exact) <= bound


def test_update_matrix_is_a_rotation_in_open3d_order():
    x = [0.3, -0.2, 0.5, 1.0, 2.0, 3.0]
    M = R.update_matrix(x)
    rot = lambda ax, a: E.rigid(ax, math.degrees(a), [0, 0, 0])[:3, :3]
    np.testing.assert_allclose(M[:3, :3], rot([0, 0, 1], x[2]) @ rot([0, 1, 0], x[1]) @ rot([1, 0, 0], x[0]), atol=1e-15)
    assert M[:3, 3].tolist() == x[3:] and M[3].tolist() == [0, 0, 0, 1]
    assert np.array_equal(R.update_matrix([0.0] * 6), np.eye(4))
    T = E.rigid([1, 2, 3], 20.0, [0.5, 0.25, -1])
    np.testing.assert_allclose(R.matmul4(M, T), M @ T, atol=1e-15)


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------------

def _planes(which):
    """targets with normals on z = 0 (and on x = 0), the source a slightly moved copy"""
    g = np.random.default_rng(8)
    uv = g.uniform(-1, 1, (600, 2))
    pts = [np.stack([uv[:, 0], uv[:, 1], 0 * uv[:, 0]], 1)]
    nrm = [np.tile([0.0, 0.0, 1.0], (600, 1))]
    if which == 2:
        pts.append(np.stack([0 * uv[:, 0], uv[:, 1], uv[:, 0]], 1))
        nrm.append(np.tile([1.0, 0.0, 0.0], (600, 1)))
    tgt = np.concatenate(pts).astype(np.float32)
    src = E.transform(tgt.astype(np.float64), E.rigid([1.0, 0.5, 0.2], 0.5, [0.004, 0.003, 0.005])).astype(np.float32)
    return src, tgt, np.concatenate(nrm).astype(np.float32)


@pytest.mark.parametrize("which, rank", [(1, 3), (2, 5)])
def test_planes_are_degenerate_at_iteration_zero(which, rank):
    src, tgt, nrm = _planes(which)
    d, i = E.nn_brute(src, tgt, 0.1)
    s = R.plane_system(src.astype(np.float64), idx=i, dist=d, targets=tgt, normals=nrm)
    assert s["k_used"] == len(src)
    assert np.linalg.matrix_rank(s["A"], tol=1e-9 * np.abs(s["A"]).max()) == rank
    assert R.ldlt_solve(s["A"], s["b"]) is None
    out = R.icp_point_to_plane(src, tgt, nrm, 0.1)
    assert out["degenerate"] and out["iterations"] == 0 and np.array_equal(out["transformation"], np.eye(4))
    assert out["fitness"] == 1.0 and out["used"] == len(src)


def test_one_plane_as_a_mesh_is_degenerate_and_the_box_is_not():
    src, _, _ = _planes(1)
    v = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    out = R.icp_point_to_plane(src, (v, f), None, 0.1)
    assert out["degenerate"] and out["iterations"] == 0
    assert not _run("surface")["degenerate"] and not _run("cloud")["degenerate"]
    # no correspondence at all: A = 0, the first pivot is not positive
    far = R.icp_point_to_plane(src + np.float32(50), (v, f), None, 0.1)
    assert far["degenerate"] and far["fitness"] == 0.0 and far["inlier_rmse"] == 0.0 and far["used"] == 0


# ---- convergence on the box case --------------------------------------------------------------------------------------------------

def test_surface_mode_converges_in_six_iterations_below_1e_6():
    out = _run("surface")
    assert out["iterations"] <= 6 and not out["degenerate"]
    assert _err(out["transformation"], _box()["truth"]) < 1e-6
    assert out["fitness"] == 1.0 and out["used"] == 1500


def test_cloud_mode_beats_point_to_point_in_iterations_and_error():
    point, cloud = _run("point"), _run("cloud")
    assert 3 * cloud["iterations"] <= point["iterations"]
    assert _err(cloud["transformation"], _box()["truth"]) < _err(point["transformation"], _box()["truth"])


def test_cloud_mode_converges_with_rows_without_a_correspondence():
    c = _box()
    out = _run("cloud", 0.03)
    d, i = E.nn_brute(c["source"], c["target"], 0.03)
    start = (i >= 0).mean()
    assert 0 < start < 1 and out["fitness"] > start                                     # some rows unmatched at first; more matched at the end
    assert out["iterations"] < 30 and not out["degenerate"]
    assert _err(out["transformation"], c["truth"]) < _err(_run("point", 0.03)["transformation"], c["truth"])


def test_robust_kernels_shed_the_outliers():
    truth = _box(300)["truth"]
    l2 = _err(_run("surface", 0.1, "l2", 300)["transformation"], truth)
    tukey = _err(_run("surface", 0.1, ("tukey", 0.03), 300)["transformation"], truth)
    huber = _err(_run("surface", 0.1, ("huber", 0.01), 300)["transformation"], truth)
    assert 3 * tukey < l2 and 3 * huber < l2, (l2, huber, tukey)


# ---- the C ABI's argument checks --------------------------------------------------------------------------------------------------

def test_argument_checks_need_no_gpu():
    import ctypes
    from nicer_slam_amd._native import EXPORTS, ICP_CLOUD, ICP_SURFACE, lib
    for name in ("nsa_icp_transform", "nsa_icp_plane_system_workspace", "nsa_icp_plane_system"):
        assert name in EXPORTS and hasattr(lib, name)
    BAD = 4
    fake = ctypes.c_void_p(4096)                                                         # never dereferenced
    eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    assert lib.nsa_icp_transform(None, 0, None, None, None) == 0                         # n = 0: nothing to do
    assert lib.nsa_icp_transform(None, 5, eye, fake, None) == BAD
    assert lib.nsa_icp_transform(fake, 5, None, fake, None) == BAD
    assert lib.nsa_icp_transform(fake, 5, eye, None, None) == BAD
    assert lib.nsa_icp_transform(fake, 1 << 31, eye, fake, None) == BAD
    ws = lib.nsa_icp_plane_system_workspace
    assert ws(0) == 0 and ws(1 << 31) == 0
    assert ws(1) == ws(4096) == 2 * 256 and ws(4097) == 3 * 256 and ws(4096 * 256 + 1) == (257 + 2) * 256

    def system(n=5, mode=ICP_CLOUD, kernel=0, k=0.0, cur=fake, corr=fake, cloud=(fake, fake, fake), surface=(fake, fake, fake, fake),
               work=fake, sums=fake, counts=fake):
        return lib.nsa_icp_plane_system(cur, n, mode, corr, cloud[0], cloud[1], cloud[2], 10, surface[0], surface[1], surface[2], 10,
                                        surface[3], 10, kernel, k, work, sums, counts, None)
    assert system(n=0, cur=None, corr=None, work=None, sums=None, counts=None) == 0      # n = 0: nothing to do
    assert system(n=1 << 31) == BAD
    assert system(mode=2) == BAD and system(kernel=3) == BAD and system(kernel=-1) == BAD
    assert system(kernel=1, k=0.0) == BAD and system(kernel=2, k=float("nan")) == BAD and system(kernel=2, k=float("inf")) == BAD
    for key in ("cur", "corr", "work", "sums", "counts"):
        assert system(**{key: None}) == BAD, key
    for i in range(3):
        assert system(cloud=tuple(None if j == i else fake for j in range(3))) == BAD
    for i in range(4):
        assert system(mode=ICP_SURFACE, surface=tuple(None if j == i else fake for j in range(4))) == BAD
    assert system(n=0, kernel=7) == BAD                                                  # the codes are checked first


def test_kernel_specs_and_host_step_of_the_package_equal_the_reference():
    from nicer_slam_amd import mesh_register as M
    assert M._kernel("l2") == (0, 0.0) and M._kernel(("huber", 0.5)) == (1, 0.5) and M._kernel(("tukey", 2)) == (2, 2.0)
    for bad in ("huber", ("tukey", 0), ("huber", float("nan")), ("cauchy", 1.0), None):
        with pytest.raises(ValueError):
            M._kernel(bad)
    s = R.plane_system(kernel="l2", **R.synthetic_cloud(2000, seed=9))
    x = M.ldlt_solve(s["A"], s["b"])
    assert x == R.ldlt_solve(s["A"], s["b"])
    assert np.array_equal(M.update_matrix(x), R.update_matrix(x))
    T = E.rigid([1, 2, 3], 20.0, [0.5, 0.25, -1])
    assert np.array_equal(M._matmul4(M.update_matrix(x), T), R.matmul4(R.update_matrix(x), T))
    assert M.ldlt_solve(np.zeros((6, 6)), np.zeros(6)) is None
