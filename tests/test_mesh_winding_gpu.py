"""Generalised winding numbers on the GPU (csrc/mesh_winding.hip, header Section 16) against the numpy oracle tests/winding_ref.py:
the exact kernel against the exact sum, the tree kernel against the tree walk with its counts, the classification w > 0.5, and
nicer_slam_amd.mesh_sdf with sign="winding" end to end on a sphere with a hole."""
import functools
import math

import numpy as np
import pytest
import torch

import p2m_ref as P
import sdf_ref as S
import winding_ref as W
from test_mesh_closest_cpu import box_queries, invalid_mesh
from test_mesh_closest_gpu import _cuda, _index, _mc_sphere, _same_bits, _shell_queries
from test_mesh_sdf_gpu import _mc_flip, _mixed_mesh
from test_mesh_winding_cpu import sphere_case

pytestmark = pytest.mark.gpu

# The two sides run the same float64 operations in the same order; +, -, *, / and sqrt are correctly rounded on both, so the tree
# (keys, order, N, M, area, P, r2), det, den and every dipole term carry the same bits.  They differ in atan2 alone: ocml's is within
# 2 ulp and glibc's within 1, so a face's Omega = 2 atan2(det, den) differs by at most 3 ulp(Omega) <= 3 * 2^-52 |Omega|.  With n
# terms added one by one on each side, every partial sum is at most A = the sum of the absolute terms, and each addition rounds by
# at most 2^-53 A on either side: n * 2^-52 A for the two.  The division by 4 pi adds 2^-53 |w| on each side.  In units of w, with
# T = A / 4 pi:
#     |w_gpu - w_ref| <= 2^-52 * (3 T + n T + T) = 2^-52 * (n + 4) * T,   n = accepted + evaluated (F_usable for the exact sum)
W_TOL = 2.0 ** -52
# a decision d2 > beta^2 r2 is compared only where the oracle's relative gap |d2 - beta^2 r2| / d2 exceeds this: the same margin as
# SIGN_MARGIN of tests/test_mesh_sdf_gpu.py, 2^16 times the rounding of d2
GAP_MARGIN = 2.0 ** -36


def _gpu(ix, q, beta, flip=False):
    w, acc, ev = ix.winding(_cuda(q, torch.float32), beta=beta, flip=flip, counts=True)
    return w.cpu().numpy(), acc.cpu().numpy(), ev.cpu().numpy()


def _within(got, ref, what):
    n = ref["accepted"] + ref["evaluated"]
    tol = W_TOL * (n + 4) * ref["abs"]
    nan = np.isnan(ref["w"])
    assert np.array_equal(np.isnan(got), nan), what
    err = np.where(nan, 0.0, np.abs(got - ref["w"]))
    with np.errstate(all="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    print("%s: max |w - w_ref| %.3e, largest share of the tolerance %.3f" % (what, err.max() if err.size else 0.0,
                                                                                  ratio.max() if ratio.size else 0.0))
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, (what, bad[:5], got[bad][:5], ref["w"][bad][:5], tol[bad][:5])


def _check(v, f, q, betas=(2.0,), flip=False, what="", tree=None):
    """index over (v, f): the layout, the exact kernel against the exact oracle and the tree kernel against the tree oracle"""
    ix = _index(v, f)
    tree = tree if tree is not None else W.Tree(v, f)
    lay = ix.winding_layout()
    assert (lay["L"], lay["nodes"], lay["usable faces"]) == (tree.L, tree.n_nodes, tree.n_usable), (what, lay)
    ref = W.exact(q, tree, flip=flip)
    w, acc, ev = _gpu(ix, q, math.inf, flip)
    _within(w, ref, what + ", exact")
    assert np.array_equal(ev, ref["evaluated"]) and (acc == 0).all(), what
    for beta in betas:
        ref = W.walk(q, tree, beta, flip=flip)
        w, acc, ev = _gpu(ix, q, beta, flip)
        sure = ref["gap"] > GAP_MARGIN
        assert (~sure).sum() <= 0.01 * max(len(q), 1), (what, beta, (~sure).sum())
        assert np.array_equal(acc[sure], ref["accepted"][sure]) and np.array_equal(ev[sure], ref["evaluated"][sure]), (what, beta)
        _within(w[sure], {k: x[sure] for k, x in ref.items()}, "%s, beta = %g" % (what, beta))
    return ix, tree


# ---- kernels against the oracle -------------------------------------------------------------------------------------------------

def test_both_boxes():
    q = box_queries()
    v, f = P.box_mesh((-1.5, -1.5, -1.0), (1.5, 1.5, 1.0))
    _check(v, f, q * np.float32([1.5, 3.0, 4.0]), betas=(1.0, 2.0), what="large box")
    v, f = P.box_mesh()
    ix, tree = _check(v, f, q, betas=(2.0, 3.0), what="box")
    assert tree.L == 1 and ix.winding_layout()["bytes"] == ix._winding[0].numel()
    w = _gpu(ix, q, math.inf)[0]
    q64 = q.astype(np.float64)
    lo, hi = np.array([-1.0, -0.5, -0.25]), np.array([1.0, 0.5, 0.25])
    outside = (np.maximum(np.maximum(lo - q64, q64 - hi), 0.0) > 0).any(1)
    inside = ((q64 > lo) & (q64 < hi)).all(1)
    assert np.abs(w[outside]).max() <= 1e-12 and np.abs(w[inside] - 1.0).max() <= 1e-12


def test_spike():
    v, f, apex, _ = S.spike()
    q = (np.random.default_rng(0).standard_normal((257, 3)) * 0.3 + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    q[0] = v[apex]                                                    # on a vertex of 43 faces: det == 0 for every one of them
    _check(v, f, q, betas=(2.0, 3.0), what="spike")


@pytest.mark.parametrize("soup", [False, True])
def test_latlong_sphere_welded_and_as_a_soup(soup):
    v, f, tree, q, ex, walks = sphere_case(False)
    if soup:                                                          # every face with vertices of its own: the same field
        v, f = v[f.reshape(-1)], np.arange(3 * f.shape[0], dtype=np.int32).reshape(-1, 3)
        tree = None
    ix, tree = _check(v, f, q[:513], betas=(2.0,), what="lat-long sphere%s" % (" soup" if soup else ""), tree=tree)
    assert tree.L == 5 and tree.n_usable == 2208


def test_holed_sphere_and_its_motivating_queries():
    v, f, tree, q, ex, walks = sphere_case(True)
    q = np.concatenate([W.HOLE_QUERIES, q[:506]])
    ix, _ = _check(v, f, q, betas=(2.0, 3.0), what="holed sphere", tree=tree)
    _check(v, f, q[:65], betas=(2.0,), flip=True, what="holed sphere, flipped", tree=tree)
    w = _gpu(ix, W.HOLE_QUERIES, math.inf)[0]
    assert (w < 0.5).all() and w[-1] == pytest.approx(0.26, abs=0.005)


def test_open_non_manifold_and_cancelling_meshes():
    rng = np.random.default_rng(21)
    v, f = S.open_square()
    q = np.concatenate([np.array([[0.5, 0.5, -0.5], [0.5, 0.5, 0.5], [0.25, 0.5, 0], [2, 0.5, 0], [0, 0, 0], [1, 1, 0]]),
                        rng.uniform(-1, 2, (251, 3))]).astype(np.float32)
    ix, tree = _check(v, f, q, what="open square")
    assert tree.L == 0 and tree.n_nodes == 1                          # at most 8 faces: the root is the only node
    w = _gpu(ix, q[:6], math.inf)[0]
    assert w[0] == pytest.approx(1 / 6, abs=1e-15) and w[1] == pytest.approx(-1 / 6, abs=1e-15)
    assert (w[2:] == 0.0).all()                                       # in the plane, on it, beside it and on its corners: det == 0
    v, f = S.three_on_an_edge()
    q = np.concatenate([np.array([[0.5, 0, 0], [0.5, 0, -1], [0.5, 0.5, -1]]), rng.uniform(-1, 2, (62, 3))]).astype(np.float32)
    _check(v, f, q, what="three on an edge")
    v, f = W.opposite_twins()
    q = np.concatenate([np.array([[0.25, 0.25, 1], [0.25, 0.25, -1], [-1, -1, 1], [0.5, 0.5, 1e-3]]),
                        rng.uniform(-2, 2, (61, 3))]).astype(np.float32)
    ix, _ = _check(v, f, q, what="opposite twins")
    w = _gpu(ix, q, math.inf)[0]
    # exact in the plane x = y, and elsewhere the oracle's 8 * 2^-53 (both pinned by tests/test_mesh_winding_cpu.py) plus the
    # tolerance above for n = 2 terms of T <= 1
    assert (w[:4] == 0.0).all() and np.abs(w).max() <= 8 * 2.0 ** -53 + 6 * W_TOL


def test_mixed_scales_invalid_faces_and_non_finite_queries():
    v, f = _mixed_mesh()
    rng = np.random.default_rng(8)
    near = _shell_queries(128, 0, 0.5, 9)
    above = np.stack([rng.uniform(-45, 45, 48), rng.uniform(-45, 45, 48), rng.uniform(-3.0, 6.0, 48)], 1)
    stray = np.array([1000.0, 3.0, -2.0]) + rng.uniform(-0.5, 0.5, (32, 3))
    far = np.array([[1e6, 0, 0], [-1e6, 1e6, 0], [0, 0, -1e6], [999, 1e6, -2]])
    nonfinite = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]])
    q = np.concatenate([near, above, stray, far, nonfinite]).astype(np.float32)
    ix, tree = _check(v, f, q, betas=(2.0,), what="mixed scales")
    assert tree.n_usable == f.shape[0] - 7
    w, acc, ev = _gpu(ix, q, 2.0)
    assert np.isnan(w[-4:]).all() and (acc[-4:] == 0).all() and (ev[-4:] == 0).all() and np.isfinite(w[:-4]).all()


def test_marching_cubes_sphere():
    m = _mc_sphere(32)
    flip = _mc_flip(m)
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    q = _shell_queries(320, 192, 0.5, 3)
    ix, tree = _check(v, f, q, betas=(2.0,), flip=flip, what="MC sphere")
    w = _gpu(ix, q, 2.0, flip)[0]
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    assert (w[r > 0.6] < 0.1).all() and (w[r < 0.4] > 0.9).all() and (r < 0.4).sum() > 50


def test_invalid_meshes_one_face_and_one_leaf():
    v, f, totals, good = invalid_mesh()
    q = np.array([[-1, -1, 1], [0.25, 0.25, -1], [2, -1, 0.5], [np.nan, 0, 0], [0, -np.inf, 0]], np.float32)
    ix, tree = _check(v, f, q, what="invalid mesh")
    assert tree.n_usable == 1 and tree.n_nodes == 1
    ix, tree = _check(v, np.delete(f, good, 0), q, what="only invalid faces")
    assert tree.n_nodes == 0
    for beta in (2.0, math.inf):
        w, acc, ev = _gpu(ix, q, beta)
        assert (w[:3] == 0.0).all() and np.isnan(w[3:]).all() and (acc == 0).all() and (ev == 0).all()
    v, f = W.opposite_twins()
    ix, tree = _check(v, f[:1], np.array([[0.25, 0.25, 2], [0.25, 0.25, -2], [2, 2, 1], [0, 0, 0]], np.float32), what="F = 1")
    empty = torch.empty(0, 3, device="cuda")
    w = ix.winding(empty)
    assert w.shape == (0,) and w.dtype == torch.float64 and len(ix.winding(empty, counts=True)) == 3
    v, f = W.coincident_copies(40)
    q = np.concatenate([np.array([[0.25, 0.25, 0.5], [0.25, 0.25, -0.5], [50, 0, 0]]),
                        np.random.default_rng(4).uniform(-1, 2, (62, 3))]).astype(np.float32)
    ix, tree = _check(v, f, q, betas=(2.0, 3.0), what="40 coincident faces")
    assert tree.L == 2 and tree.n_nodes == 3
    w, acc, ev = _gpu(ix, q[:3], 2.0)
    assert ev.tolist() == [40, 40, 0] and acc.tolist() == [0, 0, 1]


@pytest.mark.parametrize("m", [65, 257, 4097])
def test_partial_waves_and_blocks(m):
    v, f = P.box_mesh()
    q = (np.random.default_rng(m).uniform(-2, 2, (m, 3))).astype(np.float32)
    _check(v, f, q, betas=(2.0,), what="m = %d" % m)


def test_repeated_queries_and_a_second_build_give_identical_bits():
    m = _mc_sphere(32)
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    q = _shell_queries(2000, 48, 0.5, 12)
    ix = _index(v, f)
    for beta in (2.0, math.inf):
        first, second, third = _gpu(ix, q, beta), _gpu(ix, q, beta), _gpu(_index(v, f), q, beta)
        for other in (second, third):
            _same_bits(other[0], first[0], "w")
            assert np.array_equal(other[1], first[1]) and np.array_equal(other[2], first[2])
    a, b = ix._winding[0], _index(v, f)._winding_tree()[0]
    lay = ix.winding_layout()
    # the tree's head (48 bytes of its 256-byte slot are written) and the order of the usable faces behind it
    assert torch.equal(a[:48], b[:48]) and torch.equal(a[256:256 + 4 * lay["usable faces"]], b[256:256 + 4 * lay["usable faces"]])


# ---- classification --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("holed", [False, True])
def test_contains_by_winding_number(holed):
    from nicer_slam_amd import mesh_sdf
    v, f, tree, q, ex, walks = sphere_case(holed)
    inside = mesh_sdf.contains({"verts": v, "faces": f}, _cuda(q, torch.float32), method="winding").cpu().numpy()
    decided = np.abs(ex["w"] - 0.5) > 0.1
    print("%s sphere: %.2f %% of %d queries within 0.1 of w = 0.5" % ("holed" if holed else "closed", 100 * (~decided).mean(), len(q)))
    assert (~decided).mean() <= 0.02
    assert np.array_equal(inside[decided], (ex["w"] > 0.5)[decided])
    exact = mesh_sdf.contains({"verts": v, "faces": f}, _cuda(q, torch.float32), method="winding", beta=math.inf).cpu().numpy()
    assert np.array_equal(exact[decided], (ex["w"] > 0.5)[decided])
    nan = mesh_sdf.contains({"verts": v, "faces": f}, _cuda(np.array([[np.nan, 0, 0]], np.float32)), method="winding")
    assert nan.tolist() == [False]
    w = mesh_sdf.winding_number({"verts": v, "faces": f}, q[:65])     # an array of points: moved to the mesh's device
    assert w.is_cuda and w.dtype == torch.float64 and w.shape == (65,)
    with pytest.raises(ValueError):
        _index(v, f).winding(_cuda(q[:4], torch.float32), beta=0.5)


# ---- nicer_slam_amd/mesh_sdf.py with sign="winding" ------------------------------------------------------------------------------

def _grid_points(R, bound):
    from nicer_slam_amd import inference
    return inference.get_grid_uniform(R, (-bound, bound), "cuda")["grid_points"].cpu().numpy()


def test_mesh_sdf_grid_of_the_holed_sphere():
    from nicer_slam_amd import mesh_sdf
    v, f, tree, _, _, _ = sphere_case(True)
    mesh = {"verts": _cuda(v, torch.float32), "faces": _cuda(f, torch.int32)}
    R, bound, band = 32, 1.5, 0.2
    normal = mesh_sdf.mesh_sdf_grid(mesh, R, (-bound, bound), band=band).reshape(-1).cpu().numpy()
    wind = mesh_sdf.mesh_sdf_grid(mesh, R, (-bound, bound), band=band, sign="winding").reshape(-1).cpu().numpy()
    assert wind.dtype == np.float32 and np.array_equal(np.isnan(wind), np.isnan(normal))
    _same_bits(np.abs(wind), np.abs(normal), "|grid|")
    inband = np.nonzero(~np.isnan(wind))[0]
    assert 0.05 < inband.size / R ** 3 < 0.3
    pts = _grid_points(R, bound)[inband]
    w = W.exact(pts, tree)["w"]
    decided = np.abs(w - 0.5) > 0.1
    assert decided.mean() > 0.9
    assert np.array_equal((wind[inband] < 0)[decided], (w > 0.5)[decided])
    differ = (wind[inband] > 0) & (normal[inband] < 0)
    print("holed sphere grid: %d points in the band, %d where the pseudo-normal says inside and the winding number outside"
          % (inband.size, differ.sum()))
    assert differ.sum() >= 10 and (pts[differ][:, 2] > 0.7).all()    # all of them about the hole
    chunked = mesh_sdf.mesh_sdf_grid(mesh, R, (-bound, bound), band=band, sign="winding", chunk=5000).reshape(-1).cpu().numpy()
    _same_bits(chunked, wind, "chunked grid")
    # the default is the path of before: the same bits as the signed query
    again = mesh_sdf.mesh_sdf_grid(mesh, R, (-bound, bound), band=band, sign="normal").reshape(-1).cpu().numpy()
    _same_bits(again, normal, "sign = normal")


def test_the_two_rules_agree_on_the_closed_sphere():
    from nicer_slam_amd import mesh_sdf
    v, f, tree, _, _, _ = sphere_case(False)
    mesh = {"verts": _cuda(v, torch.float32), "faces": _cuda(f, torch.int32)}
    R, bound, band = 32, 1.5, 0.2
    normal = mesh_sdf.mesh_sdf_grid(mesh, R, (-bound, bound), band=band).reshape(-1).cpu().numpy()
    wind = mesh_sdf.mesh_sdf_grid(mesh, R, (-bound, bound), band=band, sign="winding").reshape(-1).cpu().numpy()
    _same_bits(np.abs(wind), np.abs(normal), "|grid|")
    r = np.linalg.norm(_grid_points(R, bound).astype(np.float64), axis=1)
    clear = ~np.isnan(wind) & (np.abs(r - 1.0) > P.sag(v, f) + 2.0 ** -22)      # where the sphere decides the side of the mesh
    assert clear.sum() > 2000
    assert np.array_equal(wind[clear] < 0, r[clear] < 1.0) and np.array_equal(normal[clear] < 0, r[clear] < 1.0)


def test_signed_distance_above_the_hole():
    from nicer_slam_amd import mesh_sdf
    v, f, tree, _, _, _ = sphere_case(True)
    ix = _index(v, f)
    q = _cuda(W.HOLE_QUERIES, torch.float32)
    normal = mesh_sdf.signed_distance(ix, q)
    wind = mesh_sdf.signed_distance(ix, q, sign="winding")
    exact = mesh_sdf.signed_distance(ix, q, sign="winding", beta=math.inf)
    assert bool((normal < 0).all()) and bool((wind > 0).all()) and torch.equal(wind, -normal) and torch.equal(exact, wind)
    _same_bits(normal.cpu().numpy(), ix.signed_query(q)[0].cpu().numpy(), "sign = normal")
    # under a bound: only the points with a closest point within it are given a sign
    far = _cuda(np.array([[0, 0, -0.5], [0, 0, -0.95], [0, 0, -1.05], [0, 0, 3], [np.nan, 0, 0]], np.float32))
    d = mesh_sdf.signed_distance(ix, far, max_dist=0.2, sign="winding").cpu().numpy()
    assert d[0] == np.inf and d[1] < 0 < d[2] and d[3] == np.inf and np.isnan(d[4])
    flipped = mesh_sdf.signed_distance(ix, far, max_dist=0.2, sign="winding", flip=True).cpu().numpy()
    assert flipped[1] > 0 and flipped[2] > 0 and flipped[0] == np.inf   # normals declared inward: w = -1 inside, 0 outside


def test_sdf_field_metrics_by_winding_number():
    from nicer_slam_amd import mesh_sdf
    v, f, tree, _, _, _ = sphere_case(False)
    ix = _index(v, f)
    sag = P.sag(v, f) + 2.0 ** -22
    seen = []

    def field(x):
        """|x| - 1, and within the sag of the sphere -- where the mesh and the sphere may differ on the side -- the mesh's own"""
        true = x.double().norm(dim=1) - 1.0
        own = mesh_sdf.signed_distance(ix, x, sign="winding")
        seen.append(int((true.abs() > sag).sum()))
        return torch.where(true.abs() > sag, true, own)

    out = mesh_sdf.sdf_field_metrics(field, ix, n_points=20000, sigma=0.01, band=0.05, seed=4, sign="winding")
    print("field metrics by winding number: %s; %d of 20000 points farther than the sag from the sphere" % (out, seen[0]))
    assert out["sign agreement"] == 1.0 and out["points"] > 0.95 * 20000 and seen[0] > 10000
    assert out["mean abs error"] <= out["rms error"] <= sag
    normal = mesh_sdf.sdf_field_metrics(field, ix, n_points=20000, sigma=0.01, band=0.05, seed=4)
    assert normal["points"] == out["points"] and normal["sign agreement"] == 1.0


def test_cli_round_trip_with_the_winding_sign(tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_sdf
    v, f, tree, _, _, _ = sphere_case(True)
    mesh = {"verts": _cuda(v, torch.float32), "faces": _cuda(f, torch.int32), "normals": _cuda(v, torch.float32)}
    inference.write_ply(tmp_path / "m.ply", mesh)
    pts = np.concatenate([W.HOLE_QUERIES, _shell_queries(100, 20, 1.0, 6)])
    np.save(tmp_path / "p.npy", pts)
    argv = [str(tmp_path / "m.ply"), "--resolution", "16", "--bounds", "-1.5", "1.5", "--band", "0.8", "--out", str(tmp_path / "s.npy"),
            "--points", str(tmp_path / "p.npy"), "--out-dist", str(tmp_path / "d.npy"), "--sign", "winding", "--out-winding",
            str(tmp_path / "w.npy")]
    mesh_sdf.main(argv)
    text = capsys.readouterr().out
    assert "grid: 16^3" in text and "points: 127" in text and "winding numbers: 127" in text
    back = inference.read_ply(tmp_path / "m.ply")
    want = mesh_sdf.mesh_sdf_grid(back, 16, (-1.5, 1.5), band=0.8, sign="winding")
    _same_bits(np.load(tmp_path / "s.npy"), want.cpu().numpy(), "grid file")
    d = mesh_sdf.signed_distance(back, pts, max_dist=0.8, sign="winding").cpu().numpy()   # (0, 0, 1.2) is 0.73 from the rim
    _same_bits(np.load(tmp_path / "d.npy"), np.where(np.isfinite(d), d, np.nan), "distance file")
    w = np.load(tmp_path / "w.npy")
    assert w.dtype == np.float64 and w.shape == (127,)
    _same_bits(w, mesh_sdf.winding_number(back, pts).cpu().numpy(), "winding file")
    assert (w[:7] < 0.5).all() and (np.load(tmp_path / "d.npy")[:7] > 0).all()
    mesh_sdf.main(argv + ["--exact"])
    exact = np.load(tmp_path / "w.npy")
    assert np.abs(exact - W.exact(pts, tree)["w"]).max() <= 1e-12 and np.abs(exact - w).max() <= 0.05
