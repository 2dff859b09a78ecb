"""Closest point on a triangle mesh on the device (csrc/mesh_closest.hip, nicer_slam_amd/mesh_eval.py: TriIndex, closest_point,
distance_p2m, mesh_metrics(surface="mesh")) against the numpy oracle tests/p2m_ref.py -- bit for bit: face, float64 d2 and the fp32
closest point -- and against a chunked float64 brute force on the device where numpy would take too long."""
import functools
import math

import numpy as np
import pytest
import torch

import p2m_ref as P
from test_mesh_closest_cpu import box_queries, invalid_mesh, sphere_queries

pytestmark = pytest.mark.gpu


def _cuda(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _index(v, f):
    from nicer_slam_amd.mesh_eval import TriIndex
    return TriIndex(_cuda(v, torch.float32), _cuda(f, torch.int32))


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    view = np.int64 if got.dtype == np.float64 else np.int32
    bad = np.nonzero((got.view(view) != want.view(view)) & ~nan)
    assert bad[0].size == 0, (what, bad[0][:5], got[bad][:5], want[bad][:5])


def _check(v, f, q, ref=None):
    """index over (v, f), query q, everything equal to the oracle (or to ``ref`` = (face, d2, closest, totals))"""
    ix = _index(v, f)
    d2, face, close = ix.query(_cuda(q, torch.float32), squared=True)
    rface, rd2, rclose, rtot = ref if ref is not None else P.closest_brute(q, v, f)
    assert list(ix.skipped) == [int(x) for x in rtot]
    face = face.cpu().numpy()
    assert np.array_equal(face, rface), (np.nonzero(face != rface)[0][:5], face[face != rface][:5], rface[face != rface][:5])
    _same_bits(d2.cpu().numpy(), rd2, "d2")
    _same_bits(close.cpu().numpy(), rclose, "closest")
    return ix, d2, face, close


def _mc_sphere(res, r=0.5, bound=1.0):
    from nicer_slam_amd import inference
    ax = torch.linspace(-bound, bound, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - r).float().cuda()
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol, 0.0, (step,) * 3, (-bound,) * 3)


def _shell_queries(n_near, n_far, r, seed):
    """n_near points within 0.3 of the sphere of radius r, n_far far outside it"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n_near + n_far, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rad = np.concatenate([r + rng.uniform(-0.3, 0.3, n_near), r + 10.0 ** rng.uniform(0.5, 2.0, n_far)])
    return (d * rad[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _latlong_case():
    """the 24 x 48 sphere, 4096 queries and the oracle's answer: computed once, shared, never written to"""
    v, f, n_degenerate = P.latlong_sphere(24, 48)
    q = sphere_queries()
    return v, f, q, P.closest_brute(q, v, f), n_degenerate


def _brute_torch(q, v, f, pairs=1 << 21):
    """(face, d2, closest fp32, totals) by a float64 brute force on the device in the header's operation order: separate torch
    operations, each rounded on its own, no fused multiply-add; the lowest index among the exact minima"""
    q64, v64, f = q.double(), v.double(), f.long()
    V = v.shape[0]
    bad_idx = ((f < 0) | (f >= V)).any(1)
    fc = torch.where(bad_idx[:, None], torch.zeros_like(f), f)
    a, b, c = v64[fc[:, 0]], v64[fc[:, 1]], v64[fc[:, 2]]
    nonfinite = ~(torch.isfinite(a).all(1) & torch.isfinite(b).all(1) & torch.isfinite(c).all(1))
    ab, ac = b - a, c - a
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    flat = (nx == 0) & (ny == 0) & (nz == 0)
    cause = torch.where(bad_idx, 1, torch.where(nonfinite, 2, torch.where(flat, 3, 0)))
    totals = [int((cause == k).sum()) for k in (1, 2, 3)]
    use = (cause == 0).nonzero()[:, 0]
    M = q.shape[0]
    face = torch.full((M,), -1, dtype=torch.long, device=q.device)
    best = torch.full((M,), math.inf, dtype=torch.float64, device=q.device)
    close = torch.full((M, 3), math.nan, dtype=torch.float64, device=q.device)
    if use.numel():
        a, b, c = a[use][None], b[use][None], c[use][None]
        ab, ac = b - a, c - a
        dot = lambda u, w: (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]
        step = max(1, pairs // use.numel())
        for lo in range(0, M, step):
            qq = q64[lo:lo + step, None, :]
            ap, bp, cp = qq - a, qq - b, qq - c
            d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
            vc = d1 * d4 - d3 * d2
            vb = d5 * d2 - d1 * d6
            va = d3 * d6 - d5 * d4
            w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            e = 1.0 / ((va + vb) + vc)
            zero, one = torch.zeros_like(d1), torch.ones_like(d1)
            tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                     (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
            s, t = vb * e, vc * e
            for test, sv, tv in reversed(list(zip(tests, [zero, one, d1 / (d1 - d3), zero, zero, 1.0 - w],
                                                  [zero, zero, zero, one, d2 / (d2 - d6), w]))):
                s, t = torch.where(test, sv, s), torch.where(test, tv, t)
            p = (a + s[..., None] * ab) + t[..., None] * ac
            r = qq - p
            dd = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
            dd = torch.where(torch.isnan(dd), torch.full_like(dd, math.inf), dd)
            m = dd.min(1).values
            ar = torch.arange(use.numel(), device=q.device)
            k = torch.where(dd == m[:, None], ar[None, :], use.numel()).min(1).values       # the first of the exact minima
            found = m < math.inf
            k = torch.where(found, k, torch.zeros_like(k))
            rows = torch.arange(k.numel(), device=q.device)
            best[lo:lo + step] = m
            face[lo:lo + step] = torch.where(found, use[k], torch.full_like(k, -1))
            close[lo:lo + step] = torch.where(found[:, None], p[rows, k], torch.full_like(p[rows, k], math.nan))
    bad = ~torch.isfinite(q64).all(1)
    face[bad] = -1
    best[bad] = math.nan
    close[bad] = math.nan
    return face.cpu().numpy(), best.cpu().numpy(), close.float().cpu().numpy(), np.array(totals)


# ---- bit for bit against the oracle -------------------------------------------------------------------------------------------

def test_box_every_face_large():
    """a 3 x 3 x 2 box: the centroids span (3, 3, 2) and 2 F = 24 cells allow a 3 x 3 x 2 grid of unit cells (the cube root of
    18 / 24 is 0.909; 3 / 0.909 = 3.3 and 2 / 0.909 = 2.2 round down), so every face is 3 cells long on an axis: all on the list"""
    lo, hi = (-1.5, -1.5, -1.0), (1.5, 1.5, 1.0)
    v, f = P.box_mesh(lo, hi)
    q = box_queries() * np.float32([1.5, 3.0, 4.0])                    # the special points land on this box's faces, edges, corners
    ix, d2, *_ = _check(v, f, q)
    lay = ix.layout()
    assert lay["cells"] == [3, 3, 2] and lay["cell size"] == [1.0, 1.0, 1.0], lay
    assert lay["large faces"] == 12 and lay["grid faces"] == 0 and lay["skipped faces"] == 0, lay
    # the closed form, within the roundings counted in tests/test_mesh_closest_cpu.py
    err = np.abs(np.sqrt(d2.cpu().numpy()) - P.box_distance(q.astype(np.float64), lo, hi)).max()
    assert err <= 20 * np.spacing(np.abs(q).max().astype(np.float64)), err


def test_box_split_between_the_grid_and_the_list():
    """the 2 x 1 x 0.5 box of the CPU tests: 5 x 2 x 1 cells of (0.4, 0.5, 0.5); the four triangles of the x = -1 and x = +1 sides are
    exactly 2 cells long in y and one in z and stay in the grid, the other eight are 5 cells long in x"""
    v, f = P.box_mesh()
    ix, *_ = _check(v, f, box_queries())
    lay = ix.layout()
    assert lay["cells"] == [5, 2, 1], lay
    assert lay["grid faces"] == 4 and lay["large faces"] == 8 and lay["skipped faces"] == 0, lay


def test_latlong_sphere_with_degenerate_poles():
    v, f, q, ref, n_degenerate = _latlong_case()
    ix, *_ = _check(v, f, q, ref)
    assert ix.skipped == (0, 0, n_degenerate) and ix.layout()["skipped faces"] == n_degenerate


def test_marching_cubes_sphere_near_and_far_queries():
    m = _mc_sphere(32)
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    assert 1000 < f.shape[0] < 10000
    _check(v, f, _shell_queries(512, 512, 0.5, 3))


# ---- device-side brute force --------------------------------------------------------------------------------------------------

def test_device_brute_force_equals_numpy_then_serves_at_64_cubed():
    v, f, q, ref, _ = _latlong_case()
    got = _brute_torch(_cuda(q), _cuda(v), _cuda(f))
    assert np.array_equal(got[0], ref[0]) and got[3].tolist() == ref[3].tolist()
    _same_bits(got[1], ref[1], "brute d2")
    _same_bits(got[2], ref[2], "brute closest")
    m = _mc_sphere(64)
    vq = _shell_queries(3072, 1024, 0.5, 4)
    assert m["faces"].shape[0] > 5000
    big = _brute_torch(_cuda(vq), m["verts"], m["faces"])
    ix, d2, face, close = _check(m["verts"].cpu().numpy(), m["faces"].cpu().numpy(), vq, big)
    lay = ix.layout()
    assert lay["grid faces"] > 0.9 * m["faces"].shape[0], lay          # the grid, not the list, answered these
    # ... and it pruned: only faces no farther than the answer by about their own size get the full evaluation.  For a query at
    # distance d from a sphere of radius R those lie in a cap of height about one face size l, of area 2 pi R l: some 200 of the
    # 64^3 mesh's faces (l = 0.03, R = 0.5, mean face area 2.6e-4) whatever d is.  A tenth of the mesh leaves a factor of five.
    n_eval = ix.query(_cuda(vq), counts=True)[3].double()
    print("64^3 sphere, F = %d: faces evaluated per query mean %.1f max %d" % (m["faces"].shape[0], n_eval.mean(), n_eval.max()))
    assert float(n_eval.mean()) < 0.1 * m["faces"].shape[0]


# ---- mixed scales -------------------------------------------------------------------------------------------------------------

def _mixed_mesh():
    m = _mc_sphere(32)
    sv, sf = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    plane_v = np.array([[-50, -50, -1], [50, -50, -1], [50, 50, -1], [-50, 50, -1]], np.float32)
    plane_f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    rng = np.random.default_rng(7)
    stray_v = (np.array([1000.0, 3.0, -2.0]) + 0.05 * rng.standard_normal((12, 3))).astype(np.float32)
    stray_f = np.stack([np.arange(10), np.arange(10) + 1, np.arange(10) + 2], 1).astype(np.int32)
    bad_v = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.1, 0.1]], np.float32)
    n0, n1, n2 = sv.shape[0], sv.shape[0] + 4, sv.shape[0] + 16
    v = np.concatenate([sv, plane_v, stray_v, bad_v])
    V = v.shape[0]
    invalid = np.array([[0, 1, -1], [0, V, 2], [n2, 1, 2], [3, n2 + 1, 4], [5, 5, 6], [n2 + 2, n2 + 2, n2 + 2], [n2, V + 7, 1]],
                       np.int32)
    totals = [3, 2, 2]
    parts = [sf[:500], invalid[:3], sf[500:], plane_f + n0, invalid[3:5], stray_f + n1, invalid[5:]]
    return v, np.concatenate(parts).astype(np.int32), totals


def test_mixed_scales_in_one_mesh():
    v, f, totals = _mixed_mesh()
    rng = np.random.default_rng(8)
    near = _shell_queries(256, 0, 0.5, 9)
    above = np.stack([rng.uniform(-45, 45, 128), rng.uniform(-45, 45, 128), rng.uniform(-0.9, 6.0, 128)], 1)
    above = above[np.abs(above[:, :2]).max(1) > 3.0]
    stray = np.array([1000.0, 3.0, -2.0]) + rng.uniform(-0.5, 0.5, (64, 3))
    far = np.array([[1e6, 0, 0], [-1e6, 1e6, 0], [3e5, -2e5, 1e6], [0, 0, -1e6], [1e6, 1e6, 1e6], [999, 1e6, -2]])
    nonfinite = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]])
    q = np.concatenate([near, above, stray, far, nonfinite]).astype(np.float32)
    ref = P.closest_brute(q, v, f)
    assert ref[3].tolist() == totals
    ix, d2, face, close = _check(v, f, q, ref)
    lay = ix.layout()
    # the plane's two triangles (longer than 2 cells) and the stray component's ten (1000 units = thousands of cells outside the grid)
    # are on the list
    assert lay["large faces"] >= 12 and lay["skipped faces"] == sum(totals), lay
    # ... so the far component costs the queries near the sphere a box test per face, not the pruning: with it in the grid faces' box
    # rho would exceed 1/4 and every query would evaluate every face
    n_eval = ix.query(_cuda(q[:256]), counts=True)[3].double()
    print("mixed scales, F = %d: faces evaluated per query near the sphere mean %.1f max %d" % (f.shape[0], n_eval.mean(), n_eval.max()))
    assert float(n_eval.mean()) < 0.25 * f.shape[0]
    n_plane = int((face[256:256 + above.shape[0]] >= 0).sum())
    assert n_plane == above.shape[0]
    assert (face[-4:] == -1).all() and np.isnan(d2.cpu().numpy()[-4:]).all() and np.isnan(close.cpu().numpy()[-4:]).all()
    # the grid still resolves the sphere although a component lies 1000 units away
    assert max(lay["cell size"]) < 0.5, lay


def test_a_mesh_of_only_invalid_faces():
    v, f, totals, good = invalid_mesh()
    f = np.delete(f, good, 0)
    q = np.array([[0.25, 0.25, 1], [0, 0, 5], [1e6, 0, 0]], np.float32)
    ix, d2, face, close = _check(v, f, q)
    assert ix.skipped == tuple(totals)
    assert (face == -1).all() and bool(torch.isinf(d2).all()) and bool((d2 > 0).all()) and bool(torch.isnan(close).all())
    dist, face, _ = ix.query(_cuda(q))
    assert bool(torch.isinf(dist).all())


# ---- edge sizes ---------------------------------------------------------------------------------------------------------------

def test_one_face_one_query_and_no_query():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    ix, d2, face, close = _check(v, f, np.array([[0.25, 0.25, 2]], np.float32))
    assert face.tolist() == [0] and float(d2[0]) == 4.0 and close.cpu().tolist() == [[0.25, 0.25, 0.0]]
    dist, face, close = ix.query(torch.empty(0, 3, device="cuda"))
    assert dist.shape == (0,) and dist.dtype == torch.float64 and face.shape == (0,) and close.shape == (0, 3)


@pytest.mark.parametrize("m", [65, 4097])
def test_partial_waves_and_blocks(m):
    v, f = P.box_mesh()
    q = (np.random.default_rng(m).uniform(-2, 2, (m, 3))).astype(np.float32)
    _check(v, f, q)


def test_every_face_in_one_cell():
    """500 copies of one triangle and one distinct face above it.  The 1/64 and 63/64 quantiles of the 501 centroids coincide on
    every axis, so the grid is one cell of size 1; the faces (legs 0.5: 0.5 cells long, sigma = 0.5 / 0.25^2 = 8, far below 2^16)
    all stay in it, and every query walks all 501 records of that cell"""
    tri = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]], np.float32)
    v = np.concatenate([tri, tri + np.float32([0, 0, 0.125])]).astype(np.float32)
    f = np.concatenate([np.tile([[0, 1, 2]], (500, 1)), [[3, 4, 5]]]).astype(np.int32)
    q = (np.random.default_rng(11).uniform(-1.0, 1.5, (300, 3))).astype(np.float32)
    ix, d2, face, close = _check(v, f, q)
    lay = ix.layout()
    assert lay["cells"] == [1, 1, 1] and lay["cell size"] == [1.0, 1.0, 1.0], lay
    assert lay["grid faces"] == 501 and lay["large faces"] == 0 and lay["skipped faces"] == 0, lay
    assert set(face.tolist()) == {0, 500}                             # the copies tie: the lowest index; the distinct face wins above


def test_repeated_queries_and_a_second_build_give_identical_bits():
    m = _mc_sphere(32)
    q = _cuda(_shell_queries(2000, 48, 0.5, 12))
    from nicer_slam_amd.mesh_eval import TriIndex
    ix = TriIndex(m["verts"], m["faces"])
    first = ix.query(q, squared=True)
    second = ix.query(q, squared=True)
    third = TriIndex(m["verts"], m["faces"]).query(q, squared=True)
    for other in (second, third):
        assert torch.equal(first[1], other[1])
        assert torch.equal(first[0].view(torch.int64), other[0].view(torch.int64))
        assert torch.equal(first[2].view(torch.int32), other[2].view(torch.int32))
    assert not torch.isnan(first[0]).any()


# ---- the public functions -----------------------------------------------------------------------------------------------------

def test_closest_point_and_distance_p2m():
    from nicer_slam_amd import mesh_eval as M
    v, f = P.box_mesh()
    q = box_queries()
    mesh = {"verts": v, "faces": f}
    close, dist, face = M.closest_point(mesh, q)                       # numpy in: the order of trimesh.proximity.closest_point
    rface, rd2, rclose, _ = P.closest_brute(q, v, f)
    assert close.dtype == torch.float32 and dist.dtype == torch.float64 and face.dtype == torch.int64
    assert np.array_equal(face.cpu().numpy(), rface)
    _same_bits(close.cpu().numpy(), rclose, "closest")
    assert torch.equal(dist, torch.sqrt(_cuda(rd2)))
    # sqrt of an exact d2 differs from the closed form by the roundings counted in tests/test_mesh_closest_cpu.py
    assert np.abs(dist.cpu().numpy() - P.box_distance(q.astype(np.float64))).max() <= 20 * np.spacing(np.abs(q).max().astype(np.float64))
    d = M.distance_p2m(_cuda(q), {"verts": _cuda(v), "faces": _cuda(f)})
    assert torch.equal(d, dist)


def _plane_range(mesh):
    """(least distance of a usable face's plane from the origin, largest vertex norm): the mesh's surface lies radially between"""
    v, f = mesh["verts"].cpu().numpy(), mesh["faces"].cpu().numpy()
    f = f[P.face_causes(v, f) == 0]
    n = P.face_normals(v, f)
    v64 = v.astype(np.float64)
    return float(np.abs((n * v64[f[:, 0]]).sum(1)).min()), float(np.linalg.norm(v64, axis=1).max())


def test_mesh_metrics_surface_equals_the_oracle_on_the_same_samples():
    from nicer_slam_amd import mesh_eval as M
    rec, gt = _mc_sphere(32, 0.5), _mc_sphere(32, 0.55)
    n = 1000
    out = M.mesh_metrics(rec, gt, n_points=n, seed=3, align=False, surface="mesh")
    assert out["surface"] == "mesh"
    rp, ri = M.sample_surface(rec["verts"], rec["faces"], n, 3)
    gp, gi = M.sample_surface(gt["verts"], gt["faces"], n, 4)
    rv, rf, gv, gf = (x.cpu().numpy() for x in (rec["verts"], rec["faces"], gt["verts"], gt["faces"]))
    fa, da, _, _ = P.closest_brute(rp.cpu().numpy(), gv, gf)
    fc, dc, _, _ = P.closest_brute(gp.cpu().numpy(), rv, rf)
    rn, gn = M._face_normals(rec["verts"], rec["faces"].long())[ri], M._face_normals(gt["verts"], gt["faces"].long())[gi]
    fed = M.metrics_from_surfaces(rp, rn, (rec["verts"], rec["faces"]), gp, gn, (gt["verts"], gt["faces"]),
                                  acc=(torch.sqrt(_cuda(da)), _cuda(fa)), com=(torch.sqrt(_cuda(dc)), _cuda(fc)))
    for k, x in fed.items():
        assert out[k] == x, k                                          # float equality, key by key
    ref = P.surface_metrics(np.sqrt(da), np.sqrt(dc), (P.face_normals(gv, gf)[fa] * rn.cpu().numpy()).sum(1),
                            (P.face_normals(rv, rf)[fc] * gn.cpu().numpy()).sum(1))
    for k, x in ref.items():
        assert out[k] == pytest.approx(x, rel=1e-12, abs=1e-15), k


def test_a_mesh_against_itself_has_no_floor():
    """what the feature is for: against the surface a perfect reconstruction scores (almost) 0, against samples 0.5 sqrt(A / n)"""
    from nicer_slam_amd import mesh_eval as M
    m = _mc_sphere(64, 0.5)
    n = 20000
    v = m["verts"].double()
    mag = float(v.abs().max())
    extent = float((v.max(0).values - v.min(0).values).max())
    out = M.mesh_metrics(m, m, n_points=n, align=False, surface="mesh")
    # a sample is (v0 + a e1) + b e2 in fp32, e = v - v0: six roundings of values up to 2 |v| per coordinate, so it lies within
    # sqrt(3) * 6 * 2^-24 * 2 mag of its own face; the distance to the mesh is no larger
    bound = math.sqrt(3) * 12 * 2.0 ** -24 * mag
    print("self: accuracy %.3e completion %.3e bound %.3e" % (out["accuracy"], out["completion"], bound))
    assert bound <= 1e-6 * extent
    assert 0 <= out["accuracy"] < bound and 0 <= out["completion"] < bound, out
    assert out["completion ratio"] == 1.0 and out["f-score"] == 1.0 and out["normals"] > 0.999
    f = m["faces"].long()
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    area = float(0.5 * torch.linalg.cross(e1, e2).norm(dim=1).sum())
    floor = 0.5 * math.sqrt(area / n)
    same = M.mesh_metrics(m, m, n_points=n, align=False, surface="samples")
    print("self, samples: accuracy %.3e completion %.3e floor %.3e" % (same["accuracy"], same["completion"], floor))
    assert same["accuracy"] >= 0.5 * floor and same["completion"] >= 0.5 * floor, (same, floor)


def test_concentric_spheres():
    from nicer_slam_amd import mesh_eval as M
    a, b = _mc_sphere(31, 1.0, 1.5), _mc_sphere(31, 1.1, 1.5)           # voxel size 0.1
    lo_a, hi_a = _plane_range(a)
    lo_b, hi_b = _plane_range(b)
    sag_a, sag_b = hi_a - lo_a, hi_b - lo_b
    out = M.mesh_metrics(a, b, n_points=20000, align=False, surface="mesh")
    print("concentric: accuracy %.4f completion %.4f normals %.4f; a in [%.4f, %.4f], b in [%.4f, %.4f]"
          % (out["accuracy"], out["completion"], out["normals"], lo_a, hi_a, lo_b, hi_b))
    # every point of a has a norm in [lo_a, hi_a] and every point of b one in [lo_b, hi_b]; both are closed and star-shaped, so
    # the distance from a point of one to the other surface is at least lo_b - hi_a and at most hi_b - lo_a (along the ray)
    for key in ("accuracy", "completion"):
        assert lo_b - hi_a <= out[key] <= hi_b - lo_a, (key, out[key])
        assert abs(out[key] - 0.1) <= sag_a + sag_b + 0.1, (key, out[key])
    # a face's normal is within alpha = acos(lo / hi) of the direction of any of its points; a sample x and its closest point y
    # are at most D = hi_b - lo_a apart, so their directions differ by at most asin(D / lo_a)
    angle = math.acos(lo_a / hi_a) + math.acos(lo_b / hi_b) + math.asin((hi_b - lo_a) / lo_a)
    assert angle < math.pi / 2 and out["normals"] >= math.cos(angle), (out["normals"], math.cos(angle))


def test_the_default_is_the_sample_form_and_the_cli_names_the_mode(tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_eval as M
    rec, gt = _mc_sphere(32, 0.5), _mc_sphere(32, 0.52)
    default = M.mesh_metrics(rec, gt, n_points=5000, seed=2)
    named = M.mesh_metrics(rec, gt, n_points=5000, seed=2, surface="samples")
    assert set(default) == set(named) and "surface" not in default
    for k, x in default.items():
        assert np.array_equal(x, named[k]) if isinstance(x, np.ndarray) else x == named[k], k
    inference.write_ply(tmp_path / "rec.ply", rec)
    inference.write_ply(tmp_path / "gt.ply", gt)
    want = M.mesh_metrics(inference.read_ply(tmp_path / "rec.ply"), inference.read_ply(tmp_path / "gt.ply"), n_points=5000, seed=2,
                          surface="mesh")
    capsys.readouterr()
    got = M.main([str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "--points", "5000", "--seed", "2", "--surface", "mesh"])
    text = capsys.readouterr().out
    assert "surface: mesh" in text
    for k, x in want.items():
        assert np.array_equal(x, got[k]) if isinstance(x, np.ndarray) else x == got[k], k
    assert f"accuracy:  {want['accuracy'] * 100} cm" in text and f"completion:  {want['completion'] * 100} cm" in text
    assert want["accuracy"] != default["accuracy"]
    capsys.readouterr()
    M.main([str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "--points", "5000", "--seed", "2"])
    assert "surface:" not in capsys.readouterr().out                   # the default printout is unchanged
