"""Signed and range-limited closest-point queries on the device (csrc/mesh_sdf.hip; mesh_eval.TriIndex.signed_query / query(max_dist=);
nicer_slam_amd/mesh_sdf.py) against the numpy oracle tests/sdf_ref.py: face, float64 d2, the fp32 closest point and the feature bit
for bit -- against the oracle and against TriIndex.query -- the pseudo-normal within a counted tolerance, the sign wherever the
oracle's own margin decides it, and the cost of a bounded query from the cells it visits."""
import functools
import math

import numpy as np
import pytest
import torch

import p2m_ref as P
import sdf_ref as S
from test_mesh_closest_cpu import box_queries, invalid_mesh, sphere_queries
from test_mesh_closest_gpu import _cuda, _index, _mc_sphere, _plane_range, _same_bits, _shell_queries
from test_mesh_sdf_cpu import box_case, spike_apex_query, spike_case

pytestmark = pytest.mark.gpu

# |N_gpu - N_ref| <= N_TOL * W per component.  The unit normals are the same IEEE operations in the same order on both sides (subtract,
# multiply, add, square root, divide), so they agree to the last bit -- or to 2 ulp where a library's float64 square root is within one
# ulp and not correctly rounded.  Otherwise the two sides differ in atan2 alone, within 2 ulp of the true angle in ocml and 1 ulp in
# glibc, and its argument |u x w| carries the square root's ulp: alpha_g differs by at most 4 * 2^-52 alpha_g.  The product
# alpha_g * n and the running additions of N and of W then round operands that differ by that much: one more ulp of the running sum
# (<= 2^-52 W, as |n| = 1) per corner.  In all |dN| <= 7 k * 2^-52 * W for a vertex of k corners, 2 k * 2^-52 * W for an edge of k faces.
# 2^-40 = 4096 * 2^-52 leaves a factor 9 at k = 64 and 13 at the spike's apex (k = 43), counted this pessimistically.
N_TOL = 2.0 ** -40
# the sign is compared where |e . N| > SIGN_MARGIN * |e| * W in the oracle: e . N inherits |e| |dN| <= 2^-40 |e| W from the above and
# three roundings of its own; 2^-36 is 16 times that.  At most 1 % of a case's queries may lie under the margin.
SIGN_MARGIN = 2.0 ** -36


def _raw(ix, q, weld=True, flip=False, max_d2=math.inf, adj=None):
    """nsa_tri_signed_query_counted itself: dict of face, d2, closest, feature, sign, N, W, evaluated, cells as numpy arrays.  ``adj``:
    adjacency faces to build the lists from in place of the index's own"""
    from nicer_slam_amd._native import lib, check
    q = _cuda(q, torch.float32)
    m, dev = q.shape[0], q.device
    if adj is None:
        adj_t, buf = ix.adjacency(weld)
    else:
        adj_t = _cuda(adj, torch.int32)
        buf = torch.empty(lib.nsa_tri_adjacency_workspace(ix.V, ix.F), dtype=torch.uint8, device=dev)
        check(lib.nsa_tri_adjacency_build(ix.verts.data_ptr(), ix.V, ix.faces.data_ptr(), adj_t.data_ptr(), ix.F, buf.data_ptr(), None))
    out = dict(face=torch.empty(m, dtype=torch.int32, device=dev), d2=torch.empty(m, dtype=torch.float64, device=dev),
               closest=torch.empty(m, 3, dtype=torch.float32, device=dev), feature=torch.empty(m, dtype=torch.int8, device=dev),
               sign=torch.empty(m, dtype=torch.int8, device=dev), N=torch.empty(m, 3, dtype=torch.float64, device=dev),
               W=torch.empty(m, dtype=torch.float64, device=dev), evaluated=torch.empty(m, dtype=torch.int32, device=dev),
               cells=torch.empty(m, dtype=torch.int32, device=dev))
    check(lib.nsa_tri_signed_query_counted(ix.buf.data_ptr(), buf.data_ptr(), ix.verts.data_ptr(), ix.V, ix.faces.data_ptr(),
                                           adj_t.data_ptr(), ix.F, q.data_ptr(), m, float(max_d2), int(flip),
                                           *(out[k].data_ptr() for k in ("face", "d2", "closest", "feature", "sign", "N", "W",
                                                                         "evaluated", "cells")), None))
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in out.items()}


def _compare(got, ref, what=""):
    """the kernel's answers against the oracle's, as the module docstring says; returns how many queries lay under the sign margin"""
    assert np.array_equal(got["face"].astype(np.int64), ref["face"]), what
    _same_bits(got["d2"], ref["d2"], what + " d2")
    _same_bits(got["closest"], ref["closest"], what + " closest")
    assert np.array_equal(got["feature"], ref["feature"]), what
    tol = N_TOL * ref["W"]
    err_n, err_w = np.abs(got["N"] - ref["N"]).max(1), np.abs(got["W"] - ref["W"])
    print("%s: max |dN| / W %.3e, max |dW| / W %.3e" % (what, (err_n / np.maximum(ref["W"], 1e-300)).max(),
                                                        (err_w / np.maximum(ref["W"], 1e-300)).max()))
    assert (err_n <= tol).all() and (err_w <= tol).all(), what
    # (d2 = 0 is + by the contract on both sides, d2 being equal bit for bit; so is W = 0 -- no contributing face -- where the
    # tolerance above is 0 and holds the kernel's N to exactly 0)
    decided = (np.abs(ref["edotn"]) > SIGN_MARGIN * ref["enorm"] * ref["W"]) | (ref["d2"] == 0) | (ref["W"] == 0)
    no_winner = ref["face"] < 0
    assert np.array_equal(got["sign"][decided | no_winner], ref["sign"][decided | no_winner]), what
    undecided = int((~decided & ~no_winner).sum())
    assert undecided <= 0.01 * max(1, ref["face"].shape[0]), (what, undecided)
    return undecided


def _check(v, f, q, weld=True, flip=False, max_dist=None, ref=None, adj=None, what=""):
    """index over (v, f); the raw entry point against the oracle; TriIndex.query and TriIndex.signed_query against the raw entry point"""
    ix = _index(v, f)
    max_d2 = math.inf if max_dist is None else float(max_dist) ** 2
    got = _raw(ix, q, weld, flip, max_d2, adj)
    if ref is None:
        ref = S.signed_brute(q, v, f, adj=adj, weld=weld, flip=flip, max_d2=max_d2)
    undecided = _compare(got, ref, what)
    qc = _cuda(q, torch.float32)
    d2, face, close = ix.query(qc, squared=True) if max_dist is None else ix.query(qc, squared=True, max_dist=max_dist)
    assert np.array_equal(face.cpu().numpy(), got["face"]), what
    _same_bits(d2.cpu().numpy(), got["d2"], what + " d2 of query")
    _same_bits(close.cpu().numpy(), got["closest"], what + " closest of query")
    if adj is None:
        dist, sface, sclose, feature, N, W = ix.signed_query(qc, max_dist=max_dist, flip=flip, weld=weld, normals=True)
        assert dist.dtype == torch.float64 and sface.dtype == torch.int64 and feature.dtype == torch.int8
        want = _cuda(got["sign"].astype(np.float64)) * torch.sqrt(_cuda(got["d2"]))
        _same_bits(dist.cpu().numpy(), want.cpu().numpy(), what + " signed distance")
        assert np.array_equal(sface.cpu().numpy(), got["face"]) and np.array_equal(feature.cpu().numpy(), got["feature"])
        _same_bits(sclose.cpu().numpy(), got["closest"], what + " closest of signed_query")
        _same_bits(N.cpu().numpy(), got["N"], what + " N")
        _same_bits(W.cpu().numpy(), got["W"], what + " W")
    return ix, got, ref, undecided


# ---- kernel against oracle ------------------------------------------------------------------------------------------------------

def test_box_every_face_on_the_list():
    lo, hi = (-1.5, -1.5, -1.0), (1.5, 1.5, 1.0)
    v, f = P.box_mesh(lo, hi)
    q = box_queries() * np.float32([1.5, 3.0, 4.0])
    ix, got, ref, undecided = _check(v, f, q, what="box, listed")
    lay = ix.layout()
    assert lay["large faces"] == 12 and lay["grid faces"] == 0, lay
    assert (got["cells"] == 0).all()                                 # nothing in the grid: no cell is looked at
    assert set(np.unique(ref["feature"]).tolist()) == {0, 1, 2, 3, 4, 5, 6}
    q64 = q.astype(np.float64)
    outside = (np.maximum(np.maximum(np.array(lo) - q64, q64 - np.array(hi)), 0.0) > 0).any(1)
    on = ref["d2"] == 0
    assert np.array_equal(got["sign"][~on] > 0, outside[~on]) and (got["sign"][on] == 1).all()


def test_box_split_between_the_grid_and_the_list():
    v, f, q, ref = box_case()
    ix, got, _, undecided = _check(v, f, q, ref=ref, what="box, split")
    lay = ix.layout()
    assert lay["grid faces"] == 4 and lay["large faces"] == 8, lay
    assert undecided == 0                                            # the oracle's least margin on these inputs is 0.34
    dist = ix.signed_query(_cuda(q, torch.float32))[0].cpu().numpy()
    q64 = q.astype(np.float64)
    outside = (np.maximum(np.maximum(np.array([-1, -0.5, -0.25]) - q64, q64 - np.array([1, 0.5, 0.25])), 0.0) > 0).any(1)
    want = np.where(outside, 1.0, -1.0) * P.box_distance(q64)      # within the roundings counted in tests/test_mesh_closest_cpu.py
    assert np.abs(dist - want).max() <= 20 * np.spacing(np.abs(q64).max()) and np.array_equal(dist < 0, ~outside)
    flipped = ix.signed_query(_cuda(q, torch.float32), flip=True)[0].cpu().numpy()
    assert np.array_equal(flipped, -dist)


def test_spike():
    v, f, q, ref = spike_case()
    ix, got, _, undecided = _check(v, f, q, ref=ref, what="spike")
    assert undecided == 0                                            # the oracle's least margin on these inputs is 0.0139
    naive = S.closest_face_sign(q, v, f, ref)
    assert int((naive != got["sign"]).sum()) >= 1                    # the inputs tell the rules apart
    apex = _check(v, f, spike_apex_query(), what="spike apex")[1]
    assert apex["sign"][0] == 1 and apex["feature"][0] in (1, 2, 4)
    assert apex["W"][0] == pytest.approx(8 * math.atan(math.tan(0.1) / math.sqrt(1 + math.tan(0.1) ** 2)), rel=1e-6)


@functools.lru_cache(maxsize=None)
def _latlong_case(weld):
    v, f, _ = P.latlong_sphere(24, 48)
    q = sphere_queries(512)
    return v, f, q, S.signed_brute(q, v, f, weld=weld)


@pytest.mark.parametrize("weld", [True, False])
def test_latlong_sphere(weld):
    v, f, q, ref = _latlong_case(weld)
    ix, got, _, _ = _check(v, f, q, weld=weld, ref=ref, what="lat-long sphere, weld=%s" % weld)
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    clear = np.abs(r - 1.0) > P.sag(v, f) + 2.0 ** -22
    assert np.array_equal(got["sign"][clear], np.where(r > 1.0, 1, -1)[clear])
    if weld:                                                         # contains(): the public form of the same answer
        from nicer_slam_amd import mesh_sdf
        inside = mesh_sdf.contains({"verts": v, "faces": f}, _cuda(q, torch.float32)).cpu().numpy()
        assert np.array_equal(inside[clear], (r < 1.0)[clear])


def _mc_flip(m):
    """whether the faces of a marching-cubes mesh wind against its vertex normals (which point towards increasing value)"""
    v, f, n = m["verts"].double(), m["faces"].long(), m["normals"].double()
    fn = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    agree = (fn * n[f].sum(1)).sum(1)
    assert bool((agree > 0).all()) or bool((agree < 0).all())        # one winding throughout
    return bool((agree < 0).all())


def test_marching_cubes_sphere_near_and_far_queries():
    m = _mc_sphere(32)
    flip = _mc_flip(m)
    print("marching_cubes: face normals %s the vertex normals (increasing value): flip = %s" % ("oppose" if flip else "follow", flip))
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    q = _shell_queries(320, 192, 0.5, 3)
    ix, got, ref, _ = _check(v, f, q, flip=flip, what="MC sphere")
    lo, hi = _plane_range(m)
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    assert np.array_equal(got["sign"][r > hi], np.ones((r > hi).sum(), np.int8))            # outside the volume's level set: +
    assert np.array_equal(got["sign"][r < lo], -np.ones((r < lo).sum(), np.int8)) and (r < lo).sum() > 50


def test_open_and_non_manifold_meshes():
    rng = np.random.default_rng(21)
    v, f = S.open_square()
    q = np.concatenate([np.array([[0.25, 0.5, 1], [0.25, 0.5, -1], [2, 0.5, 0.5], [2, 0.5, -0.5], [2, 0.5, 0], [-1, -1, 2],
                                  [-1, -1, -2], [0.5, 0.5, 0.25], [0.5, 0.5, -0.25]]), rng.uniform(-1, 2, (248, 3))]).astype(np.float32)
    got = _check(v, f, q, what="open square")[1]
    assert got["sign"][:9].tolist() == [1, -1, 1, -1, 1, 1, -1, 1, -1]
    v, f = S.three_on_an_edge()
    q = np.concatenate([np.array([[0.5, 0, -1], [0.5, 0.01, -1], [0.5, 0.5, -1]]), rng.uniform(-1, 2, (62, 3))]).astype(np.float32)
    got = _check(v, f, q, what="three on an edge")[1]
    assert got["W"][0] == 3.0 and got["N"][0].tolist() == [0.0, -1.0, 2.0] and got["sign"][:3].tolist() == [-1, -1, -1]
    # two coincident faces of opposite winding: N = 0 on their interior, sign +
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    q = np.array([[0.25, 0.25, 1], [0.25, 0.25, -1], [-1, -1, 1], [0.5, -1, 1]], np.float32)
    got, ref = _raw(_index(v, f), q), S.signed_brute(q, v, f)
    _compare({k: x[:2] for k, x in got.items()}, {k: x[:2] for k, x in ref.items()}, "opposite twins")
    assert got["face"].tolist() == [0, 0, 0, 0] and got["feature"].tolist() == [0, 0, 1, 3]
    assert got["sign"].tolist() == [1, -1, 1, 1]                     # the interior is the lower face's own normal ...
    assert got["N"][2:].tolist() == [[0.0, 0.0, 0.0]] * 2 and got["W"][2] == pytest.approx(math.pi) and got["W"][3] == 2.0   # ... vertices and edges sum both: N = 0, +


def _mixed_mesh():
    """a 32^3 sphere, a plane of two triangles 100 units wide, a stray component 1000 units away and faces of every skipped kind"""
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
    invalid = np.array([[0, 1, -1], [0, V, 2], [n2, 1, 2], [3, n2 + 1, 4], [5, 5, 6], [n2 + 2, n2 + 2, n2 + 2], [n2, V + 7, 1]], np.int32)
    parts = [sf[:500], invalid[:3], sf[500:], plane_f + n0, invalid[3:5], stray_f + n1, invalid[5:]]
    return v, np.concatenate(parts).astype(np.int32)


def test_mixed_scales_invalid_faces_and_non_finite_queries():
    v, f = _mixed_mesh()
    rng = np.random.default_rng(8)
    near = _shell_queries(128, 0, 0.5, 9)
    above = np.stack([rng.uniform(-45, 45, 48), rng.uniform(-45, 45, 48), rng.uniform(-3.0, 6.0, 48)], 1)
    stray = np.array([1000.0, 3.0, -2.0]) + rng.uniform(-0.5, 0.5, (32, 3))
    far = np.array([[1e6, 0, 0], [-1e6, 1e6, 0], [0, 0, -1e6], [999, 1e6, -2]])
    nonfinite = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]])
    q = np.concatenate([near, above, stray, far, nonfinite]).astype(np.float32)
    ix, got, ref, _ = _check(v, f, q, what="mixed scales")
    assert ix.layout()["large faces"] >= 12 and sum(ix.skipped) == 7
    assert (got["face"][-4:] == -1).all() and np.isnan(got["d2"][-4:]).all() and (got["feature"][-4:] == -1).all()
    assert (got["sign"][-4:] == 1).all() and (got["N"][-4:] == 0).all()
    dist = ix.signed_query(_cuda(q, torch.float32))[0]
    assert bool(torch.isnan(dist[-4:]).all()) and bool(torch.isfinite(dist[:-4]).all())
    # the same under a bound of 2: the far queries and most of those about the plane drop out, the rest is unchanged
    _check(v, f, q, max_dist=2.0, what="mixed scales, bounded")


def test_invalid_meshes():
    v, f, totals, good = invalid_mesh()
    q = np.array([[-1, -1, 1], [0.25, 0.25, -1], [2, -1, 0.5], [np.nan, 0, 0], [0, -np.inf, 0]], np.float32)
    for weld in (True, False):
        got = _check(v, f, q, weld=weld, what="invalid mesh, weld=%s" % weld)[1]
        assert got["face"].tolist() == [good, good, good, -1, -1] and got["sign"].tolist() == [1, -1, 1, 1, 1]
    adj = f.copy()
    adj[good] = [0, 1, 99]                                           # an adjacency index outside [0, V): never looked up
    adj[0] = [-5, 1 << 30, 2]
    got = _check(v, f, q, adj=adj, what="invalid mesh, adjacency out of range")[1]
    assert got["W"].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]
    none = _check(v, np.delete(f, good, 0), q, what="only invalid faces")[1]
    assert (none["face"] == -1).all() and (none["d2"][:3] == np.inf).all() and (none["sign"] == 1).all()


def test_one_face_and_no_query():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    ix, got, _, _ = _check(v, f, np.array([[0.25, 0.25, 2], [0.25, 0.25, -2], [2, 2, 1]], np.float32), what="F = 1")
    assert got["sign"].tolist() == [1, -1, 1] and got["feature"].tolist() == [0, 0, 6]
    empty = torch.empty(0, 3, device="cuda")
    dist, face, close, feature = ix.signed_query(empty)
    assert dist.shape == (0,) and dist.dtype == torch.float64 and face.shape == (0,) and close.shape == (0, 3) and feature.shape == (0,)
    assert len(ix.signed_query(empty, normals=True, counts=True)) == 8
    assert ix.query(empty, max_dist=1.0)[0].shape == (0,) and len(ix.query(empty, counts=True, max_dist=1.0)) == 5


@pytest.mark.parametrize("m", [65, 257, 4097])
def test_partial_waves_and_blocks(m):
    v, f = P.box_mesh()
    q = (np.random.default_rng(m).uniform(-2, 2, (m, 3))).astype(np.float32)
    _check(v, f, q, what="m = %d" % m)
    _check(v, f, q, max_dist=0.75, what="m = %d, bounded" % m)


def test_repeated_queries_and_a_second_build_give_identical_bits():
    m = _mc_sphere(32)
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    q = _shell_queries(2000, 48, 0.5, 12)
    ix = _index(v, f)
    first, second, third = _raw(ix, q), _raw(ix, q), _raw(_index(v, f), q)
    for other in (second, third):
        for k in ("face", "feature", "sign", "evaluated", "cells"):
            assert np.array_equal(first[k], other[k]), k
        for k in ("d2", "closest", "N", "W"):
            _same_bits(other[k], first[k], k)
    kinds = set(np.unique(first["feature"]).tolist())
    assert 0 in kinds and kinds & {1, 2, 4} and kinds & {3, 5, 6} and not np.isnan(first["N"]).any()


# ---- the bound ------------------------------------------------------------------------------------------------------------------

def test_the_bound_at_and_about_a_distance():
    v, f = P.box_mesh()
    q = np.array([[2, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0]], np.float32)
    at = _check(v, f, q, max_dist=1.0, what="at the bound")[1]
    assert at["face"][0] >= 0 and at["d2"][0] == 1.0                  # d2 == max_d2 is inside
    ix = _index(v, f)
    below = _raw(ix, q, max_d2=np.nextafter(1.0, 0.0))
    _compare(below, S.signed_brute(q, v, f, max_d2=np.nextafter(1.0, 0.0)), "just outside")
    assert below["face"][0] == -1 and below["d2"][0] == np.inf and np.isnan(below["closest"][0]).all() and below["sign"][0] == 1
    zero = _check(v, f, q, max_dist=0.0, what="max_dist = 0")[1]
    assert zero["face"].tolist()[0] == -1 and zero["face"][1] >= 0 and zero["d2"][1] == 0.0 and zero["face"][2] == -1
    _check(v, f, q, max_dist=math.inf, what="max_dist = inf")
    assert ix.signed_query(_cuda(q), max_dist=0.5, flip=True)[0].cpu().tolist()[:3] == [-math.inf, 0.0, 0.25]
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError):
            ix.signed_query(_cuda(q), max_dist=bad)
        with pytest.raises(ValueError):
            ix.query(_cuda(q), max_dist=bad)


def test_a_bounded_query_equals_the_masked_one_and_stops_early():
    m = _mc_sphere(32)
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    q = _shell_queries(600, 200, 0.5, 5)
    ix = _index(v, f)
    lay = ix.layout()
    assert lay["large faces"] == 0 and lay["grid faces"] == f.shape[0], lay
    h_min = min(lay["cell size"])
    bound = 1.5 * h_min
    free = _raw(ix, q)
    got = _raw(ix, q, max_d2=bound * bound)
    inside = free["d2"] <= bound * bound
    assert 100 < inside.sum() < 500
    for k in ("face", "feature", "sign"):
        assert np.array_equal(got[k], np.where(inside, free[k], {"face": -1, "feature": -1, "sign": 1}[k])), k
    _same_bits(got["d2"], np.where(inside, free["d2"], np.inf), "d2")
    _same_bits(got["closest"], np.where(inside[:, None], free["closest"], np.float32(np.nan)), "closest")
    _same_bits(got["N"], np.where(inside[:, None], free["N"], 0.0), "N")
    # Cells.  The rings stop at ring r once, on every axis and side, the cell plane r cells from the query's own cell, pulled back
    # by 2 cells (how far a grid face reaches beyond its centroid) and by 2^-9 cell and the padding, lies beyond the bound: the
    # query is somewhere in its cell, so that plane is at least (r - 1) - 2 cells of at least h_min away, and ring
    # r = ceil(bound / h_min) + 4 is never walked.  Rings 0 .. r - 1 are a cube of 2 (r - 1) + 1 = 2 ceil(bound / h_min) + 7 cells a
    # side -- for a query beyond the bound.  One within it also stops there, as its best only lowers the value pruned against.
    limit = (2 * math.ceil(bound / h_min) + 7) ** 3
    assert limit == 11 ** 3 < np.prod(lay["cells"])
    print("bounded: cells visited max %d (limit %d; unbounded max %d of %d), faces evaluated mean %.2f (unbounded %.2f)"
          % (got["cells"][~inside].max(), limit, free["cells"].max(), np.prod(lay["cells"]), got["evaluated"].mean(),
             free["evaluated"].mean()))
    assert (got["cells"][~inside] < limit).all() and (got["cells"] < limit).all()
    assert free["cells"].max() > limit                               # ... which the unbounded walk of a far query exceeds
    # Faces.  A face is evaluated only when its padded box is within the bound of the query, and the box lies within its own
    # diagonal of the face: a query farther from the mesh than bound + the longest box diagonal evaluates none.
    v64 = v.astype(np.float64)
    diag = np.linalg.norm(v64[f].max(1) - v64[f].min(1), axis=1).max() * (1 + 2.0 ** -20)
    beyond = np.sqrt(free["d2"]) > bound + diag
    assert beyond.sum() > 250 and (got["evaluated"][beyond] == 0).all()
    assert (got["evaluated"] <= free["evaluated"]).all()
    # the unsigned form: the same walk
    d2, face, close, n_eval, n_cells = ix.query(_cuda(q), counts=True, squared=True, max_dist=bound)
    assert np.array_equal(face.cpu().numpy(), got["face"]) and np.array_equal(n_cells.cpu().numpy(), got["cells"])
    _same_bits(d2.cpu().numpy(), got["d2"], "d2 of query")
    assert np.array_equal(n_eval.cpu().numpy(), got["evaluated"])


# ---- nicer_slam_amd/mesh_sdf.py ----------------------------------------------------------------------------------------------------

R_SPHERE = 0.5


def _sphere_tolerance(m):
    """the mesh's surface lies radially in [lo, hi] about the sphere of radius r: for any x the signed distance to the mesh is in
    [|x| - hi, |x| - lo] (along the ray through x the surface is met in that range, and the ball of radius lo is inside, the mesh
    inside the ball of radius hi), so it differs from |x| - r by at most max(hi - r, r - lo): the mesh's sag about the sphere"""
    lo, hi = _plane_range(m)
    return max(abs(hi - R_SPHERE), abs(R_SPHERE - lo))


def test_mesh_sdf_grid_of_a_sphere():
    from nicer_slam_amd import inference, mesh_eval, mesh_sdf
    m = _mc_sphere(32)
    flip = _mc_flip(m)
    R, step = 32, 2.0 / 31
    band = 3 * step
    grid = mesh_sdf.mesh_sdf_grid(m, R, (-1, 1), band=band, flip=flip)
    assert grid.shape == (R, R, R) and grid.dtype == torch.float32
    pts = inference.get_grid_uniform(R, (-1, 1), "cuda")["grid_points"]
    true = pts.double().norm(dim=1) - R_SPHERE
    sag = _sphere_tolerance(m)
    flat = grid.reshape(-1)
    finite = torch.isfinite(flat)
    # fp32 rounding of a value below 1: 2^-24; the points' own rounding moves |x| by less than sqrt(3) 2^-24
    err = (flat.double() - true)[finite].abs().max()
    print("grid: %d of %d points within the band, max |grid - (|x| - r)| %.3e, sag %.3e" % (finite.sum(), R ** 3, err, sag))
    assert float(err) <= sag + 3 * 2.0 ** -24
    assert bool(finite[true.abs() < band - sag].all()) and bool((~finite[true.abs() > band + sag]).all())
    assert bool(torch.isnan(flat[~finite]).all()) and 0.1 < float(finite.double().mean()) < 0.5
    # exactly the unbounded answer, masked
    d = mesh_sdf.signed_distance(m, pts, flip=flip)
    want = torch.where(d.abs() <= band, d, torch.full_like(d, math.nan)).float()
    _same_bits(flat.cpu().numpy(), want.cpu().numpy(), "grid")
    small = mesh_sdf.mesh_sdf_grid(m, R, (-1, 1), band=band, flip=flip, chunk=5000)              # chunked: the same
    _same_bits(small.cpu().numpy(), grid.cpu().numpy(), "chunked grid")
    # meshed as it is: the level set of the band lies within a voxel of the mesh it came from
    again = inference.marching_cubes(grid.permute(1, 0, 2).contiguous(), 0.0, (step,) * 3, (-1.0,) * 3)
    used = again["verts"][again["faces"].long().unique()]
    assert again["faces"].shape[0] > 1000
    far = mesh_eval.distance_p2m(used, m)
    back = mesh_eval.distance_p2m(m["verts"], again)
    print("re-meshed: %d faces, max distance to the source %.3e, of the source to it %.3e (voxel %.3e)"
          % (again["faces"].shape[0], far.max(), back.max(), step))
    assert float(far.max()) < step and float(back.max()) < step


def test_sdf_field_metrics_of_the_exact_field():
    from nicer_slam_amd import mesh_sdf
    m = _mc_sphere(32)
    flip = _mc_flip(m)
    sag = _sphere_tolerance(m)
    seen = []

    def field(x):
        seen.append(x)
        return x.double().norm(dim=1) - R_SPHERE

    out = mesh_sdf.sdf_field_metrics(field, m, n_points=20000, sigma=0.01, band=0.05, seed=4, flip=flip)
    x = seen[0]
    assert x.shape == (20000, 3) and x.dtype == torch.float32
    true = x.double().norm(dim=1) - R_SPHERE
    print("field metrics: %s; sag %.3e" % (out, sag))
    assert 0.95 * 20000 < out["points"] <= 20000                     # sigma = 0.01 per coordinate: almost all within 0.05
    assert 0 <= out["mean abs error"] <= out["rms error"] <= sag
    doubtful = float((true.abs() <= sag).double().mean())            # only there may the mesh and the sphere disagree on the side
    assert 1.0 - doubtful * 20000 / out["points"] <= out["sign agreement"] <= 1.0
    assert float((true < 0).double().mean()) > 0.3 and float((true > 0).double().mean()) > 0.3
    again = mesh_sdf.sdf_field_metrics(field, m, n_points=20000, sigma=0.01, band=0.05, seed=4, flip=flip)
    assert again == out and torch.equal(seen[1], seen[0])
    wrong = mesh_sdf.sdf_field_metrics(lambda p: -(p.double().norm(dim=1) - R_SPHERE), m, n_points=20000, seed=4, flip=flip)
    assert wrong["sign agreement"] < 0.5 and wrong["mean abs error"] > out["mean abs error"]


def test_cli_round_trip(tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_sdf
    m = _mc_sphere(32)
    flip = _mc_flip(m)
    inference.write_ply(tmp_path / "m.ply", m)
    pts = _shell_queries(100, 20, 0.5, 6)
    np.save(tmp_path / "p.npy", pts)
    argv = [str(tmp_path / "m.ply"), "--resolution", "16", "--bounds", "-0.8", "0.8", "--band", "0.2", "--out", str(tmp_path / "s.npy"),
            "--points", str(tmp_path / "p.npy"), "--out-dist", str(tmp_path / "d.npy")] + (["--flip"] if flip else [])
    mesh_sdf.main(argv)
    text = capsys.readouterr().out
    assert "grid: 16^3" in text and "points: 120" in text
    back = inference.read_ply(tmp_path / "m.ply")
    want = mesh_sdf.mesh_sdf_grid(back, 16, (-0.8, 0.8), band=0.2, flip=flip)
    grid = np.load(tmp_path / "s.npy")
    assert grid.dtype == np.float32 and grid.shape == (16, 16, 16)
    _same_bits(grid, want.cpu().numpy(), "grid file")
    d = mesh_sdf.signed_distance(back, pts, max_dist=0.2, flip=flip).cpu().numpy()
    got = np.load(tmp_path / "d.npy")
    assert got.dtype == np.float64 and np.isnan(got[100:]).all() and np.isfinite(got[:100]).sum() > 40
    _same_bits(got, np.where(np.isfinite(d), d, np.nan), "distance file")
