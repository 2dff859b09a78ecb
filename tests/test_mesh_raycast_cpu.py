"""Ray casting against a mesh without a GPU: the numpy oracle tests/raycast_ref.py (header Section 17) against closed forms, its
rules (culling, ties, windows, degenerate rays), the walk against the brute force and the box clause against its absence on every
case of the suite, the watertight property the test was chosen for, the pruning, and the argument checks of the C ABI entry points
and of the Python layer.  The GPU tests (tests/test_mesh_raycast_gpu.py) hold the kernels to this oracle bit for bit."""
import ctypes
import functools
import math

import numpy as np
import pytest

import mc_ref
import p2m_ref as P
import raster_ref as rr
import raycast_ref as R
import sdf_ref as S
import winding_ref as W


def mc_sphere_np(res, r=0.5, bound=1.0):
    """the marching-cubes sphere of tests/test_mesh_closest_gpu.py::_mc_sphere from the numpy oracle of the extraction"""
    ax = np.linspace(-bound, bound, res)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    step = float(ax[1] - ax[0])
    m = mc_ref.marching_cubes((np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - r).astype(np.float32), 0.0, (step,) * 3, (-bound,) * 3)
    return m["verts"], m["faces"]


def mixed_mesh_np():
    """tests/test_mesh_sdf_gpu.py::_mixed_mesh over the lat-long sphere: a large plane, a stray far component, faces of every
    skipped kind"""
    sv, sf, _ = P.latlong_sphere(12, 24, 0.5)
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
    parts = [sf[:100], invalid[:3], sf[100:], plane_f + n0, invalid[3:5], stray_f + n1, invalid[5:]]
    return v, np.concatenate(parts).astype(np.int32)


def mixed_rays(n=120, seed=5):
    """rays at the sphere, down at the plane, at the stray component and away from everything, then the degenerate ones"""
    o, d = R.sphere_rays(n, seed, 3.0, 0.6)
    rng = np.random.default_rng(seed)
    po = np.stack([rng.uniform(-60, 60, 40), rng.uniform(-60, 60, 40), rng.uniform(2, 30, 40)], 1)
    pd = np.stack([rng.uniform(-0.3, 0.3, 40), rng.uniform(-0.3, 0.3, 40), -np.ones(40)], 1)
    so = np.tile([[0.0, 0.0, 4.0]], (24, 1))
    sd = np.array([1000.0, 3.0, -2.0]) + rng.uniform(-0.08, 0.08, (24, 3)) - so
    bad_o = np.array([[np.nan, 0, 0], [0, 0, 3], [0, 0, 3], [0, np.inf, 0], [0, 0, 3]])
    bad_d = np.array([[0, 0, -1], [0, np.nan, -1], [0, 0, 0], [0, 0, -1], [-np.inf, 0, -1]])
    return (np.concatenate([o, po, so, bad_o]).astype(np.float32), np.concatenate([d, pd, sd, bad_d]).astype(np.float32))


def spike_rays():
    """rays through the apex of S.spike() from every side, and a spread about it"""
    v, f, apex, _ = S.spike()
    o, d = R.sphere_rays(96, 2, 3.0, 0.3)
    o = o + np.float32([0, 0, 0.5])
    rng = np.random.default_rng(3)
    ao = (v[apex].astype(np.float64) + rng.standard_normal((33, 3)) * 2.0).astype(np.float32)
    ad = (v[apex].astype(np.float64) - ao.astype(np.float64)).astype(np.float32)
    return np.concatenate([ao, o]), np.concatenate([ad, d])


CASE_NAMES = ("unit box", "stretched box", "spike", "lat-long sphere", "lat-long soup", "MC sphere 32", "mixed", "coincident centroids",
              "open square", "three on an edge", "opposite twins")


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (verts, faces, origins, dirs)}: every mesh of the suite with its rays; built once, never written to"""
    out = {}
    o, d = R.sphere_rays(513, 0, 3.0, 0.9)
    out["unit box"] = P.box_mesh() + (o, d)
    out["stretched box"] = P.box_mesh((-1.5, -1.5, -1.0), (150.0, 1.5, 1.0)) + (o * np.float32([20, 1, 1]), d * np.float32([20, 1, 1]))
    v, f, _, _ = S.spike()
    out["spike"] = (v, f) + spike_rays()
    v, f, _ = P.latlong_sphere(24, 48)
    o, d = R.sphere_rays(513, 1, 3.0, 1.1)
    out["lat-long sphere"] = (v, f, o, d)
    out["lat-long soup"] = (v[f.reshape(-1)], np.arange(3 * f.shape[0], dtype=np.int32).reshape(-1, 3), o, d)
    out["MC sphere 32"] = mc_sphere_np(32) + R.sphere_rays(513, 2, 3.0, 0.6)
    out["mixed"] = mixed_mesh_np() + mixed_rays()
    out["coincident centroids"] = R.coincident_centroids(40) + R.sphere_rays(65, 4, 3.0, 0.5)
    out["open square"] = S.open_square() + R.sphere_rays(63, 5, 3.0, 1.0)
    out["three on an edge"] = S.three_on_an_edge() + R.sphere_rays(64, 6, 3.0, 1.0)
    out["opposite twins"] = W.opposite_twins() + R.sphere_rays(64, 7, 3.0, 1.0)
    assert tuple(out) == CASE_NAMES
    return out


@functools.lru_cache(maxsize=None)
def tree_of(name):
    v, f = cases()[name][:2]
    return R.Tree(v, f)


@functools.lru_cache(maxsize=None)
def walked(name):
    v, f, o, d = cases()[name]
    return R.walk(o, d, tree_of(name))


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want) if want.dtype.kind == "f" else np.zeros(want.shape, bool)
    assert np.array_equal(np.isnan(got) if got.dtype.kind == "f" else nan, nan), what
    view = np.int64 if got.dtype.itemsize == 8 else np.int32
    bad = np.nonzero((got.view(view) != want.view(view)) & ~nan)
    assert bad[0].size == 0, (what, bad[0][:5], got[bad][:5], want[bad][:5])


def same_answer(got, want, what):
    assert np.array_equal(got["face"], want["face"]), (what, np.nonzero(got["face"] != want["face"])[0][:5])
    same_bits(got["t"], want["t"], what + ": t")
    same_bits(got["bary"], want["bary"], what + ": bary")


# ---- closed forms -------------------------------------------------------------------------------------------------------------------

def test_axis_aligned_rays_into_the_box_hit_at_the_analytic_t():
    v, f = P.box_mesh()                                              # (-1, -0.5, -0.25) .. (1, 0.5, 0.25)
    tree = R.Tree(v, f)
    o = np.array([[-3, 0.125, 0.0625], [3, 0.125, 0.0625], [0.25, -2, 0.125], [0.25, 0.125, 5], [0.25, 0.125, 0], [4, 4, 4]], np.float32)
    d = np.array([[1, 0, 0], [-2, 0, 0], [0, 0.5, 0], [0, 0, -1], [0, 0, 1], [1, 0, 0]], np.float32)
    want = np.array([2.0, 1.0, 3.0, 4.75, 0.25, np.inf])
    for r in (R.brute(o, d, tree), R.walk(o, d, tree), R.brute(o, d, tree, box=False)):
        assert np.array_equal(r["t"], want), r["t"]
        assert (r["face"][:5] >= 0).all() and r["face"][5] == -1 and np.isnan(r["bary"][5]).all()
        b = r["bary"][:5]
        assert np.abs(b.sum(1) - 1.0).max() <= 2.0 ** -52 and (b >= 0).all()
        fv = v.astype(np.float64)[f[r["face"][:5]]]
        hit = (b[:, :, None] * fv).sum(1)
        assert np.abs(hit - (o[:5].astype(np.float64) + want[:5, None] * d[:5])).max() <= 1e-15
    far = R.walk(o, d, tree, tmin=3.5)                                # past the first wall of rays 0 and 2: their far one
    assert np.array_equal(far["t"], [4.0, np.inf, 5.0, 4.75, np.inf, np.inf])
    assert np.array_equal(R.walk(o, d, tree, tmax=1.5)["t"], [np.inf, 1.0, np.inf, np.inf, 0.25, np.inf])


def test_open_square_from_both_sides_with_and_without_culling():
    v, f = S.open_square()                                            # normals +z
    tree = R.Tree(v, f)
    o = np.array([[0.25, 0.5, 2], [0.25, 0.5, -2], [0.75, 0.25, 2], [2, 2, 2]], np.float32)
    d = np.array([[0, 0, -1], [0, 0, 4], [0, 0, -1], [0, 0, -1]], np.float32)
    r = R.walk(o, d, tree)
    assert np.array_equal(r["t"], [2.0, 0.5, 2.0, np.inf]) and r["face"].tolist() == [1, 1, 0, -1]
    back = R.walk(o, d, tree, flags=R.CULL_BACK)                      # the ray from below meets the faces from behind
    assert np.array_equal(back["t"], [2.0, np.inf, 2.0, np.inf])
    front = R.walk(o, d, tree, flags=R.CULL_FRONT)
    assert np.array_equal(front["t"], [np.inf, 0.5, np.inf, np.inf])
    for flags in (0, R.CULL_BACK, R.CULL_FRONT):
        same_answer(R.walk(o, d, tree, flags=flags), R.brute(o, d, tree, flags=flags), "square, flags %d" % flags)
    # on the diagonal both faces are hit at the same t: the lower index wins; in the plane nothing is hit (det == 0)
    diag = R.walk(np.float32([[0.5, 0.5, 1], [-1, 0.5, 0]]), np.float32([[0, 0, -1], [1, 0, 0]]), tree)
    assert diag["face"].tolist() == [0, -1] and diag["t"][0] == 1.0


def test_three_faces_on_an_edge_and_opposite_twins():
    v, f = S.three_on_an_edge()
    tree = R.Tree(v, f)
    o = np.float32([[0.5, 0, -3], [0.5, 3, 3], [0.25, 0, -3]])        # at the shared edge from below, and from the +y +z side
    d = np.float32([[0, 0, 1], [0, -1, -1], [0, 0, 1]])
    r = R.walk(o, d, tree)
    assert np.array_equal(r["t"], [3.0, 3.0, 3.0]) and r["face"].tolist() == [0, 0, 0]        # every face holds the edge: the lowest
    assert R.walk(o, d, tree, flags=R.ANY_HIT)["hit"].all()
    v, f = W.opposite_twins()
    tree = R.Tree(v, f)
    o, d = np.float32([[0.25, 0.25, 1], [0.25, 0.25, -1]]), np.float32([[0, 0, -1], [0, 0, 1]])
    r = R.walk(o, d, tree)
    assert r["face"].tolist() == [0, 0] and np.array_equal(r["t"], [1.0, 1.0])                # a tie: the lower face index
    assert R.walk(o, d, tree, flags=R.CULL_BACK)["face"].tolist() == [0, 1]                   # each side sees its own front
    assert R.walk(o, d, tree, flags=R.CULL_FRONT)["face"].tolist() == [1, 0]


def test_degenerate_rays_and_meshes():
    v, f = P.box_mesh()
    tree = R.Tree(v, f)
    o = np.float32([[np.nan, 0, 0], [0, 0, 3], [0, 0, 3], [0, -np.inf, 0], [0, 0, 3]])
    d = np.float32([[0, 0, -1], [0, np.nan, -1], [0, 0, 0], [0, 0, -1], [0, 0, -1]])
    for r in (R.walk(o, d, tree), R.brute(o, d, tree)):
        assert np.isnan(r["t"][:4]).all() and (r["face"][:4] == -1).all() and r["t"][4] == 2.75
    w = R.walk(o, d, tree)
    assert (w["nodes"][:4] == 0).all() and (w["tested"][:4] == 0).all() and not w["hit"][:4].any()
    empty = R.Tree(v, np.array([[0, 0, 1], [0, 1, 99]], np.int32))    # no usable face
    assert empty.n_nodes == 0
    r = R.walk(o, d, empty)
    assert np.isnan(r["t"][:4]).all() and r["t"][4] == np.inf and (r["face"] == -1).all() and (r["nodes"] == 0).all()


# ---- the tree against the brute force, the box clause against its absence --------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_NAMES)
def test_walk_equals_brute_force_and_the_box_clause_changes_nothing(name):
    v, f, o, d = cases()[name]
    tree = tree_of(name)
    assert tree.n_nodes <= R.max_nodes(tree.F) and tree.L == R.level_of(tree.n_usable)
    w = walked(name)
    b = R.brute(o, d, tree)
    plain = R.brute(o, d, tree, box=False)
    same_answer(w, b, name + ": walk against brute force")
    same_answer(b, plain, name + ": with against without the box clause")
    assert np.array_equal(R.walk(o, d, tree, flags=R.ANY_HIT)["hit"], np.isfinite(w["t"])), name
    hits = np.isfinite(w["t"])
    print("%s: L = %d, %d nodes, %d usable faces; %d of %d rays hit; %.1f nodes and %.1f faces tested per ray"
          % (name, tree.L, tree.n_nodes, tree.n_usable, hits.sum(), hits.size, w["nodes"].mean(), w["tested"].mean()))
    if "box" in name or "sphere" in name or "soup" in name:
        assert hits.sum() >= hits.size // 4, name                    # the rays are aimed at the mesh
    # a window that cuts off the first hit returns the second: equal to the brute force under the same window
    t1 = w["t"][hits]
    if t1.size:
        cut = float(np.median(t1))
        w2, b2 = R.walk(o, d, tree, tmin=cut), R.brute(o, d, tree, tmin=cut)
        same_answer(w2, b2, name + ": tmin window")
        same_answer(b2, R.brute(o, d, tree, tmin=cut, box=False), name + ": tmin window, box clause")
        assert (w2["t"][np.isfinite(w2["t"])] >= cut).all()
        w3 = R.walk(o, d, tree, tmax=cut)
        same_answer(w3, R.brute(o, d, tree, tmax=cut), name + ": tmax window")
        assert np.array_equal(np.isfinite(w3["t"]), hits & (w["t"] <= cut))
    for flags in (R.CULL_BACK, R.CULL_FRONT):
        same_answer(R.walk(o[:65], d[:65], tree, flags=flags), R.brute(o[:65], d[:65], tree, flags=flags), name + ": culling")


def test_layout_of_small_and_worst_case_trees():
    assert tree_of("unit box").L == 1 and tree_of("open square").n_nodes == 1 and tree_of("open square").L == 0
    t = tree_of("coincident centroids")
    assert t.L == 2 and t.n_nodes == 3 and t.leaf.tolist() == [False, False, True]        # a chain down to one leaf of 40 faces
    w = walked("coincident centroids")
    assert w["tested"].max() <= 40 and w["nodes"].max() == 3
    t = tree_of("lat-long sphere")
    assert t.L == 5 and t.n_usable == 2208
    # every child entry points at a node one level down whose key has that octant
    ks, octs = np.nonzero(t.child)
    ch = t.child[ks, octs]
    assert ch.size == t.n_nodes - 1 and np.array_equal(np.sort(ch), np.arange(1, t.n_nodes))
    assert np.array_equal(t.level[ch], t.level[ks] + 1)
    assert np.array_equal((t.key[t.begin[ch]] >> (3 * (t.L - t.level[ch]))) & 7, octs)
    assert (t.lo[ks] <= t.lo[ch]).all() and (t.hi[ks] >= t.hi[ch]).all()


# ---- the property the test was chosen for ------------------------------------------------------------------------------------------

def test_no_ray_passes_through_a_vertex_or_an_edge_of_the_sphere():
    """6000 rays from outside, within 15 degrees of the normal, exactly through fp32 vertices (target - origin is exact in fp32 for
    most of them: t == 1.0), edge midpoints and random edge points of the 24 x 48 lat-long sphere.  On the sphere with one vertex per
    position every ray hits at its target.  On P.latlong_sphere as it is, whose longitude seam is listed twice with y = 0 on one side
    and y = sin(2 pi) = -1.2e-16 on the other, 3 of the 6000 -- all aimed at seam vertices -- pass through that crack and report the
    far side (t = 2.94 .. 2.99), with and without the box clause: the mesh is open there, by 1e-16, and the test says so."""
    v, f = R.welded_latlong_sphere(24, 48)
    tree = R.Tree(v, f)
    assert tree.n_usable == 2208
    o, d, target = R.watertight_rays(v, f, 6000, 0, 1.0, 15.0)
    r = R.walk(o, d, tree)
    assert (r["t"] == 1.0).sum() > 1000                                                  # rays exactly through a vertex
    assert np.isfinite(r["t"]).all(), np.nonzero(~np.isfinite(r["t"]))[0][:5]          # every ray hits ...
    assert np.abs(r["t"] - 1.0).max() <= 1e-6, np.abs(r["t"] - 1.0).max()              # ... at its target, never the far side
    same_answer(r, R.brute(o, d, tree, box=False), "watertight rays: walk against the plain brute force")
    # the hit lies on the near side: its face normal opposes the ray
    fv = v.astype(np.float64)[f[r["face"]]]
    n = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0])
    assert ((n * d.astype(np.float64)).sum(1) < 0).all()
    # the sphere with the doubled seam: only rays aimed at the seam itself can leak
    raw = walked_seam_sphere(o, d)
    leak = np.abs(raw["t"] - 1.0) > 1e-6
    print("doubled seam: %d of %d rays leak, at t = %s" % (leak.sum(), leak.size, np.round(raw["t"][leak], 3).tolist()))
    on_seam = (np.abs(target[:, 1]) < 1e-6) & (target[:, 0] > 0)
    assert not (leak & ~on_seam).any() and np.isfinite(raw["t"]).all()


def walked_seam_sphere(o, d):
    return R.walk(o, d, tree_of("lat-long sphere"))


# ---- pruning -------------------------------------------------------------------------------------------------------------------------

def sphere_view(res):
    """a 48 x 64 camera outside the marching-cubes sphere: (c2w, intrinsics, size)"""
    return R.look_at((1.6, 0.9, 0.7), (0.0, 0.0, 0.0)), (70.0, 70.0, 31.5, 23.5), (48, 64)


def test_camera_rays_test_a_small_share_of_the_faces():
    v, f = cases()["MC sphere 32"][:2]
    tree = tree_of("MC sphere 32")
    c2w, K, size = sphere_view(32)
    o, d = R.camera_rays(c2w, K, size)
    w = R.walk(o, d, tree)
    hits = np.isfinite(w["t"])
    print("32^3 sphere, %d faces, %d camera rays, %d hit: %.2f faces tested and %.1f nodes visited per ray (brute force: %d)"
          % (tree.n_usable, hits.size, hits.sum(), w["tested"].mean(), w["nodes"].mean(), tree.n_usable))
    assert hits.sum() > hits.size // 4
    assert w["tested"].mean() < tree.n_usable / 20
    same_answer(w, R.brute(o, d, tree), "camera rays")


# ---- against the rasteriser -------------------------------------------------------------------------------------------------------

# Where the ray cast and the rasteriser are compared face by face, pixels whose hit lies within this barycentric distance of an edge
# are left out: the rasteriser decides coverage on vertices snapped to 1/256 pixel, so next to an edge it may name the neighbour.
# A vertex moves by up to 1/256 pixel (half a unit of snap per axis and the projection error, twice over for the two ends of an
# edge); the faces of the 32^3 sphere are about 2 pixels across in the view used, so an edge moves by about 2^-9 of a face: the margin
# is twice that.  Checked with the two numpy oracles alone (test_the_two_oracles_agree_on_the_sphere_away_from_edges): they agree on
# every remaining pixel (in this view, on every hit pixel even without a margin), and it leaves out 1.9 % of them; the cap is 20 %.
FACE_MARGIN = 2.0 ** -8


@functools.lru_cache(maxsize=None)
def room_case():
    """(mesh, c2w, intrinsics, size, closed-form depth [H, W], straddles [12]) of a camera inside a box room of 12 faces, looking
    along +x with axis-aligned axes (so camera-space z = 1 survives the rounding of the directions and t is the z-depth exactly).
    The closed form: a ray from inside a box leaves it at the least positive (wall_k - o_k) / d_k, in float64 on the fp32 ray.
    ``straddles``: the faces with a vertex behind the camera, which the rasteriser drops whole."""
    lo, hi = np.array([-2.0, -1.5, -1.0]), np.array([2.0, 1.5, 1.0])
    v, f = P.box_mesh(tuple(lo), tuple(hi))
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = (0, -1, 0), (0, 0, -1), (1, 0, 0), (0.3, 0.2, 0.1)
    K, size = (30.0, 30.0, 31.5, 23.5), (48, 64)
    o, d = (x.astype(np.float64) for x in R.camera_rays(c2w, K, size))
    assert (d[:, 0] == 1.0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
    straddles = (v[f][:, :, 0] < 0.3).any(1)
    return {"verts": v, "faces": f}, c2w, K, size, t.min(1).reshape(size), straddles


def test_the_oracle_gives_the_closed_form_depth_inside_the_room():
    mesh, c2w, K, size, want, straddles = room_case()
    assert straddles.sum() == 10
    o, d = R.camera_rays(c2w, K, size)
    r = R.walk(o, d, R.Tree(mesh["verts"], mesh["faces"]), tmin=0.01)
    assert (r["face"] >= 0).all() and (np.abs(r["t"] - want.reshape(-1)) <= 1e-12 * want.reshape(-1)).all()
    assert straddles[r["face"]].mean() > 0.3


def raster_depth_bound(mesh, c2w, K, face, depth, exact):
    """Section 12's bound on |rasterised depth - exact| per pixel, for pixels that show ``face``:
        depth * exact * (|d(1/z)/di| + |d(1/z)/dj|) * s  +  depth * r
    with the slopes of the face's plane on the screen (1/z = n . (x, y, 1) / (n . A) in camera space, x = (i - cx) / fx), s the
    largest snap_bound_units of its vertices over 256 plus 2^-18 pixel for the fp32 rounding of the ray's direction (2^-24 of at most
    64 pixels), and r the roundings between the vertices and the depth, 8 u + max_k 4 u m_2 / p_2 (tests/test_mesh_render_cpu.py)."""
    v, f = mesh["verts"].astype(np.float64), mesh["faces"][face]
    M = rr.w2c_rows(c2w)[0]
    cam = v @ M[:, :3].astype(np.float64).T + M[:, 3].astype(np.float64)
    A, B, C = cam[f[:, 0]], cam[f[:, 1]], cam[f[:, 2]]
    n = np.cross(B - A, C - A)
    c = (n * A).sum(1)
    slope = np.abs(n[:, 0] / (c * K[0])) + np.abs(n[:, 1] / (c * K[1]))
    (bx, by), _ = rr.snap_bound_units(mesh["verts"], M, K)
    s = np.maximum(bx, by)[f].max(1) / 256.0 + 2.0 ** -18
    r = 8 * 2.0 ** -24 + rr.depth_term_rel(mesh["verts"], M)[f].max(1)
    return depth * exact * slope * s + depth * r


def test_the_two_oracles_agree_on_the_sphere_away_from_edges():
    v, f = cases()["MC sphere 32"][:2]
    mesh = {"verts": v, "faces": f}
    c2w, K, (H, W) = sphere_view(32)
    zb, _ = rr.raster(v, f, rr.w2c_rows(c2w), np.float32([K]), H, W, np.float32(0.01))
    img = rr.resolve(v, f, rr.w2c_rows(c2w), np.float32([K]), np.float32(0.01), zb)
    rf, rd = img["face_id"][0].reshape(-1), img["depth"][0].reshape(-1).astype(np.float64)
    o, d = R.camera_rays(c2w, K, (H, W))
    r = R.walk(o, d, tree_of("MC sphere 32"), tmin=0.01)
    hit = r["face"] >= 0
    least = np.where(hit[:, None], r["bary"], 0.0).min(1)
    smallest = 1.0
    for e in range(12, 1, -1):                                         # the smallest power of two that leaves the oracles in agreement
        inner = hit & (least > 2.0 ** -e)
        if np.array_equal(rf[inner], r["face"][inner]):
            smallest = 2.0 ** -e
            break
    out = (hit & ~(least > FACE_MARGIN)).sum()
    print("sphere view: %d pixels hit; the oracles agree on the face from a margin of %g on; FACE_MARGIN = %g leaves out %d (%.1f %%)"
          % (hit.sum(), smallest, FACE_MARGIN, out, 100.0 * out / hit.sum()))
    assert smallest <= FACE_MARGIN and out <= 0.2 * hit.sum()
    inner = hit & (least > FACE_MARGIN)
    err = np.abs(rd[inner] - r["t"][inner])
    bound = raster_depth_bound(mesh, c2w, K, r["face"][inner], rd[inner], r["t"][inner])
    print("sphere view: largest |rasterised - ray-cast depth| %.3e, largest share of Section 12's bound %.3f" % (err.max(), (err / bound).max()))
    assert (err <= bound).all()


# ---- argument checks ------------------------------------------------------------------------------------------------------------------

def test_python_argument_errors():
    from nicer_slam_amd import mesh_raycast, mesh_render
    mesh = {"verts": np.zeros((3, 3), np.float32), "faces": np.zeros((1, 3), np.int32)}
    o = np.zeros((2, 3), np.float32)
    for kw in (dict(cull="left"), dict(tmin=math.nan), dict(tmax=math.nan)):
        with pytest.raises(ValueError):
            mesh_raycast.cast_rays(mesh, o, o, **kw)
    with pytest.raises(ValueError):
        mesh_raycast.cast_rays(mesh, o, np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        mesh_raycast.occluded(mesh, o, o, rel=1.5)
    with pytest.raises(ValueError):
        mesh_raycast.camera_rays(np.eye(4), (1.0, 1.0, 0.0, 0.0), (0, 4))
    with pytest.raises(ValueError):
        mesh_raycast.render_depth(mesh, np.eye(4), (1.0, 1.0, 0.0, 0.0), (4, 4), channels=("depth", "colour"))
    for fn in (mesh_render.visible_faces, mesh_render.cull_mesh):
        with pytest.raises(ValueError):
            fn(mesh, np.eye(4), (1.0, 1.0, 0.0, 0.0), (4, 4), method="zbuffer")
    with pytest.raises(ValueError):
        mesh_render.depth_l1(mesh, np.zeros((4, 4), np.float32), np.eye(4), (1.0, 1.0, 0.0, 0.0), method="zbuffer")
    o, d = mesh_raycast.camera_rays(np.eye(4), (2.0, 4.0, 1.0, 1.0), (2, 3))
    assert o.shape == (6, 3) and d.dtype == np.float32
    assert np.array_equal(d, np.float32([[-0.5, -0.25, 1], [0, -0.25, 1], [0.5, -0.25, 1], [-0.5, 0, 1], [0, 0, 1], [0.5, 0, 1]]))
    c2w = R.look_at((1.6, 0.9, 0.7), (0, 0, 0))
    for px in (None, np.array([[3, 1], [0, 0], [5, 4]])):
        got, want = mesh_raycast.camera_rays(c2w, (70.0, 70.0, 31.5, 23.5), (48, 64), px), R.camera_rays(c2w, (70.0, 70.0, 31.5, 23.5),
                                                                                                          (48, 64), px)
        same_bits(got[0], want[0], "origins")
        same_bits(got[1], want[1], "dirs")
    for argv in (["m.ply", "--poses", "p.npy", "--intrinsics", "1", "1", "0", "0", "--size", "0", "4", "--out", "d"],
                 ["m.ply", "--poses", "p.npy", "--intrinsics", "1", "1", "0", "0", "--size", "4", "4"]):
        with pytest.raises(SystemExit):
            mesh_raycast.parse_args(argv)


def test_section17_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib, EXPORTS
    NSA_EBADARG = 4
    for name in ("nsa_tri_ray_workspace", "nsa_tri_ray_build", "nsa_tri_ray_cast"):
        assert name in EXPORTS
    assert lib.nsa_tri_ray_workspace(0) == 0 and lib.nsa_tri_ray_workspace(1 << 31) == 0
    for F in (1, 8, 9, 12, 2304, 707336, (1 << 31) - 1):                               # the header's formula, with its roundings
        assert 0 < lib.nsa_tri_ray_workspace(F) <= R.workspace_bound(F) + 12 * 256
        assert lib.nsa_tri_ray_workspace(F) >= R.workspace_bound(F)
    fake = ctypes.c_void_p(4096)                          # never dereferenced: every call below is rejected before a launch
    b = dict(v=fake, V=8, f=fake, F=4, t=fake)
    for key, val in (("v", None), ("f", None), ("t", None), ("V", 0), ("V", 1 << 31), ("F", 1 << 31)):
        x = dict(b, **{key: val})
        assert lib.nsa_tri_ray_build(x["v"], x["V"], x["f"], x["F"], x["t"], None, None) == NSA_EBADARG, key
    assert lib.nsa_tri_ray_build(None, 8, None, 0, None, None, None) == 0                # no face: nothing to do
    s = dict(tree=fake, v=fake, V=8, f=fake, F=4, o=fake, d=fake, M=5, tmin=0.0, tmax=math.inf, flags=0, t=fake, face=fake)

    def cast(x):
        return lib.nsa_tri_ray_cast(x["tree"], x["v"], x["V"], x["f"], x["F"], x["o"], x["d"], x["M"], x["tmin"], x["tmax"], x["flags"],
                                    x["t"], x["face"], None, None, None, None)

    for key, val in (("tree", None), ("v", None), ("f", None), ("o", None), ("d", None), ("t", None), ("face", None), ("V", 0),
                     ("V", 1 << 31), ("F", 1 << 31), ("M", 1 << 31), ("tmin", math.nan), ("tmax", math.nan), ("flags", 6), ("flags", 16),
                     ("flags", 7)):
        assert cast(dict(s, **{key: val})) == NSA_EBADARG, key
    for flags in (0, 1, 2, 4, 8, 9, 13):
        assert cast(dict(s, M=0, o=None, d=None, t=None, face=None, flags=flags)) == 0    # no ray: nothing to do
        assert cast(dict(s, F=0, tree=None, f=None, flags=flags)) == 0                    # no face: nothing to do
    assert cast(dict(s, M=0, tmin=math.nan)) == NSA_EBADARG                               # ... but the window is checked first
