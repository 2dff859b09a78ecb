"""Mesh rasterisation and visibility without a GPU: the numpy oracle tests/raster_ref.py (include/nicer_slam_amd.h Section 12) against
the closed form of the analytic room, the properties the rule promises, argument validation of the entry points, and the host code of
nicer_slam_amd/mesh_render.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import raster_ref as rr
import tsdf_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEAR = 0.01
U = 2.0 ** -24


def _room_views(n_views=8, H=60, W=80, focal=50.0):
    poses = tsdf_ref.ring_poses(n_views)
    return poses, rr.w2c_rows(poses), tsdf_ref.shared_K4(H, W, focal), H, W, focal


def _render(mesh, w2c, K, H, W, **kw):
    zb, totals = rr.raster(mesh["verts"], mesh["faces"], w2c, K, H, W, NEAR, **kw)
    return zb, totals, rr.resolve(mesh["verts"], mesh["faces"], w2c, K, NEAR, zb, colours=mesh.get("colors"))


def test_room_against_closed_form():
    """Every pixel of the closed room is covered; face_id names the wall the closed form hits except where the pixel centre lies within
    one snapping unit of a seam; depth agrees with tsdf_ref.room_frames within the header's bound, every term computed, none chosen:
        depth * exact * (|d(1/z)/di| + |d(1/z)/dj|) * s  +  depth * r  +  |room_frames - its float64 restatement|
    s   how far the point whose exact 1/z the interpolation returns can lie from the pixel centre: sum_k l_k b_k with l_k the winning
        face's weights at the pixel and b_k its vertices' bounds on |X - 256 x_exact| (snap_bound_units: half a unit of snap plus the
        projection error, which grows with a vertex's distance from the image while its weight falls)
    r   the roundings between the vertices and the depth: 3 u per l_k (two conversions and a quotient), u + 4 u m_2 / p_2 per 1 / p_2k
        (depth_term_rel), u per product, 2 u for the two sums, u for the reciprocal: 8 u + max_k 4 u m_2 / p_2
    and the last term is the reference's own error: room_frames is an fp32 closed form, measured here against float64 (room_hit).
    At a seam pixel the winner may be the neighbouring wall, whose plane is then evaluated up to one unit + s past the seam: the first
    term with both walls' slopes and that distance.  Largest observed ratio to the bound (oracle alone, this scene): 0.909, recorded in DESIGN 4k."""
    n = 8            # no near-plane clipping: the walls are split finely enough that no face in the image reaches behind the camera
    mesh = rr.room_mesh(n)
    poses, w2c, K, H, W, focal = _room_views()
    zb, totals, img = _render(mesh, w2c, K, H, W)
    ref_depth, _ = tsdf_ref.room_frames(poses, H, W, focal)
    ref_depth = ref_depth.numpy()
    assert (img["face_id"] >= 0).all(), "a pixel of the closed room is not covered"
    jj, ii = np.mgrid[0:H, 0:W]
    worst = 0.0
    unit = 1.0 / 256
    for k in range(len(poses)):
        w, d, g = rr.room_hit(poses[k], K[0], ii, jj)
        ref_err = np.abs(d - ref_depth[k])
        assert ref_err.max() < 1e-5                                        # the two closed forms agree
        seam = np.zeros((H, W), dtype=bool)
        g_max = g.copy()
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                w2, _, g2 = rr.room_hit(poses[k], K[0], ii + di * 1.001 * unit, jj + dj * 1.001 * unit)
                seam |= w2 != w
                g_max = np.maximum(g_max, g2)
        got_wall = rr.wall_of_face(img["face_id"][k].astype(np.int64), n)
        assert (got_wall == w)[~seam].all(), f"view {k}: wrong wall away from every seam"
        assert seam.mean() < 0.02
        # the winning face's weights and its vertices' bounds at every pixel
        su = rr.Setup(mesh["verts"], mesh["faces"], w2c[k], K[0], NEAR)
        f = img["face_id"][k].astype(np.int64).reshape(-1)
        cov, again, ls = su.pixel(f, ii.reshape(-1), jj.reshape(-1))
        assert cov.all() and np.array_equal(again.view(np.uint32), img["depth"][k].reshape(-1).view(np.uint32))
        (bx, by), _ = rr.snap_bound_units(mesh["verts"], w2c[k], K[0])
        b_vert, r_vert = np.maximum(bx, by), rr.depth_term_rel(mesh["verts"], w2c[k])
        s = sum(l.astype(np.float64) * b_vert[vid[f]] for l, vid in zip(ls, su.vid)).reshape(H, W) * unit
        r = 8 * U + np.max([r_vert[vid[f]] for vid in su.vid], axis=0).reshape(H, W)
        depth = img["depth"][k].astype(np.float64)
        exact = ref_depth[k].astype(np.float64)
        bound = depth * exact * np.where(seam, 2 * g_max * (unit + s), g * s) + depth * r + ref_err
        err = np.abs(depth - exact)
        worst = max(worst, float((err / bound).max()))
        print(f"view {k}: max |depth - closed form| {err.max():.3e}, largest ratio to the bound {(err / bound).max():.3f}, "
              f"seam pixels {int(seam.sum())}, s up to {s.max() / unit:.4f} units, r up to {r.max() / U:.1f} u")
        assert (err <= bound).all(), f"view {k}: depth off by {(err / bound).max():.3f} times the bound"
    print(f"largest ratio to the depth bound: {worst:.3f}")
    assert int(totals[rr.OK]) + int(totals[rr.DEPTH]) + int(totals[rr.GUARD_FAIL]) + int(totals[rr.DEGENERATE]) == len(poses) * len(mesh["faces"])


def test_snapped_coordinates_against_float64_projection():
    """|X - 256 x_exact| stays within the header's derived bound (below 0.6 units inside this image) for every vertex in front of the camera."""
    mesh = rr.room_mesh(5)
    poses, w2c, K, H, W, _ = _room_views(8, 340, 600, 300.0)
    worst = 0.0
    for k in range(len(poses)):
        code, x, y, p2 = rr.project(w2c[k], K[0], NEAR, mesh["verts"])
        ok = code == rr.OK
        (bx, by), (xe, ye) = rr.snap_bound_units(mesh["verts"], w2c[k], K[0])
        ex, ey = np.abs(rr.snap(x) - 256.0 * xe)[ok], np.abs(rr.snap(y) - 256.0 * ye)[ok]
        assert ok.sum() > 20
        assert (ex <= bx[ok]).all() and (ey <= by[ok]).all()
        inside = (np.abs(xe - 300) < 300) & (np.abs(ye - 170) < 170)       # in the image the bound is half a unit and a little
        assert (bx[ok & inside] < 0.6).all() and (by[ok & inside] < 0.6).all()
        worst = max(worst, float((ex - 0.5).max()), float((ey - 0.5).max()))
    print(f"largest excess over half a unit: {worst:.5f} units")


def test_face_order_changes_ids_only_through_the_tie_rule():
    mesh = rr.room_mesh(3)
    poses, w2c, K, H, W, _ = _room_views(4)
    zb, _, img = _render(mesh, w2c, K, H, W)
    perm = np.random.default_rng(0).permutation(len(mesh["faces"]))
    zb2, _, img2 = _render(dict(verts=mesh["verts"], faces=mesh["faces"][perm]), w2c, K, H, W)
    assert np.array_equal(img["depth"].view(np.uint32), img2["depth"].view(np.uint32))
    back = perm[img2["face_id"]]                                  # the original index of the permuted winner
    differ = back != img["face_id"]
    # where the winners differ, two faces tie in depth at that pixel and each run chose its own smaller index
    assert differ.mean() < 0.01
    for k, j, i in np.argwhere(differ):
        s = rr.Setup(mesh["verts"], mesh["faces"], w2c[k], K[0], NEAR)
        f = np.array([img["face_id"][k, j, i], back[k, j, i]])
        cov, depth, _ = s.pixel(f, np.array([i, i]), np.array([j, j]))
        assert cov.all() and depth[0].view(np.uint32) == depth[1].view(np.uint32)
        assert f[0] < f[1] and np.flatnonzero(perm == f[1])[0] < np.flatnonzero(perm == f[0])[0]


def test_reversed_winding_renders_identically_and_backface_culling_is_complementary():
    mesh = rr.room_mesh(8)
    poses, w2c, K, H, W, _ = _room_views(4)
    for rev in (mesh["faces"][:, ::-1], mesh["faces"][:, [0, 2, 1]], mesh["faces"][:, [1, 0, 2]]):
        a = _render(mesh, w2c, K, H, W)[2]
        b = _render(dict(verts=mesh["verts"], faces=np.ascontiguousarray(rev)), w2c, K, H, W)[2]
        assert np.array_equal(a["face_id"], b["face_id"]) and np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
        assert np.array_equal(a["shade"].view(np.uint32), b["shade"].view(np.uint32))
    rev = np.ascontiguousarray(mesh["faces"][:, ::-1])
    full = _render(mesh, w2c, K, H, W)[0]
    front = rr.raster(mesh["verts"], mesh["faces"], w2c, K, H, W, NEAR, cull_backface=True)[0]
    back = rr.raster(mesh["verts"], rev, w2c, K, H, W, NEAR, cull_backface=True)[0]
    assert np.array_equal(np.minimum(front, back), full)                  # together they draw every face once ...
    both = (front != rr.EMPTY) & (back != rr.EMPTY)
    assert not (front[both] == back[both]).any()                          # ... and no face is drawn by both
    # the room's faces are wound to face inwards: with culling, the camera inside sees all of them, the reversed copy none
    assert (front != rr.EMPTY).all() and (back == rr.EMPTY).all()


def test_coincident_faces_resolve_to_the_smaller_index():
    mesh = rr.room_mesh(8)
    poses, w2c, K, H, W, _ = _room_views(3)
    faces = np.concatenate([mesh["faces"], np.roll(mesh["faces"], 1, axis=1)])        # every face twice, listed from another vertex
    img = _render(dict(verts=mesh["verts"], faces=faces), w2c, K, H, W)[2]
    assert (img["face_id"] >= 0).all() and (img["face_id"] < len(mesh["faces"])).all()
    assert np.array_equal(img["face_id"], _render(mesh, w2c, K, H, W)[2]["face_id"])


def test_shared_edge_is_covered_exactly_once():
    """Random triangle pairs on either side of a shared edge, on the plane z = 1 of an identity camera with fx = fy = 1, cx = cy = 0, so
    that screen coordinates are the vertex coordinates; vertices on a half-pixel lattice, so that many edges pass through centres."""
    rng = np.random.default_rng(1)
    M = np.eye(4, dtype=F32)[:3]
    K = np.array([1, 1, 0, 0], dtype=F32)
    H = W = 24
    on_edge = 0
    jj, ii = np.mgrid[0:H, 0:W]
    for _ in range(600):
        while True:
            P, Q, R, S = (rng.integers(0, 2 * W, size=2) * 0.5 for _ in range(4))
            o = lambda a, b, c: (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
            if o(P, Q, R) * o(P, Q, S) < 0:
                break
        verts = np.array([[*P, 1], [*Q, 1], [*R, 1], [*S, 1]], dtype=F32)
        order = rng.permutation(3)
        t1 = np.array([0, 1, 2])[order]
        t2 = np.array([1, 0, 3])[rng.permutation(3)]
        z1 = rr.raster(verts, t1[None], M[None], K[None], H, W, NEAR)[0][0] != rr.EMPTY
        z2 = rr.raster(verts, t2[None], M[None], K[None], H, W, NEAR)[0][0] != rr.EMPTY
        assert not (z1 & z2).any(), "a pixel centre is covered by both faces"
        # centres exactly on the open shared edge and strictly inside the other two edges of both triangles: covered exactly once
        c = (ii.astype(np.float64), jj.astype(np.float64))
        e = o(P, Q, c)
        sign1, sign2 = np.sign(o(P, Q, R)), np.sign(o(P, Q, S))
        in1 = (o(Q, R, c) * sign1 > 0) & (o(R, P, c) * sign1 > 0)
        in2 = (o(Q, S, c) * sign2 > 0) & (o(S, P, c) * sign2 > 0)
        shared = (e == 0) & in1 & in2
        on_edge += int(shared.sum())
        assert (z1 ^ z2)[shared].all(), "a pixel centre on the shared edge is covered by neither face"
        # and everything strictly inside either triangle is covered by it
        assert z1[(e * sign1 > 0) & in1].all() and z2[(e * sign2 > 0) & in2].all()
    assert on_edge > 100


def test_closed_room_any_equals_frustum_at_the_default_rel():
    """With no occluder every vertex inside a frustum is on the nearest surface: "any" must equal "frustum" on every face at every view.
    The default rel is the smallest power of two for which this holds with the oracle on these views (2^-7 leaves faces out)."""
    from nicer_slam_amd.mesh_render import DEFAULT_REL
    mesh = rr.room_mesh(6)
    smallest = None
    for H, W, focal in ((60, 80, 50.0), (45, 61, 30.0), (120, 160, 100.0)):
        poses, w2c, K, H, W, _ = _room_views(16, H, W, focal)
        zb = rr.raster(mesh["verts"], mesh["faces"], w2c, K, H, W, NEAR)[0]
        for k in range(len(poses)):
            fr = rr.visible(mesh["verts"], mesh["faces"], w2c[k:k + 1], K, H, W, NEAR, None, rr.FRUSTUM, 0.0)
            assert fr.any()
            for e in range(-12, 1):
                if np.array_equal(rr.visible(mesh["verts"], mesh["faces"], w2c[k:k + 1], K, H, W, NEAR, zb[k:k + 1], rr.ANY, 2.0 ** e), fr):
                    smallest = e if smallest is None else max(smallest, e)
                    break
            else:
                raise AssertionError("no rel <= 1 makes 'any' equal 'frustum'")
            got = rr.visible(mesh["verts"], mesh["faces"], w2c[k:k + 1], K, H, W, NEAR, zb[k:k + 1], rr.ANY, DEFAULT_REL)
            assert np.array_equal(got, fr), f"view {k} at {H} x {W}: {int((got != fr).sum())} faces differ"
    print(f"smallest power of two over these views: 2^{smallest}")
    assert 2.0 ** smallest == DEFAULT_REL


def test_slab_shadow_is_culled():
    """A slab between the camera and the wall x = +half: wall faces whose vertices all lie inside the slab's shadow by more than a pixel's
    footprint are dropped, faces with a vertex outside it by that margin (and inside the image) are kept, the slab's camera side is kept.
    The slab is sized so that the margin is exercised: its shadow's edge runs 1.5 footprints outside one line of the wall's vertex
    lattice (z) and 1.5 footprints inside another (y), so vertices 1.5 pixels from the edge decide faces on both sides."""
    from nicer_slam_amd.mesh_render import DEFAULT_REL
    n = 12
    room = rr.room_mesh(n)
    hx, hy, hz = tsdf_ref.ROOM_HALF
    H, W, focal = 120, 160, 100.0
    foot = hx / focal                                           # one pixel's footprint on the wall x = hx, seen from the origin
    front = 0.30
    s = hx / front                                              # the shadow of the slab's front face on that wall: scale hx / front
    edge_y = hy * 4 / 6 - 1.5 * foot                            # the lattice line y = hy * 4 / 6 is 1.5 footprints OUTSIDE the shadow
    edge_z = hz * 4 / 6 + 1.5 * foot                            # the lattice line z = hz * 4 / 6 is 1.5 footprints INSIDE it
    slab = rr.slab_mesh((front, -edge_y / s, -edge_z / s), (0.34, edge_y / s, edge_z / s))
    mesh = rr.merge(room, slab)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2] = [0, 0, -1], [0, 1, 0], [1, 0, 0]      # camera z along world +x
    K = tsdf_ref.shared_K4(H, W, focal)
    w2c = rr.w2c_rows(pose[None])
    zb = rr.raster(mesh["verts"], mesh["faces"], w2c, K, H, W, NEAR)[0]
    vis = rr.visible(mesh["verts"], mesh["faces"], w2c, K, H, W, NEAR, zb, rr.ANY, DEFAULT_REL).astype(bool)
    v = room["verts"].astype(np.float64)
    on_wall = np.isclose(v[:, 0], hx)
    deep = on_wall & (np.abs(v[:, 1]) < edge_y - foot) & (np.abs(v[:, 2]) < edge_z - foot)
    clear = on_wall & ((np.abs(v[:, 1]) > edge_y + foot) | (np.abs(v[:, 2]) > edge_z + foot))
    assert (deep | clear)[on_wall].all()                        # no vertex of this lattice sits inside the margin: every face is decided
    near_in = on_wall & deep & (np.abs(v[:, 2]) > edge_z - 2 * foot)
    near_out = on_wall & clear & (np.abs(v[:, 1]) < edge_y + 2 * foot) & (np.abs(v[:, 2]) < edge_z - foot)
    assert near_in.sum() >= 4 and near_out.sum() >= 4           # vertices within two footprints of the edge exist on both sides
    f = room["faces"]
    wall_faces = on_wall[f].all(1)
    dropped = wall_faces & deep[f].all(1)
    code, x, y, _ = rr.project(w2c[0], K[0], NEAR, room["verts"])
    inside = (code == rr.OK) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    seen_clear = wall_faces & (clear & inside)[f].any(1)
    assert inside[near_in].all() and inside[near_out].all()
    assert (dropped & near_in[f].any(1)).sum() >= 4 and (seen_clear & near_out[f].any(1) & ~(clear & inside & ~near_out)[f].any(1)).sum() >= 2
    assert not vis[:len(f)][dropped].any(), "a face inside the slab's shadow by more than a pixel's footprint survived"
    assert vis[:len(f)][seen_clear].all(), "a face outside the shadow by more than a pixel's footprint was dropped"
    slab_front = np.isclose(slab["verts"][slab["faces"]][:, :, 0], front).all(1)
    assert vis[len(f):][slab_front].all(), "the slab's camera side was dropped"


def test_argument_validation_needs_no_gpu():
    """Every Section 12 entry point rejects bad arguments before touching the device (none of these calls launches anything)."""
    from nicer_slam_amd._native import RasterViews, lib
    EBADARG = 4
    fake = ctypes.c_void_p(4096)                                  # never dereferenced

    def views(**kw):
        d = dict(w2c=4096, K=4096, n=1, K_per_view=0, H=48, W=64, near=0.01)
        d.update(kw)
        return ctypes.byref(RasterViews(d["w2c"], d["K"], d["n"], d["K_per_view"], d["H"], d["W"], d["near"]))

    assert lib.nsa_mesh_raster_workspace(0) == 16 and lib.nsa_mesh_raster_workspace(1000) == 16 + 16000

    def raster(v, verts=fake, V=8, faces=fake, F=12, points=None, P=0, size=1, ws=fake, zbuf=fake, totals=fake):
        return lib.nsa_mesh_raster(verts, V, faces, F, points, P, size, v, 0, 1, 256, ws, 0, zbuf, totals, None)

    assert raster(None) == EBADARG
    assert raster(views(w2c=None)) == EBADARG and raster(views(K=None)) == EBADARG
    assert raster(views(n=0)) == EBADARG and raster(views(H=0)) == EBADARG and raster(views(W=16385)) == EBADARG
    assert raster(views(near=0.0)) == EBADARG and raster(views(near=float("nan"))) == EBADARG and raster(views(near=-1.0)) == EBADARG
    assert raster(views(), verts=None) == EBADARG and raster(views(), faces=None) == EBADARG
    assert raster(views(), zbuf=None) == EBADARG and raster(views(), totals=None) == EBADARG and raster(views(), ws=None) == EBADARG
    assert raster(views(), P=4) == EBADARG                                   # points without their array
    assert raster(views(), points=fake, P=4, size=0) == EBADARG and raster(views(), points=fake, P=4, size=65) == EBADARG
    assert raster(views(), F=2 ** 31 - 2, points=fake, P=4) == EBADARG       # F + P must stay below 2^31

    def resolve(v, zbuf=fake, out=fake, palette=None, n_palette=0):
        return lib.nsa_mesh_raster_resolve(fake, 8, fake, 12, None, None, 0, palette, n_palette, v, zbuf, 1, out, None, None, None, None, None)

    assert resolve(None) == EBADARG and resolve(views(near=0.0)) == EBADARG
    assert resolve(views(), zbuf=None) == EBADARG and resolve(views(), out=None) == EBADARG      # no output asked for
    assert resolve(views(), n_palette=2) == EBADARG

    def visible(v, mode=0, rel=0.03, zbuf=fake, flags=fake, F=12):
        return lib.nsa_mesh_visible(fake, 8, fake, F, v, zbuf, mode, rel, flags, None)

    assert visible(None) == EBADARG and visible(views(H=0)) == EBADARG
    assert visible(views(), mode=3) == EBADARG and visible(views(), mode=-1) == EBADARG
    assert visible(views(), rel=-0.1) == EBADARG and visible(views(), rel=float("nan")) == EBADARG and visible(views(), rel=1.5) == EBADARG
    assert visible(views(), zbuf=None) == EBADARG and visible(views(), flags=None) == EBADARG
    assert visible(views(), F=0, flags=None) == 0                           # no faces: a no-op, not an error


def test_python_argument_errors_come_before_the_device():
    from nicer_slam_amd import mesh_render as mr
    mesh = rr.room_mesh(1)
    pose = np.eye(4)
    with pytest.raises(ValueError, match="channels"):
        mr.render_mesh(mesh, pose, (50, 50, 20, 20), (40, 40), channels=("depth", "albedo"))
    with pytest.raises(ValueError, match="mode"):
        mr.visible_faces(mesh, pose, (50, 50, 20, 20), (40, 40), mode="some")
    with pytest.raises(ValueError, match="rel"):
        mr.visible_faces(mesh, pose, (50, 50, 20, 20), (40, 40), rel=2.0)
    with pytest.raises(ValueError, match="viewpoint"):
        mr.fly_through(mesh, pose[None], viewpoint="above")


def test_cli_help_and_argument_errors():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.run([sys.executable, "-m", "nicer_slam_amd.mesh_render", *a], capture_output=True, text=True, env=env,
                                    cwd=ROOT, timeout=300)
    r = run("--help")
    assert r.returncode == 0 and "--cull" in r.stdout and "--depth-l1" in r.stdout and "--follow" in r.stdout
    r = run("mesh.ply", "--poses", "p.npy", "--intrinsics", "1", "1", "1", "1", "--size", "4", "4")
    assert r.returncode == 2 and "nothing to do" in r.stderr
    r = run("mesh.ply", "--poses", "p.npy", "--intrinsics", "1", "1", "1", "--size", "4", "4", "--out", "x")
    assert r.returncode == 2 and "--intrinsics" in r.stderr
    r = run("mesh.ply", "--poses", "p.npy", "--intrinsics", "1", "1", "1", "1", "--size", "4", "4", "--cull", "o.ply", "--rel", "3")
    assert r.returncode == 2 and "--rel" in r.stderr
    r = run("/nonexistent/mesh.ply", "--poses", "p.npy", "--intrinsics", "1", "1", "1", "1", "--size", "4", "4", "--cull", "o.ply")
    assert r.returncode == 2 and "mesh_render:" in r.stderr


def test_mesh_eval_cull_arguments():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.run([sys.executable, "-m", "nicer_slam_amd.mesh_eval", "a.ply", "b.ply", *a], capture_output=True, text=True,
                                    env=env, cwd=ROOT, timeout=300)
    r = run("--cull-poses", "p.npy")
    assert r.returncode == 2 and "--cull-intrinsics" in r.stderr
    r = run("--cull-size", "4", "4")
    assert r.returncode == 2 and "--cull-poses" in r.stderr


def test_pose_intrinsics_and_png_host_code(tmp_path):
    from PIL import Image
    from nicer_slam_amd import mesh_render as mr
    from nicer_slam_amd.tsdf import _intrinsics4, world_to_camera
    poses = tsdf_ref.ring_poses(5).astype(np.float64)
    np.save(tmp_path / "p.npy", poses)
    np.savetxt(tmp_path / "p.txt", poses.reshape(-1, 16), fmt="%.17e")
    os.makedirs(tmp_path / "seq")
    for k, P in enumerate(poses):
        np.savetxt(tmp_path / "seq" / f"frame-{k:06d}.pose.txt", P, fmt="%.17e")
    for src in ("p.npy", "p.txt", "seq"):
        assert np.array_equal(mr.read_poses(str(tmp_path / src)), poses), src
    with pytest.raises(ValueError):
        np.savetxt(tmp_path / "bad.txt", np.zeros((3, 5)))
        mr.read_poses(str(tmp_path / "bad.txt"))
    # depth directories: uint16 millimetre PNGs with both hole codes, or .npy frames in metres; too few frames is an error
    raw = (np.arange(6 * 8).reshape(6, 8) * 37 % 4000 + 200).astype(np.uint16)
    raw[0, 0], raw[1, 1] = 0, 65535
    os.makedirs(tmp_path / "png")
    os.makedirs(tmp_path / "npy")
    for k in range(3):
        Image.fromarray((raw + k).astype(np.uint16)).save(tmp_path / "png" / f"frame-{k:06d}.depth.png")
        np.save(tmp_path / "npy" / f"{k:04d}.npy", (raw + k).astype(np.float32) / 1000)
    d = mr.read_depth_dir(str(tmp_path / "png"), 2)
    want = np.stack([(raw + k).astype(np.float32) / np.float32(1000.0) for k in range(2)])
    want[0, 0, 0] = 0.0                                           # raw 0 is a hole (frame 1 holds 1 there: a millimetre)
    want[0, 1, 1] = 0.0                                           # 65535 is a hole; 65535 + 1 wrapped to 0 in frame 1: also a hole
    want[1, 1, 1] = 0.0
    assert d.dtype == np.float32 and np.array_equal(d, want)
    assert np.array_equal(mr.read_depth_dir(str(tmp_path / "npy"), 3)[2], (raw + 2).astype(np.float32) / 1000)
    with pytest.raises(ValueError, match="fewer than 4"):
        mr.read_depth_dir(str(tmp_path / "png"), 4)
    with pytest.raises(ValueError, match="no pose"):                # an empty pose stack is an argument error, found before the device
        mr.render_mesh(rr.room_mesh(1), np.zeros((0, 4, 4)), (50, 50, 20, 20), (40, 40))

    assert np.array_equal(world_to_camera(poses)[0], rr.w2c_rows(poses))
    K = tsdf_ref.pinhole(60, 80, 50.0)
    assert np.array_equal(_intrinsics4(K, 5), _intrinsics4((50.0, 50.0, 39.5, 29.5), 5))
    # PNG: 8-bit round trip
    img = np.linspace(0, 1, 12 * 7 * 3).reshape(12, 7, 3)
    mr.write_png(str(tmp_path / "a.png"), img)
    back = np.asarray(Image.open(tmp_path / "a.png"))
    assert back.shape == (12, 7, 3) and np.array_equal(back, np.rint(img * 255).astype(np.uint8))
    # the viewer of viz.py: 0.2 behind the pose along its z axis; scale removed from poses
    P = poses[2].copy()
    P[:3, :3] *= 1.7
    Q = mr.unscaled_pose(P)
    assert np.allclose(Q[:3, :3], poses[2][:3, :3]) and np.allclose(Q[:3, 3], P[:3, 3])
    B = mr.behind_first(Q)
    assert np.allclose(B[:3, 3], Q[:3, 3] - 0.2 * Q[:3, 2]) and np.allclose(B[:3, :3], Q[:3, :3])
    # the camera glyph: 12 segments of 100 points, apex at the centre, base at depth 1.5 * scale, inside the 2 x 2.4 outline
    pts, idx = mr.camera_actor(np.eye(4), scale=0.1, gt=True)
    assert pts.shape == (1200, 3) and (idx == 1).all()
    assert np.isclose(pts[:, 2].max(), 0.15) and np.isclose(np.linalg.norm(pts, axis=1).min(), 0.0)
    base = pts[np.isclose(pts[:, 2], 0.15)]
    assert np.isclose(base[:, 0].min(), -0.1) and np.isclose(base[:, 0].max(), 0.1) and np.isclose(base[:, 1].max(), 0.12)
    moved, _ = mr.camera_actor(poses[1], scale=0.1)
    assert np.allclose(moved, pts.astype(np.float64) @ poses[1][:3, :3].T + poses[1][:3, 3], atol=1e-6)
    tp, ti = mr.trajectory_points(poses, upto=4)
    assert np.array_equal(tp, poses[1:4, :3, 3].astype(np.float32)) and (ti == 0).all()
