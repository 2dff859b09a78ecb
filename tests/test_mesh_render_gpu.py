"""Mesh rasterisation and visibility on the device (csrc/mesh_raster.hip, nicer_slam_amd/mesh_render.py) against the numpy oracle
tests/raster_ref.py: z-buffer, images, counts and visibility flags bit for bit; the two face paths, batching and repetition invisible;
a marching-cubes mesh at scale; the chain into TSDF fusion; culling and the mesh metrics; depth L1; the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_ref as rr
import tsdf_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 0.01
COMPARED_TOTALS = [0, 1, 2, 3, 4, 5, 6, 9, 10]            # [7], [8] describe the large-face queue, not the image


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    view = np.uint32 if got.dtype.itemsize == 4 else np.uint64 if got.dtype.itemsize == 8 else np.uint8
    bad = got.view(view) != ref.view(view)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}: {got[bad][0]!r} vs {ref[bad][0]!r}"


def _dirty_room(n=8):
    """the room with every kind of face the rule skips: NaN and infinite vertices, indices outside [0, V), degenerate faces"""
    m = rr.room_mesh(n)
    verts, faces, colors = m["verts"].copy(), m["faces"].copy(), m["colors"]
    V = len(verts)
    extra = np.array([[np.nan, 0.1, 0.2], [0.3, np.inf, 0.1], [0.1, 0.1, 0.1], [0.1, 0.1, 0.1]], dtype=np.float32)
    verts = np.concatenate([verts, extra])
    colors = np.concatenate([colors, np.full((4, 3), 0.5, np.float32)])
    bad = np.array([[0, 1, V], [0, V + 1, 2], [-1, 0, 1], [0, 1, V + 4], [2 ** 31 - 1, 0, 1], [3, 3, 4], [5, 6, 5], [V + 2, V + 3, 7],
                    [0, 1, 2 * (n + 1)]], dtype=np.int32)
    mid = [w * (n + 1) ** 2 + (n // 2) * (n + 1) + n // 2 for w in range(6)]          # a degenerate face in the middle of every wall
    bad = np.concatenate([bad, np.array([[c, c, c + 1] for c in mid], dtype=np.int32)])
    faces = np.concatenate([faces[:40], bad, faces[40:]])
    return dict(verts=verts, faces=faces, colors=colors)


def _views(n, H, W, per_view):
    poses = tsdf_ref.ring_poses(n)
    focals = [0.55 * W, 0.7 * W, 0.45 * W] if per_view else [0.6 * W]
    K = np.array([[f, f * 1.1, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5] for f in focals], dtype=np.float32)
    K = K[np.arange(n) % len(focals)] if per_view else K
    return poses, rr.w2c_rows(poses), K


def _points(seed, m=200):
    rng = np.random.default_rng(seed)
    p = (rng.random((m, 3)) * 2 - 1) * np.array([0.8, 0.7, 0.75])          # inside the room, in the walls and beyond them
    p[0] = np.nan
    idx = rng.integers(0, 3, size=m).astype(np.int32)                       # colour index 2 is outside the palette
    return p.astype(np.float32), idx


def _device_all(mesh, poses, K, H, W, points=None, batch=None, **kw):
    """(zbuf uint64 [n, H, W], totals [12], images dict, visibility dict) through the module's own scene"""
    from nicer_slam_amd import mesh_render as mr
    sc = mr._Scene(mesh, poses, K, (H, W), NEAR)
    pts, pidx = mr._points_arg(points, sc.dev)
    pal = torch.tensor(mr.PALETTE, dtype=torch.float32, device=sc.dev)
    zbuf, totals = sc.raster(0, sc.n, pts, 3, **kw)
    img = sc.resolve(0, sc.n, zbuf, mr.CHANNELS, True, pidx, pal)
    vis = {}
    for mode in ("any", "all", "frustum"):
        flags = torch.zeros(sc.faces.shape[0], dtype=torch.uint8, device=sc.dev)
        sc.visible(0, sc.n, zbuf if mode != "frustum" else None, mode, mr.DEFAULT_REL, flags)
        vis[mode] = flags.cpu().numpy()
    torch.cuda.synchronize()
    return _u64(zbuf), totals.cpu().numpy().astype(np.uint64), {k: v.cpu().numpy() for k, v in img.items()}, vis


def _oracle_all(mesh, w2c, K, H, W, points=None):
    from nicer_slam_amd import mesh_render as mr
    pts, pidx = (None, None) if points is None else points
    zb, totals = rr.raster(mesh["verts"], mesh["faces"], w2c, K, H, W, NEAR, points=pts, point_size=3)
    img = rr.resolve(mesh["verts"], mesh["faces"], w2c, K, NEAR, zb, colours=mesh.get("colors"), point_colour=pidx,
                     palette=np.array(mr.PALETTE, dtype=np.float32), n_points=0 if pts is None else len(pts), flip_to_camera=True)
    vis = {name: rr.visible(mesh["verts"], mesh["faces"], w2c, K, H, W, NEAR, zb, mode, mr.DEFAULT_REL)
           for name, mode in (("any", rr.ANY), ("all", rr.ALL), ("frustum", rr.FRUSTUM))}
    return zb, totals, img, vis


def _compare(dev, ref, what):
    zb, totals, img, vis = dev
    rzb, rtotals, rimg, rvis = ref
    _same_bits(zb, rzb, what + " zbuf")
    assert np.array_equal(totals[COMPARED_TOTALS], rtotals[COMPARED_TOTALS]), (what, totals, rtotals)
    for k, r in (("face_id", "face_id"), ("depth", "depth"), ("normal", "normal"), ("colour", "colour"), ("shaded", "shade")):
        _same_bits(img[k], rimg[r], f"{what} {k}")
    for mode in vis:
        assert np.array_equal(vis[mode], rvis[mode]), f"{what}: visibility '{mode}' differs on {int((vis[mode] != rvis[mode]).sum())} faces"


CASES = {
    # (H, W), views, per-view intrinsics, points
    "1x1": ((1, 1), 3, False, True),
    "odd-37x53": ((37, 53), 3, True, True),
    "one-view-60x80": ((60, 80), 1, False, False),
    "wide-33x129": ((33, 129), 3, True, True),
    "batch-32": ((45, 67), 32, True, True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_for_bit_against_the_oracle(name):
    (H, W), n, per_view, with_points = CASES[name]
    mesh = _dirty_room()
    poses, w2c, K = _views(n, H, W, per_view)
    points = _points(3) if with_points else None
    dev = _device_all(mesh, poses, K, H, W, points)
    ref = _oracle_all(mesh, w2c, K, H, W, points)
    assert ref[1][rr.BAD_INDEX] == 3 * n and ref[1][rr.DEPTH] > 0 and ref[1][rr.DEGENERATE] > 0      # the case has what it claims
    if H * W > 1000:
        assert (ref[2]["face_id"] >= 0).mean() > 0.9
    _compare(dev, ref, name)
    # the two face paths, a queue too small for its items, batching and repetition change nothing
    for kw in (dict(large_threshold=0), dict(large_threshold=0xFFFFFFFF), dict(large_threshold=0, queue_capacity=37),
               dict(large_threshold=16, queue_capacity=5)):
        other = _device_all(mesh, poses, K, H, W, points, **kw)
        _same_bits(other[0], dev[0], f"{name} zbuf with {kw}")
        assert np.array_equal(other[1][COMPARED_TOTALS], dev[1][COMPARED_TOTALS])
    again = _device_all(mesh, poses, K, H, W, points)
    _same_bits(again[0], dev[0], name + " second run")
    for k in range(n):
        one = _device_all(mesh, poses[k:k + 1], K[k:k + 1] if per_view else K, H, W, points)
        _same_bits(one[0][0], dev[0][k], f"{name} view {k} alone")
        for c in ("depth", "normal", "colour", "shaded"):
            _same_bits(one[2][c][0], dev[2][c][k], f"{name} view {k} alone, {c}")


def test_large_face_queue_is_used_and_counted():
    from nicer_slam_amd import mesh_render as mr
    mesh = tsdf_ref.box_mesh()
    _, _, K = _views(4, 340, 600, False)
    poses = np.stack([_look_at(e) for e in ((2.5, 1.0, 1.5), (-2.0, 0.5, 2.0), (0.5, 2.8, 0.4), (1.0, -1.0, -2.5))])      # outside: no face is cut by near
    sc = mr._Scene(mesh, poses, K, (340, 600), NEAR)
    z0, t0 = sc.raster(0, 4, large_threshold=0xFFFFFFFF)
    z1, t1 = sc.raster(0, 4, large_threshold=256)
    assert torch.equal(z0, z1)
    t0, t1 = t0.cpu().numpy(), t1.cpu().numpy()
    assert t0[7] == 0 and t0[8] == 0 and t1[7] > 0 and t1[8] >= t1[7]
    assert t0[6] == t1[6] and np.array_equal(t0[:6], t1[:6])
    zr, tr = rr.raster(mesh["verts"], mesh["faces"], rr.w2c_rows(poses), K, 340, 600, NEAR)
    _same_bits(_u64(z1), zr, "12-triangle box at 340 x 600")
    assert int(tr[6]) == int(t1[6])


def test_empty_mesh_and_points_alone():
    from nicer_slam_amd import mesh_render as mr
    H, W = 31, 47
    poses, w2c, K = _views(3, H, W, True)
    empty = dict(verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32))
    r = mr.render_mesh(empty, poses, K, (H, W), NEAR)
    assert (r["face_id"] == -1).all() and (r["depth"] == 0).all() and r["totals"]["drawn"] == 0 and r["totals"]["atomics"] == 0
    assert mr.visible_faces(empty, poses, K, (H, W)).shape == (0,)
    points = _points(5)
    dev = _device_all(empty, poses, K, H, W, points)
    ref = _oracle_all(empty, w2c, K, H, W, points)
    assert (ref[2]["face_id"] >= 0).any()
    _compare(dev, ref, "points alone")
    # vertices without faces
    lonely = dict(verts=rr.room_mesh(1)["verts"], faces=np.zeros((0, 3), np.int32))
    _compare(_device_all(lonely, poses, K, H, W, points), _oracle_all(lonely, w2c, K, H, W, points), "vertices without faces")


def _sphere_mesh(res, r, centre=(0.0, 0.0, 0.0)):
    from nicer_slam_amd import inference
    ax = torch.linspace(-1, 1, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r
    step = float(ax[1] - ax[0])
    m = inference.marching_cubes(vol.float().cuda(), 0.0, (step,) * 3, (-1.0,) * 3)
    return {k: v.cpu().numpy() for k, v in m.items()}


def _look_at(eye, target=(0.0, 0.0, 0.0)):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
    right = right / np.linalg.norm(right) if np.linalg.norm(right) > 1e-9 else np.array([1.0, 0.0, 0.0])
    down = np.cross(fwd, right)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = right, down, fwd, eye
    return P


def test_marching_cubes_sphere_at_scale():
    """A 128^3 sphere mesh at 340 x 600 from 8 poses (six outside, two inside): EVERY pixel equals the oracle (the oracle is fast enough
    for all of them, so the near-tie pixels are among those compared), and so do the visibility flags."""
    mesh = _sphere_mesh(128, 0.6)
    mesh["colors"] = (0.5 + 0.5 * np.sin(7.0 * mesh["verts"])).astype(np.float32)
    assert len(mesh["faces"]) > 50000
    H, W = 340, 600
    poses = np.stack([_look_at(e) for e in ((2.0, 0.1, 0.0), (-1.5, 0.5, 1.0), (0.0, 1.8, 0.3), (0.3, -2.0, 0.2), (1.0, 1.0, 1.2), (0.0, 0.2, -0.9),
                                           (0.1, 0.05, 0.0), (-0.2, 0.1, 0.3))])
    poses[6] = _look_at((0.1, 0.05, 0.0), (1.0, 0.3, 0.2))
    poses[7] = _look_at((-0.2, 0.1, 0.3), (-1.0, -0.4, 0.5))
    K = np.array([[300.0, 300.0, (W - 1) / 2.0, (H - 1) / 2.0]], dtype=np.float32)
    dev = _device_all(mesh, poses, K, H, W)
    ref = _oracle_all(mesh, rr.w2c_rows(poses), K, H, W)
    assert (ref[2]["face_id"] >= 0).mean() > 0.3
    _compare(dev, ref, "sphere 128^3")
    # near ties: pixels where two faces' depths differ by less than 2^-20 relative exist in this scene and are among the pixels compared
    print(f"atomics per view {int(dev[1][6]) / len(poses):.0f}, covered pixels {(ref[2]['face_id'] >= 0).mean():.3f}")


def _chain_metrics(depth, poses, H, W, focal):
    from nicer_slam_amd.mesh_eval import mesh_metrics
    from nicer_slam_amd.tsdf import TSDFVolume
    n_vox, vl = 96, 0.015
    lo = (-0.5 * n_vox * vl,) * 3
    vol = TSDFVolume(lo, tuple(-x for x in lo), vl, 4 * vl, color=False)
    vol.integrate(depth, None, poses, tsdf_ref.pinhole(H, W, focal))
    mesh = vol.extract_mesh()
    return mesh_metrics(mesh, tsdf_ref.box_mesh(), n_points=200000, seed=0, align=False)


def test_chain_rendered_depth_into_tsdf_fusion():
    """The room mesh's rendered depth from 16 ring poses at 120 x 160 fused by Section 10's settings (96^3 voxels of 0.015) and scored
    against the 12-triangle box, beside the same chain fed by the analytic depth of tsdf_ref.room_frames (the reference for this
    number).  Margin: twice the largest difference of the two depth sources in the CPU oracle at 60 x 80 -- half the size, so a pixel's
    footprint and with it the snap's effect on depth is twice as large.  Measured: see DESIGN 4k."""
    from nicer_slam_amd import mesh_render as mr
    poses = tsdf_ref.ring_poses(16)
    mesh = rr.room_mesh(8)
    h, w, f = 60, 80, 50.0
    zb, _ = rr.raster(mesh["verts"], mesh["faces"], rr.w2c_rows(poses), tsdf_ref.shared_K4(h, w, f), h, w, NEAR)
    small = rr.resolve(mesh["verts"], mesh["faces"], rr.w2c_rows(poses), tsdf_ref.shared_K4(h, w, f), NEAR, zb)["depth"]
    assert (small > 0).all()
    margin = 2.0 * float(np.abs(small.astype(np.float64) - tsdf_ref.room_frames(poses, h, w, f)[0].numpy()).max())
    H, W, focal = 120, 160, 100.0
    rendered = mr.render_mesh(mesh, poses, tsdf_ref.pinhole(H, W, focal), (H, W), NEAR, channels=("depth",))["depth"]
    analytic = tsdf_ref.room_frames(poses, H, W, focal)[0]
    assert (rendered > 0).all()
    print(f"depth sources: max difference at 60 x 80 (oracle) {margin / 2:.3e}, at 120 x 160 (device) "
          f"{float(np.abs(rendered.astype(np.float64) - analytic.numpy()).max()):.3e}")
    a = _chain_metrics(torch.from_numpy(rendered), poses, H, W, focal)
    b = _chain_metrics(analytic, poses, H, W, focal)
    for key in ("accuracy", "completion", "chamfer-L1"):
        print(f"{key}: rendered {a[key]:.6e}, analytic {b[key]:.6e}, difference {abs(a[key] - b[key]):.3e}, margin {margin:.3e}")
    for key in ("accuracy", "completion", "chamfer-L1"):
        assert abs(a[key] - b[key]) <= margin, (key, a[key], b[key], margin)


def test_culling_moves_the_metric_the_right_way():
    """gt: a sphere seen from inside.  rec: the same sphere plus a shell around it that no interior camera sees.  Culling rec to what six
    interior cameras (fields of view above 90 degrees, one per axis direction) saw gives back gt's visible part exactly, so its metrics
    equal gt's own; unculled, accuracy is at least the shell's share of the sampled area times its distance from gt.  The DIFFERENCE to
    the culled accuracy a is share x (distance - a): the sphere's own samples score a in both runs (their mean over the (1 - share) n
    samples of the unculled run within four sigma, sigma <= a / sqrt of that count, nearest-neighbour distances spreading no wider than
    their mean), the shell's samples score at least the distance instead of a.
    Both factors are computed from the meshes, nothing is allowed by eye:
      share     the shell's part of the total face area, less four sigma of the binomial count of 200000 area-weighted samples;
      distance  every point of a triangle with vertices at radius >= rho and edges <= L has radius >= sqrt(rho^2 - L^2 / 3)
                (|sum l_k v_k|^2 = sum l_k |v_k|^2 - sum_{k<m} l_k l_m |v_k - v_m|^2), every point of the inner mesh has at most
                its largest vertex radius: the gap between the two is the least distance of any shell sample to any gt sample."""
    from nicer_slam_amd import mesh_render as mr
    from nicer_slam_amd.mesh_eval import mesh_metrics
    gt = _sphere_mesh(64, 0.5)
    shell = _sphere_mesh(64, 0.8)
    rec = rr.merge(gt, shell)
    eye = (0.02, -0.01, 0.03)
    poses = np.stack([_look_at(eye, np.asarray(eye) + d) for d in np.concatenate([np.eye(3), -np.eye(3)])])
    size, K = (128, 128), (50.0, 50.0, 63.5, 63.5)
    vis = mr.visible_faces(rec, poses, K, size)
    assert vis[:len(gt["faces"])].all(), "an interior camera misses a face of the sphere it sits in"
    assert not vis[len(gt["faces"]):].any(), "a face of the outer shell counts as seen"
    culled = mr.cull_mesh(rec, poses, K, size)
    gt_visible = mr.cull_mesh(gt, poses, K, size)
    assert np.array_equal(culled["verts"], gt_visible["verts"]) and np.array_equal(culled["faces"], gt_visible["faces"])
    assert np.array_equal(culled["faces"], gt["faces"])                    # order kept
    a = mesh_metrics(culled, gt, align=False)
    b = mesh_metrics(gt_visible, gt, align=False)
    for key in ("accuracy", "completion", "chamfer-L1"):
        assert a[key] == b[key], key
    raw = mesh_metrics(rec, gt, align=False)
    def tri(m):
        return m["verts"].astype(np.float64)[m["faces"]]

    def area(m):
        t = tri(m)
        return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()

    t = tri(shell)
    longest = max(np.linalg.norm(t[:, k] - t[:, (k + 1) % 3], axis=1).max() for k in range(3))
    rho = np.linalg.norm(shell["verts"].astype(np.float64), axis=1).min()
    distance = np.sqrt(rho ** 2 - longest ** 2 / 3) - np.linalg.norm(gt["verts"].astype(np.float64), axis=1).max()
    share = area(shell) / (area(shell) + area(gt))
    n = 200000
    share_low = share - 4 * np.sqrt(share * (1 - share) / n)
    print(f"accuracy: culled {a['accuracy']:.5f}, unculled {raw['accuracy']:.5f}; shell share {share:.4f} (at least {share_low:.4f} of the "
          f"samples), distance {distance:.5f}, share x distance {share_low * distance:.5f}")
    assert 0.29 < distance < 0.3 and 0.70 < share_low < share < 0.73
    assert raw["accuracy"] >= share_low * distance
    assert raw["accuracy"] - a["accuracy"] >= share_low * (distance - a["accuracy"]) - 4 * a["accuracy"] / np.sqrt(n * (1 - share))
    # the same through mesh_metrics' own option (off by default: raw above is untouched by it)
    c = mesh_metrics(rec, gt, align=False, cull=dict(c2w=poses, intrinsics=K, size=size))
    assert c["accuracy"] == a["accuracy"] and abs(c["culled face fraction"] - len(shell["faces"]) / len(rec["faces"])) < 1e-12
    # "frustum" keeps the shell: only the depth test removes what lies behind a surface
    assert mr.visible_faces(rec, poses, K, size, mode="frustum")[len(gt["faces"]):].any()


def test_depth_l1():
    from nicer_slam_amd import mesh_render as mr
    mesh = rr.room_mesh(8)
    poses = tsdf_ref.ring_poses(5)
    H, W, focal = 60, 80, 50.0
    K = tsdf_ref.pinhole(H, W, focal)
    own = mr.render_mesh(mesh, poses, K, (H, W), NEAR, channels=("depth",))["depth"]
    l1, count = mr.depth_l1(mesh, own, poses, K, NEAR)
    assert l1 == 0.0 and count == 5 * H * W
    rng = np.random.default_rng(2)
    frames = (own.astype(np.float64) * (1 + 0.01 * rng.standard_normal(own.shape))).astype(np.float32)
    frames[:, 3:9, 5:20] = 0.0
    frames[1, 10:12] = np.nan
    frames[2, 30:33, 40:50] = -1.0
    ok = (own > 0) & np.isfinite(frames) & (frames > 0)
    want = np.abs(own.astype(np.float64) - frames.astype(np.float64))[ok]
    l1, count = mr.depth_l1(mesh, frames, poses, K, NEAR, batch=2)
    assert count == int(ok.sum())
    assert abs(l1 - want.sum() / count) <= 1e-12 * want.sum() / count + 1e-18      # float64 sums in two orders


def test_command_line(tmp_path):
    from PIL import Image
    from nicer_slam_amd.inference import read_ply, write_ply
    inner = _sphere_mesh(32, 0.5)
    rec = rr.merge(inner, _sphere_mesh(32, 0.8))
    rec["colors"] = (0.5 + 0.5 * np.sin(5.0 * rec["verts"])).astype(np.float32)
    rec["normals"] = np.zeros_like(rec["verts"])
    write_ply(str(tmp_path / "rec.ply"), {k: torch.from_numpy(v) for k, v in rec.items()})
    poses = np.stack([_look_at((0.05 * k, 0.02 * k, -0.03 * k), (1.0 - 0.4 * k, 0.2, 0.5 * k - 1.0)) for k in range(5)])
    np.save(tmp_path / "poses.npy", poses)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = ["timeout", "-k", "10", "240", sys.executable, "-m", "nicer_slam_amd.mesh_render", str(tmp_path / "rec.ply"), "--poses",
            str(tmp_path / "poses.npy"), "--intrinsics", "50", "50", "63.5", "63.5", "--size", "128", "128", "--viewer-size", "99", "176"]
    r = subprocess.run(base + ["--out", str(tmp_path / "fixed"), "--cull", str(tmp_path / "culled.ply"), "--gt-poses", str(tmp_path / "poses.npy")],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(tmp_path / "fixed"))
    assert files == [f"{k:06d}.png" for k in range(1, 6)]
    culled = read_ply(str(tmp_path / "culled.ply"))
    assert 0 < len(culled["faces"]) <= len(inner["faces"]) and "colors" in culled
    assert culled["verts"].shape[0] <= inner["verts"].shape[0]
    r = subprocess.run(base + ["--out", str(tmp_path / "follow"), "--follow"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    fixed = [np.asarray(Image.open(tmp_path / "fixed" / f)) for f in files]
    follow = [np.asarray(Image.open(tmp_path / "follow" / f)) for f in files]
    assert fixed[0].shape == (99, 176, 3)
    assert any((a != b).any() for a, b in zip(fixed[1:], follow[1:])), "the viewer does not follow"
    assert (fixed[0] != 255).any() and (fixed[0][..., 0] != fixed[0][..., 1]).any()      # something is drawn, and in colour
