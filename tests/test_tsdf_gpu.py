"""Depth fusion on the device (csrc/tsdf_fuse.hip, nicer_slam_amd/tsdf.py) against the numpy oracle tests/tsdf_ref.py: the volume bit
for bit, batching and culling invisible, the mesh chain, the 7-Scenes command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mc_ref
import tsdf_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bits(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][0]!r} vs {ref[bad][0]!r}"


def _volume(dims, origin, vl, trunc, color=True):
    from nicer_slam_amd.tsdf import TSDFVolume
    hi = [o + n * vl for o, n in zip(origin, dims)]
    vol = TSDFVolume(origin, hi, vl, trunc, color)
    assert vol.dims == tuple(dims)
    return vol


def _frames(n, H, W, focals, holes):
    """n frames of the analytic room (frame k with focal focals[k % len]); with ``holes`` every kind of missing measurement"""
    poses = tsdf_ref.ring_poses(n)
    depth, rgb = [], []
    for k in range(n):
        d, c = tsdf_ref.room_frames(poses[k:k + 1], H, W, focals[k % len(focals)])
        depth.append(d)
        rgb.append(c)
    depth, rgb = torch.cat(depth), torch.cat(rgb)
    if holes:
        depth[:, 3:7, 5:11] = 0.0
        depth[:, 10:12, 2:20] = float("nan")
        depth[:, H // 2:H // 2 + 3, W // 3:W // 2] = -0.3
        depth[0::2, -6:-2, -9:-1] = float("inf")
        depth[1::3, 1, :] = 0.0
    K4 = np.array([[f, f, (W - 1) / 2.0, (H - 1) / 2.0] for f in focals], dtype=np.float32)
    K4 = K4[np.arange(n) % len(focals)] if len(focals) > 1 else K4
    w2c = np.linalg.inv(poses.astype(np.float64))[:, :3, :].astype(np.float32)
    return poses, depth, rgb, K4, w2c


CASES = {
    # dims, origin, voxel, truncation, frames, (H, W), focals, holes, depth_trunc, colour
    "cubic": ((40, 40, 40), (-0.7, -0.7, -0.7), 0.035, 0.12, 16, (60, 80), (50.0,), False, np.inf, True),
    "odd-sizes-holes": ((37, 21, 70), (-0.66, -0.4, -0.7), 0.02, 0.07, 14, (48, 64), (40.0,), True, np.inf, True),
    "per-frame-K-depth-trunc": ((13, 50, 33), (-0.2, -0.6, -0.5), 0.03, 0.1, 15, (48, 64), (40.0, 55.0, 33.0), True, 0.55, True),
    "no-colour": ((21, 3, 65), (-0.65, -0.1, -0.66), 0.0203, 0.05, 12, (48, 64), (45.0, 38.0), True, 0.7, False),
    "beyond-the-room": ((30, 30, 30), (0.1, 0.0, 0.2), 0.05, 0.11, 12, (48, 64), (40.0,), False, np.inf, True),
    "thin-z": ((9, 11, 1), (-0.3, -0.3, 0.5), 0.06, 0.2, 8, (48, 64), (40.0,), False, np.inf, True),
    "thin-x": ((1, 1, 131), (0.4, 0.1, -0.66), 0.01, 0.04, 8, (48, 64), (40.0,), True, np.inf, True),
    "many-frames": ((20, 18, 40), (-0.66, -0.52, -0.6), 0.033, 0.1, 300, (24, 32), (20.0,), True, np.inf, True),
}


def _run_case(name, batch=None):
    dims, origin, vl, trunc, n, (H, W), focals, holes, depth_trunc, colour = CASES[name]
    poses, depth, rgb, K4, w2c = _frames(n, H, W, focals, holes)
    vol = _volume(dims, origin, vl, trunc, colour)
    vol.integrate(depth, rgb if colour else None, poses, K4, depth_trunc, batch or n)
    ref = tsdf_ref.integrate_volume(dims, vol.origin, vol.voxel_length, vol.sdf_trunc, depth.numpy(), rgb.numpy() if colour else None,
                                    w2c, K4, depth_trunc)
    return vol, ref


@pytest.mark.parametrize("name", list(CASES))
def test_volume_equals_the_oracle_bit_for_bit(name):
    """tsdf, weight and colour at EVERY voxel: cubic and non-cubic volumes, sizes that are no multiple of the brick (4 x 8 x 32) or of
    64, voxels behind the cameras (they stand inside the volume), outside every frustum and beyond the walls, frames with holes (0,
    NaN, negative, beyond depth_trunc, +inf), shared and per-frame intrinsics, with and without colour, more frames than one chunk of
    256."""
    vol, (ts, wt, col) = _run_case(name)
    assert 0 < (wt > 0).sum() < wt.size or name.startswith("thin")
    assert wt.max() >= 2 or name.startswith("thin")
    _assert_bits(vol.weight.cpu().numpy(), wt, f"{name}: weight")
    _assert_bits(vol.tsdf.cpu().numpy(), ts, f"{name}: tsdf")
    if col is not None:
        _assert_bits(vol.colour.cpu().numpy(), col, f"{name}: colour")
    else:
        assert vol.colour is None


def test_batching_is_invisible():
    """n frames in one call == n calls of one frame == any split into batches, bit for bit; two runs are bit-identical; device,
    host and numpy frames are the same frames; reset() gives a fresh volume."""
    name = "odd-sizes-holes"
    dims, origin, vl, trunc, n, (H, W), focals, holes, depth_trunc, colour = CASES[name]
    poses, depth, rgb, K4, w2c = _frames(n, H, W, focals, holes)
    K44 = tsdf_ref.pinhole(H, W, focals[0])
    outs = []
    vol = _volume(dims, origin, vl, trunc)
    for batch in (n, 1, 3, 2, n):
        vol.reset()
        vol.integrate(depth, rgb, poses, K4, depth_trunc, batch)
        outs.append([x.cpu().numpy().copy() for x in (vol.tsdf, vol.weight, vol.colour)])
    vol.reset()
    for k in range(n):                                                      # one frame per call, un-stacked, the 4 x 4 intrinsics
        vol.integrate(depth[k], rgb[k].reshape(H, W, 3), poses[k], K44)
    outs.append([x.cpu().numpy().copy() for x in (vol.tsdf, vol.weight, vol.colour)])
    vol.reset()
    vol.integrate(depth[:4].cuda(), rgb[:4].cuda(), torch.from_numpy(poses[:4]).cuda(), torch.from_numpy(K44).cuda())   # device frames
    vol.integrate(depth[4:].numpy(), rgb[4:].numpy(), poses[4:].astype(np.float64), tuple(float(x) for x in K4[0]))    # numpy frames
    outs.append([x.cpu().numpy().copy() for x in (vol.tsdf, vol.weight, vol.colour)])
    assert outs[0][1].max() >= 3
    for o in outs[1:]:
        for a, b, what in zip(o, outs[0], ("tsdf", "weight", "colour")):
            _assert_bits(a, b, what)
    vol.reset()
    assert float(vol.weight.abs().max()) == 0.0 and float(vol.tsdf.abs().max()) == 0.0 and float(vol.colour.abs().max()) == 0.0


def _border_indices(g, count, dims, origin, vl, trunc, poses, depth, K4, H, W):
    """flat voxel indices within two voxels of a frustum plane of some frame (a point on the plane u_f = 0, u_f = W, v_f = 0 or v_f = H
    at a random depth) or of its truncation band (a pixel's measured depth plus sdf_trunc along the camera axis), float64"""
    m = 6 * count
    k = g.integers(0, len(poses), m)
    kind = g.integers(0, 5, m)
    fx, fy, cx, cy = (K4[0, j] for j in range(4))
    u = g.uniform(-0.5, W - 0.5, m)
    v = g.uniform(-0.5, H - 0.5, m)
    u = np.where(kind == 0, -0.5, np.where(kind == 1, W - 0.5, u))
    v = np.where(kind == 2, -0.5, np.where(kind == 3, H - 0.5, v))
    z = g.uniform(0.02, 1.3, m)
    ui, vi = np.clip(np.rint(u), 0, W - 1).astype(np.int64), np.clip(np.rint(v), 0, H - 1).astype(np.int64)
    band = kind == 4
    u, v = np.where(band, ui, u), np.where(band, vi, v)
    z = np.where(band, depth[k, vi, ui].astype(np.float64) + trunc, z)
    cam = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
    P = poses.astype(np.float64)[k]
    world = np.einsum("mij,mj->mi", P[:, :3, :3], cam) + P[:, :3, 3]
    idx = np.floor((world - np.asarray(origin)) / vl).astype(np.int64) + g.integers(-2, 3, (m, 3))
    ok = ((idx >= 0) & (idx < np.asarray(dims))).all(1)
    idx = idx[ok][:count]
    assert len(idx) == count
    return (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]


def test_culling_is_invisible_at_size():
    """512^3 voxels, 48 frames of 480 x 640 of the analytic room in batches of 16: 10^6 voxel indices, half drawn uniformly and half
    within two voxels of some frame's frustum planes or of its truncation band, equal to the per-index oracle bit for bit."""
    n, H, W, focal, N = 48, 480, 640, 400.0, 512
    vl = 1.44 / N
    dims, origin, trunc = (N, N, N), (-0.72, -0.72, -0.72), 4 * vl
    poses = tsdf_ref.ring_poses(n)
    depth, rgb = tsdf_ref.room_frames(poses, H, W, focal, device="cuda")
    K4 = tsdf_ref.shared_K4(H, W, focal)
    vol = _volume(dims, origin, vl, trunc)
    vol.integrate(depth, rgb, poses, K4, batch=16)
    depth_h, rgb_h = depth.cpu().numpy(), rgb.cpu().numpy()
    g = np.random.default_rng(20)
    flat = np.concatenate([g.integers(0, N ** 3, 500000),
                           _border_indices(g, 500000, dims, vol.origin, vol.voxel_length, vol.sdf_trunc, poses, depth_h, K4, H, W)])
    w2c = np.linalg.inv(poses.astype(np.float64))[:, :3, :].astype(np.float32)
    ts, wt, col = tsdf_ref.integrate(flat, dims, vol.origin, vol.voxel_length, vol.sdf_trunc, depth_h, rgb_h, w2c, K4)
    sel = torch.from_numpy(flat).cuda()
    print(f"512^3: observed {float((wt > 0).mean()):.3f} of the sampled voxels, weight up to {wt.max():.0f}, "
          f"{int((wt[500000:] > 0).sum())} observed among the border voxels")
    assert 0.05 < (wt[500000:] > 0).mean() < 0.999 and wt.max() >= 4
    _assert_bits(vol.weight.reshape(-1)[sel].cpu().numpy(), wt, "weight")
    _assert_bits(vol.tsdf.reshape(-1)[sel].cpu().numpy(), ts, "tsdf")
    _assert_bits(vol.colour.reshape(3, -1)[:, sel].t().cpu().numpy(), col, "colour")


def test_mesh_chain(tmp_path):
    """extract_mesh on the analytic-room volume (96^3 voxels of 0.015, 16 frames of 120 x 160) == tests/mc_ref on the oracle volume
    (faces and vertices exactly, normals to 1e-6, as tests/test_mesh_gpu.py holds marching cubes); every vertex within one voxel
    length of the box; vertex colours against the float64 lookup; write_ply -> read_ply -> mesh_metrics against the 12-triangle box.

    Colour bound, per vertex and channel:  12 * dg * S / D + 32 * 2^-24,  where
      dg = 3 * 2^-24 * 96: the device forms the grid coordinate g = (p - origin) / voxel_length - 0.5 in fp32 from the same fp32
           vertex -- three roundings (difference, quotient, difference), each at most half an ulp of a value below 96 voxels; the
           fraction f = g - floor(g) is then exact, and the lookup is continuous where floor(g) flips;
      S  = the largest colour difference between two observed voxels of one 2 x 2 x 2 cell of the fixture (measured on the oracle's
           volume, an input of this comparison).  With colours taken relative to one corner, a shift of f_a by dg moves the
           numerator sum(w m (c - c0)) by at most 2 dg S and the denominator D = sum(w m) by at most 2 dg per axis, so the ratio
           moves by at most 3 * (2 dg S + 2 dg S) / D;
      D  = the surviving weight sum of the vertex in the float64 lookup (close to 1: a vertex lies on an edge between two observed
           voxels);
      32 * 2^-24: the eight-term fp32 sums and the division (three roundings per corner weight, one per product, seven per sum,
           one for the quotient: below 32 half-ulps of a value of at most 1)."""
    from nicer_slam_amd.inference import read_ply, write_ply
    from nicer_slam_amd.mesh_eval import mesh_metrics
    poses = tsdf_ref.ring_poses(16)
    ts, wt, col, origin, vl, depth, rgb = tsdf_ref.fuse_room(poses)
    vol = _volume((96,) * 3, origin, vl, 4 * vl)
    vol.integrate(depth, rgb, poses, tsdf_ref.pinhole(120, 160, 100.0))
    _assert_bits(vol.tsdf.cpu().numpy(), ts, "tsdf")
    _assert_bits(vol.weight.cpu().numpy(), wt, "weight")
    mesh = vol.extract_mesh()
    ref = mc_ref.marching_cubes(np.where(wt >= 1, ts, np.nan).astype(np.float32), 0.0, (vol.voxel_length,) * 3, vol.centre0)
    assert ref["verts"].shape[0] > 10000
    for k in ("verts", "normals", "faces"):
        assert tuple(mesh[k].shape) == ref[k].shape, k
    np.testing.assert_array_equal(mesh["faces"].cpu().numpy(), ref["faces"])
    np.testing.assert_array_equal(mesh["verts"].cpu().numpy(), ref["verts"])
    np.testing.assert_allclose(mesh["normals"].cpu().numpy(), ref["normals"], rtol=0, atol=1e-6)
    dist = tsdf_ref.box_distance(ref["verts"]) / vl
    assert dist.max() < 1.0
    # vertex colours
    want, D = tsdf_ref.sample_colour64(ref["verts"], wt, col, vol.origin, vol.voxel_length)
    seen = wt > 0
    big, small = np.full(wt.shape, -np.inf), np.full(wt.shape, np.inf)
    S = 0.0
    for c in range(3):
        lo, hi = np.where(seen, col[c], np.inf), np.where(seen, col[c], -np.inf)
        cmin, cmax = np.full((95,) * 3, np.inf), np.full((95,) * 3, -np.inf)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    cmin = np.minimum(cmin, lo[dx:dx + 95, dy:dy + 95, dz:dz + 95])
                    cmax = np.maximum(cmax, hi[dx:dx + 95, dy:dy + 95, dz:dz + 95])
        S = max(S, float(np.where(np.isfinite(cmax - cmin), cmax - cmin, 0.0).max()))
    assert 0.0 < S < 1.0 and D.min() > 0.5
    bound = 12 * (3 * 2.0 ** -24 * 96) * S / D + 32 * 2.0 ** -24
    err = np.abs(mesh["colors"].cpu().numpy().astype(np.float64) - want)
    print(f"vertex colours: S {S:.3f}, D min {D.min():.3f}, bound max {bound.max():.2e}, error max {err.max():.2e}")
    assert (err <= bound[:, None]).all()
    assert want.std() > 0.05
    # an unobserved neighbourhood has no colour; a point at a voxel centre has that voxel's
    far = torch.tensor([[5.0, 5.0, 5.0], [float("nan"), 0.0, 0.0]], device="cuda")
    assert float(vol.sample_colour(far).abs().max()) == 0.0
    ix = np.argwhere(seen)[::997]
    centres = np.stack(tsdf_ref.voxel_centres((ix[:, 0] * 96 + ix[:, 1]) * 96 + ix[:, 2], (96,) * 3, vol.origin, vol.voxel_length), -1)
    at = vol.sample_colour(torch.from_numpy(centres).cuda()).cpu().numpy()
    np.testing.assert_allclose(at, col[:, ix[:, 0], ix[:, 1], ix[:, 2]].T, rtol=0, atol=2e-4)
    # PLY round trip and the mesh metrics against the true room
    path = str(tmp_path / "room.ply")
    write_ply(path, mesh)
    back = read_ply(path)
    np.testing.assert_array_equal(back["verts"], ref["verts"])
    np.testing.assert_array_equal(back["faces"], ref["faces"])
    assert back["colors"].shape == ref["verts"].shape
    m = mesh_metrics(back, tsdf_ref.box_mesh(), align=False)
    print(f"mesh metrics: accuracy {m['accuracy']:.5f} completion {m['completion']:.5f} (voxel {vl})")
    assert m["accuracy"] < vl


def test_command_line_fuses_a_7scenes_directory(tmp_path):
    """python -m nicer_slam_amd.tsdf in a fresh child process on a three-frame 7-Scenes directory written here: the PLY reads back and
    equals fuse_7scenes called in-process."""
    from nicer_slam_amd.inference import read_ply, write_ply
    from nicer_slam_amd.tsdf import fuse_7scenes
    seq = str(tmp_path / "seq")
    tsdf_ref.write_7scenes_dir(seq)
    out = str(tmp_path / "cli.ply")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "nicer_slam_amd.tsdf", seq, "--out", out, "--voxel", "0.004", "--trunc", "0.02"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = read_ply(out)
    mesh = fuse_7scenes(seq, voxel_length=0.004, sdf_trunc=0.02)
    assert mesh["verts"].shape[0] > 100
    here = str(tmp_path / "here.ply")
    write_ply(here, mesh)
    want = read_ply(here)
    for k in ("verts", "normals", "faces", "colors"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    two = fuse_7scenes(seq, frames=2, voxel_length=0.004, sdf_trunc=0.02)
    assert 0 < two["verts"].shape[0] != mesh["verts"].shape[0]
