"""Depth fusion without a device: argument validation of the two entry points, the numpy oracle (tests/tsdf_ref.py) on the analytic
room, the volume's size refusal, the bounding box of frames and the 7-Scenes reader."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mc_ref
import tsdf_ref

NSA_EBADARG = 4


def _desc(tsdf=4096, weight=4096, colour=4096, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), vl=0.1, trunc=0.3):
    from nicer_slam_amd._native import TsdfVolumeDesc
    return TsdfVolumeDesc(tsdf, weight, colour, dims[0], dims[1], dims[2], (ctypes.c_float * 3)(*origin), vl, trunc)


def test_argument_validation_needs_no_gpu():
    """Both entry points check their arguments before touching the device (the pointers below are never dereferenced)."""
    from nicer_slam_amd._native import lib
    fake = ctypes.c_void_p(4096)
    inf = float("inf")

    def integrate(desc, depth=fake, rgb=fake, w2c=fake, K=fake, per_frame=0, n=2, H=48, W=64, depth_trunc=inf, zmax=fake):
        return lib.nsa_tsdf_integrate(ctypes.byref(desc) if desc is not None else None, depth, rgb, w2c, K, per_frame, n, H, W,
                                      depth_trunc, zmax, None)

    assert integrate(None) == NSA_EBADARG
    assert integrate(_desc(tsdf=None)) == NSA_EBADARG
    assert integrate(_desc(weight=None)) == NSA_EBADARG
    assert integrate(_desc(dims=(0, 8, 8))) == NSA_EBADARG
    assert integrate(_desc(dims=(8, 8, 0))) == NSA_EBADARG
    assert integrate(_desc(dims=(2048, 2048, 513))) == NSA_EBADARG              # above 2^31 voxels
    assert integrate(_desc(dims=(1 << 31, 1 << 31, 1))) == NSA_EBADARG          # a product that overflows 64 bits' lower half
    assert integrate(_desc(dims=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))) == NSA_EBADARG
    for bad in (0.0, -1.0, inf, float("nan")):
        assert integrate(_desc(vl=bad)) == NSA_EBADARG
        assert integrate(_desc(trunc=bad)) == NSA_EBADARG
    assert integrate(_desc(trunc=1e-45)) == NSA_EBADARG                          # 1 / sdf_trunc overflows
    assert integrate(_desc(origin=(0.0, float("nan"), 0.0))) == NSA_EBADARG
    ok = _desc()
    assert integrate(ok, depth=None) == NSA_EBADARG
    assert integrate(ok, w2c=None) == NSA_EBADARG
    assert integrate(ok, K=None) == NSA_EBADARG
    assert integrate(ok, zmax=None) == NSA_EBADARG
    assert integrate(ok, rgb=None) == NSA_EBADARG                                # a volume with colour needs the frames' colour
    assert integrate(ok, H=0) == NSA_EBADARG
    assert integrate(ok, W=0) == NSA_EBADARG
    assert integrate(ok, W=1 << 24) == NSA_EBADARG
    assert integrate(ok, H=1 << 16, W=1 << 16) == NSA_EBADARG                    # H * W overflows
    for bad in (0.0, -1.0, float("nan")):
        assert integrate(ok, depth_trunc=bad) == NSA_EBADARG
    assert integrate(ok, depth=None, rgb=None, w2c=None, K=None, zmax=None, n=0) == 0      # no frames: a no-op
    assert integrate(_desc(vl=0.0), n=0) == NSA_EBADARG                          # ... of a valid volume

    def sample(desc, points=fake, m=5, out=fake):
        return lib.nsa_tsdf_sample_colour(ctypes.byref(desc) if desc is not None else None, points, m, out, None)

    assert sample(None) == NSA_EBADARG
    assert sample(_desc(colour=None)) == NSA_EBADARG
    assert sample(_desc(vl=float("nan"))) == NSA_EBADARG
    assert sample(_desc(dims=(2048, 2048, 513))) == NSA_EBADARG
    assert sample(ok, points=None) == NSA_EBADARG
    assert sample(ok, out=None) == NSA_EBADARG
    assert sample(ok, points=None, out=None, m=0) == 0


def test_oracle_meshes_the_analytic_room():
    """The rule itself, before any kernel: 16 frames of 120 x 160 of the closed-form box room fused by the oracle into 96^3 voxels of
    0.015 (truncation 4 voxels), meshed by tests/mc_ref on the NaN-masked volume.  Condition: EVERY vertex within one voxel length of
    the true box surface (closed-form point-to-box distance).  Measured with this fixture (ring_poses(16), focal 100): max 0.24,
    mean 0.046 voxel lengths over 25 357 vertices."""
    ts, wt, col, origin, vl = tsdf_ref.fuse_room(tsdf_ref.ring_poses(16))[:5]
    assert (wt > 0).mean() > 0.3 and col is not None and 0.0 < col[:, wt > 0].min() and col.max() < 1.0
    vol = np.where(wt >= 1, ts, np.nan).astype(np.float32)
    c0 = tuple(float(np.float32(o) + np.float32(vl) * np.float32(0.5)) for o in origin)
    mesh = mc_ref.marching_cubes(vol, 0.0, (vl,) * 3, c0)
    assert mesh["verts"].shape[0] > 10000
    dist = tsdf_ref.box_distance(mesh["verts"]) / vl
    print(f"analytic room: {mesh['verts'].shape[0]} vertices, distance to the box max {dist.max():.3f} mean {dist.mean():.3f} voxel lengths")
    assert dist.max() < 1.0


def test_oracle_batches_and_continues():
    """the oracle's own bookkeeping: continuing from a state equals one run over all frames"""
    poses = tsdf_ref.ring_poses(8)
    depth, rgb = tsdf_ref.room_frames(poses, 30, 40, 25.0)
    w2c = np.linalg.inv(poses.astype(np.float64))[:, :3, :].astype(np.float32)
    K4 = np.array([[25.0, 25.0, 19.5, 14.5]], dtype=np.float32)
    flat = np.arange(20 * 12 * 9)
    args = ((20, 12, 9), (-0.7, -0.5, -0.4), 0.07, 0.2)
    one = tsdf_ref.integrate(flat, *args, depth.numpy(), rgb.numpy(), w2c, K4)
    half = tsdf_ref.integrate(flat, *args, depth.numpy()[:3], rgb.numpy()[:3], w2c[:3], K4)
    two = tsdf_ref.integrate(flat, *args, depth.numpy()[3:], rgb.numpy()[3:], w2c[3:], K4, state=half)
    for a, b in zip(one, two):
        np.testing.assert_array_equal(a, b)
    assert one[1].max() >= 2


def test_volume_refuses_more_than_2_31_voxels():
    from nicer_slam_amd.tsdf import TSDFVolume
    with pytest.raises(ValueError, match=r"exceed 2\^31.*voxel_length of") as e:
        TSDFVolume((-8, -8, -8), (8, 8, 8), voxel_length=4.0 / 512)               # 2048^3, refused before anything is allocated
    fit = float(str(e.value).split("voxel_length of")[1].split()[0])
    assert 16.0 / fit <= 1290.2 and fit < 1.01 * 16.0 / 1290.15                   # cbrt(2^31) = 1290.16 voxels per axis
    for bad in (dict(voxel_length=0.0), dict(sdf_trunc=float("nan")), dict(voxel_length=float("inf"))):
        with pytest.raises(ValueError):
            TSDFVolume((-1, -1, -1), (1, 1, 1), **bad)
    with pytest.raises(ValueError):
        TSDFVolume((0, 0, 0), (1, 0, 1))


def test_bounds_from_frames_against_a_hand_computed_box():
    from nicer_slam_amd.tsdf import bounds_from_frames
    H, W = 4, 6
    depth = torch.zeros(2, H, W)
    depth[0, 1, 2] = 2.0                       # camera point ((2 - 2.5) / 10 * 2, (1 - 1.5) / 5 * 2, 2) = (-0.1, -0.2, 2)
    depth[0, 3, 5] = 4.0                       # ((5 - 2.5) / 10 * 4, (3 - 1.5) / 5 * 4, 4) = (1, 1.2, 4)
    depth[0, 0, 0] = float("nan")              # no measurement
    depth[0, 2, 2] = -1.0                      # no measurement
    depth[1, 0, 0] = 1.0                       # ((0 - 2.5) / 10, (0 - 1.5) / 5, 1) = (-0.25, -0.3, 1)
    depth[1, 3, 0] = 9.0                       # beyond depth_trunc below
    c2w = torch.eye(4).repeat(2, 1, 1)
    c2w[1, :3, :3] = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])     # camera z along world x, camera x along -world z
    c2w[1, :3, 3] = torch.tensor([10.0, 0.0, 0.0])                                             # -> world (10 + 1, -0.3, 0.25)
    lo, hi = bounds_from_frames(depth, c2w, (10.0, 5.0, 2.5, 1.5), margin=0.5, depth_trunc=8.0)
    np.testing.assert_allclose(lo.numpy(), np.array([-0.1, -0.3, 0.25]) - 0.5, rtol=0, atol=1e-12)
    np.testing.assert_allclose(hi.numpy(), np.array([11.0, 1.2, 4.0]) + 0.5, rtol=0, atol=1e-12)
    K = torch.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 10.0, 5.0, 2.5, 1.5
    lo2, hi2 = bounds_from_frames(depth.numpy(), c2w.numpy(), K, margin=0.5, depth_trunc=8.0)      # numpy frames, the 4 x 4 form
    assert torch.equal(lo, lo2) and torch.equal(hi, hi2)
    with pytest.raises(ValueError):
        bounds_from_frames(torch.zeros(1, H, W), c2w[:1], K)


def test_7scenes_reader(tmp_path):
    from nicer_slam_amd import tsdf
    raws, poses = tsdf_ref.write_7scenes_dir(str(tmp_path / "seq"))
    stems = tsdf.list_7scenes(str(tmp_path / "seq"))
    assert [os.path.basename(s) for s in stems] == ["frame-000000", "frame-000001", "frame-000002"]
    assert tsdf.list_7scenes(str(tmp_path / "seq"), 2) == stems[:2]
    depth, rgb, c2w = tsdf.read_7scenes(stems)
    assert depth.dtype == np.float32 and depth.shape == (3, 48, 64) and rgb.shape == (3, 48, 64, 3) and c2w.dtype == np.float64
    hole = (raws == 0) | (raws == 65535)
    assert hole.sum() == 3 * (4 * 5 + 3 * 10) and (depth[hole] == 0).all()                        # 0 and 65535: no measurement
    np.testing.assert_array_equal(depth[~hole], raws[~hole].astype(np.float32) / np.float32(1000.0))   # millimetres -> metres
    assert 0.2 < depth[~hole].min() and depth.max() < 1.2
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0 and rgb.std() > 0.05
    np.testing.assert_allclose(c2w, poses, rtol=1e-9, atol=1e-12)
    w2c32, w2c64 = tsdf.world_to_camera(torch.from_numpy(c2w))                                    # inverted in float64, rounded once
    np.testing.assert_array_equal(w2c32, np.linalg.inv(c2w)[:, :3, :].astype(np.float32))
    np.testing.assert_allclose(w2c64 @ c2w, np.tile(np.eye(4), (3, 1, 1)), rtol=0, atol=1e-14)
    with pytest.raises(FileNotFoundError):
        tsdf.list_7scenes(str(tmp_path / "nothing"))
