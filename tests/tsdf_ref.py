"""Oracle of depth fusion (include/nicer_slam_amd.h Section 10): the per-voxel rule restated in numpy float32 with the stated
operation order -- elementwise products and sums only, every one rounded on its own, IEEE division -- frame by frame, over an
explicit LIST of voxel indices, so that a volume of any size can be spot-checked; and the colour lookup in float64.
Also the fixtures the TSDF tests share: the analytic box room seen from a ring of cameras, and the distance to that box."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def voxel_indices(flat, dims):
    flat = np.asarray(flat, dtype=np.int64)
    return flat // (dims[1] * dims[2]), (flat // dims[2]) % dims[1], flat % dims[2]


def voxel_centres(flat, dims, origin, voxel_length):
    """c_a = origin_a + voxel_length * ((float)i_a + 0.5f), fp32 -> three [m] arrays"""
    vl = F(voxel_length)
    return tuple(F(origin[a]) + vl * (i.astype(F) + F(0.5)) for a, i in enumerate(voxel_indices(flat, dims)))


def integrate(flat, dims, origin, voxel_length, sdf_trunc, depth, rgb, w2c, K, depth_trunc=np.inf, state=None):
    """Frames k = 0 .. n-1 applied in order to the voxels ``flat`` (flat indices (x * ny + y) * nz + z).
    depth [n, H, W] f32, rgb [n, H * W, 3] f32 or None, w2c [n, 3, 4] f32, K [n or 1, 4] f32 (fx, fy, cx, cy).
    state: (tsdf, weight, colour [m, 3] or None) to continue from (default zeros).  Returns (tsdf [m], weight [m], colour [m, 3] or None)."""
    depth = np.asarray(depth, dtype=F)
    w2c = np.asarray(w2c, dtype=F)
    K = np.asarray(K, dtype=F).reshape(-1, 4)
    n, H, W = depth.shape
    m = len(flat)
    cx, cy, cz = voxel_centres(flat, dims, origin, voxel_length)
    if state is None:
        ts, wt = np.zeros(m, F), np.zeros(m, F)
        col = np.zeros((m, 3), F) if rgb is not None else None
    else:
        ts, wt = state[0].astype(F).copy(), state[1].astype(F).copy()
        col = state[2].astype(F).copy() if rgb is not None else None
    trunc = F(sdf_trunc)
    inv = F(1.0) / trunc
    dt = F(depth_trunc)
    with np.errstate(all="ignore"):
        for k in range(n):
            M = w2c[k]
            fx, fy, pcx, pcy = K[k if K.shape[0] > 1 else 0]
            p = [((M[r, 0] * cx + M[r, 1] * cy) + M[r, 2] * cz) + M[r, 3] for r in range(3)]
            ok = p[2] > 0
            uf = ((p[0] * fx) / p[2] + pcx) + F(0.5)
            vf = ((p[1] * fy) / p[2] + pcy) + F(0.5)
            ok &= (uf >= 0) & (uf < F(W)) & (vf >= 0) & (vf < F(H))
            u = np.where(ok, uf, 0).astype(np.int64)
            v = np.where(ok, vf, 0).astype(np.int64)
            d = depth[k, v, u]
            ok &= (d > 0) & (d <= dt)
            sdf = d - p[2]
            ok &= sdf > -trunc
            x = sdf * inv
            t = np.where(x < 1, x, F(1.0)).astype(F)
            den = wt + F(1.0)
            ts = np.where(ok, (ts * wt + t) / den, ts).astype(F)
            if col is not None:
                px = np.asarray(rgb[k], dtype=F)[v * W + u]
                col = np.where(ok[:, None], (col * wt[:, None] + px) / den[:, None], col).astype(F)
            wt = np.where(ok, den, wt).astype(F)
    assert ts.dtype == F and wt.dtype == F
    return ts, wt, col


def integrate_volume(dims, *args, **kw):
    """the whole volume: (tsdf, weight [nx, ny, nz], colour [3, nx, ny, nz] or None) -- the device layout"""
    ts, wt, col = integrate(np.arange(dims[0] * dims[1] * dims[2]), dims, *args, **kw)
    return ts.reshape(dims), wt.reshape(dims), (None if col is None else np.ascontiguousarray(col.T).reshape((3,) + tuple(dims)))


def sample_colour64(points, weight, colour, origin, voxel_length):
    """Section 10's lookup in float64 at fp32 ``points`` [m, 3]: trilinear over the eight surrounding voxel centres, each corner's
    weight multiplied by [weight > 0], normalised by the surviving sum.  weight [nx, ny, nz], colour [3, nx, ny, nz].
    Returns (colour [m, 3] float64, surviving weight sum [m] float64)."""
    dims = weight.shape
    g = (np.asarray(points, dtype=np.float64) - np.asarray([F(o) for o in origin], dtype=np.float64)) / float(F(voxel_length)) - 0.5
    b = np.floor(g)
    f = g - b
    b = b.astype(np.int64)
    s = np.zeros(len(g))
    acc = np.zeros((len(g), 3))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                i = b + np.array([dx, dy, dz])
                inside = ((i >= 0) & (i < np.array(dims))).all(1)
                ic = np.clip(i, 0, np.array(dims) - 1)
                live = inside & (weight[ic[:, 0], ic[:, 1], ic[:, 2]] > 0)
                w = np.where(dx, f[:, 0], 1 - f[:, 0]) * np.where(dy, f[:, 1], 1 - f[:, 1]) * np.where(dz, f[:, 2], 1 - f[:, 2])
                w = np.where(live, w, 0.0)
                s += w
                acc += w[:, None] * colour[:, ic[:, 0], ic[:, 1], ic[:, 2]].T.astype(np.float64)
    out = np.where(s[:, None] > 0, acc / np.where(s > 0, s, 1.0)[:, None], 0.0)
    return out, s


# ------------------------------------------------------------------------------------------------------------------- fixtures
ROOM_HALF = (0.62, 0.5, 0.56)


def ring_poses(n, radius=0.22, pitch=0.6):
    """n camera-to-world matrices (float32 [n, 4, 4]) on a ring of ``radius`` in the plane y = 0 inside the room, looking outwards and
    alternately up and down by ``pitch`` radians, so that walls, floor and ceiling are all seen.  Camera axes: x right, y down, z forward."""
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        a = 2 * np.pi * k / n
        el = pitch * (-1.0 if k % 2 else 1.0) * (0.5 + 0.5 * ((k // 2) % 2))
        fwd = np.array([np.cos(a) * np.cos(el), np.sin(el), np.sin(a) * np.cos(el)])
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        out[k, :3, 0], out[k, :3, 1], out[k, :3, 2] = right, down, fwd
        out[k, :3, 3] = [radius * np.cos(a), 0.05 * np.sin(3 * a), radius * np.sin(a)]
    return out.astype(F)


def pinhole(H, W, focal):
    """the project's 4 x 4 intrinsics with the principal point at the image centre (pixel centres at integer coordinates)"""
    K = np.eye(4, dtype=F)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return K


def room_frames(poses, H, W, focal, device="cpu", half=ROOM_HALF):
    """(depth [n, H, W], rgb [n, H * W, 3]) float32 torch tensors on ``device``: tools/synthetic_sequence.render_analytic_room, whose
    depth is z-depth along the camera axis."""
    import torch
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import synthetic_sequence as ss
    rgb, depth, _ = ss.render_analytic_room(torch.from_numpy(np.asarray(poses)), torch.from_numpy(pinhole(H, W, focal)), H, W, device, half)
    return depth.reshape(len(poses), H, W).float().contiguous(), rgb.float().contiguous()


def shared_K4(H, W, focal):
    K = pinhole(H, W, focal)
    return np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]]], dtype=F)


def fuse_room(poses, n_vox=96, vl=0.015, H=120, W=160, focal=100.0):
    """The analytic room fused by the oracle into n_vox^3 voxels of ``vl`` centred on the room, truncation 4 voxels:
    (tsdf, weight, colour, origin, vl, depth, rgb) -- the volume in the device layout, the frames as torch host tensors."""
    depth, rgb = room_frames(poses, H, W, focal)
    w2c = np.linalg.inv(np.asarray(poses, dtype=np.float64))[:, :3, :].astype(F)
    origin = (-0.5 * n_vox * vl,) * 3
    ts, wt, col = integrate_volume((n_vox,) * 3, origin, vl, 4 * vl, depth.numpy(), rgb.numpy(), w2c, shared_K4(H, W, focal))
    return ts, wt, col, origin, vl, depth, rgb


def box_distance(points, half=ROOM_HALF):
    """closed-form distance of points [m, 3] to the SURFACE of the axis-aligned box [-half, half] (float64)"""
    q = np.abs(np.asarray(points, dtype=np.float64)) - np.asarray(half, dtype=np.float64)
    outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
    inside = -np.minimum(q.max(1), 0.0)
    return np.where((q > 0).any(1), outside, inside)


def box_mesh(half=ROOM_HALF):
    """the room as 12 triangles: dict(verts [8, 3] float32, faces [12, 3] int32)"""
    h = np.asarray(half, dtype=F)
    verts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=F) * h
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    return dict(verts=verts, faces=faces)


def write_7scenes_dir(path, n=3, H=48, W=64, seed=0):
    """A small stand-in of a 7-Scenes sequence directory, written with PIL: the top-left H x W window of 480 x 640 frames of the analytic
    room seen with the data set's camera (a window from the corner keeps 585 / 585 / 320 / 240 true for it), as uint16 millimetre depth
    PNGs with holes (0 and 65535), colour PNGs and 4 x 4 camera-to-world text files.  Returns (raw uint16 depth, poses)."""
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    poses = ring_poses(n).astype(np.float64)
    depth, rgb = room_frames(poses.astype(np.float32), 480, 640, 585.0)
    raws = []
    for k in range(n):
        raw = np.rint(depth[k].numpy()[:H, :W] * 1000.0).astype(np.uint16)
        raw[5:9, 7:12] = 0
        raw[20:23, 30:40] = 65535
        raws.append(raw)
        Image.fromarray(raw).save(os.path.join(path, f"frame-{k:06d}.depth.png"))
        col = np.rint(rgb[k].numpy().reshape(480, 640, 3)[:H, :W] * 255.0).astype(np.uint8)
        Image.fromarray(col, "RGB").save(os.path.join(path, f"frame-{k:06d}.color.png"))
        np.savetxt(os.path.join(path, f"frame-{k:06d}.pose.txt"), poses[k], fmt="%.9e", delimiter="\t")
    return np.stack(raws), poses
