"""Depth fusion: depth frames -> dense TSDF volume -> coloured mesh, on the device (include/nicer_slam_amd.h Section 10).

What the reference does offline with open3d in preprocess/get_mesh_7scenes.py (ScalableTSDFVolume, voxel 4/512 m, truncation 0.04 m,
RGB8): here a dense box of voxels, one HIP kernel that integrates a batch of frames per pass over the voxel state, the project's
marching cubes on the observed part of the volume and a colour lookup at the vertices.  The box is the caller's to size
(``bounds_from_frames``); an unbounded hashed volume is a deliberate departure.

    python -m nicer_slam_amd.tsdf SEQ_DIR --out MESH.ply [--frames N --voxel V --trunc T]

fuses one 7-Scenes sequence directory (frame-%06d.pose.txt / .color.png / .depth.png) into a PLY.
"""
import argparse
import ctypes
import glob
import math
import os

import numpy as np
import torch

from ._native import TsdfVolumeDesc, check, lib
from .ply import write_ply

MAX_VOXELS = 1 << 31                      # marching cubes' limit (Section 7)
SCENES7_CAMERA = (585.0, 585.0, 320.0, 240.0)


def _as_numpy(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def _intrinsics4(intrinsics, n):
    """-> float64 [n or 1, 4] rows (fx, fy, cx, cy) from the project's 4 x 4 (or 3 x 3) matrix, a stack of them, (fx, fy, cx, cy) or a
    stack of those."""
    K = _as_numpy(intrinsics, np.float64)
    if K.ndim >= 2 and K.shape[-1] == K.shape[-2] and K.shape[-1] in (3, 4):
        K = np.stack([K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]], -1)
    if K.shape[-1] != 4 or K.ndim > 2:
        raise ValueError("intrinsics: a 4 x 4 matrix, (fx, fy, cx, cy), or a stack of n of either")
    K = K.reshape(-1, 4)
    if K.shape[0] not in (1, n):
        raise ValueError(f"intrinsics: {K.shape[0]} cameras for {n} frames")
    return K


def world_to_camera(c2w):
    """c2w [n, 4, 4] (any float type, torch or numpy) -> (w2c float32 [n, 3, 4], w2c float64 [n, 4, 4]): inverted in float64 on the
    host and rounded once, so that every consumer of the fp32 rows sees the same matrices."""
    P = _as_numpy(c2w, np.float64)
    if P.ndim == 2:
        P = P[None]
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError("c2w: [4, 4] or [n, 4, 4] camera-to-world matrices")
    inv = np.linalg.inv(P)
    return np.ascontiguousarray(inv[:, :3, :].astype(np.float32)), inv


def _stack_frames(depth, rgb):
    """depth [H, W] or [n, H, W]; rgb None, [H, W, 3], [n, H, W, 3] or [n, H * W, 3] -> (depth [n, H, W], rgb [n, H * W, 3] or None),
    float32, torch, on whatever device they came from."""
    depth = torch.as_tensor(depth)
    if depth.dim() == 2:
        depth = depth[None]
    if depth.dim() != 3:
        raise ValueError("depth: [H, W] or [n, H, W]")
    n, H, W = depth.shape
    if rgb is not None:
        rgb = torch.as_tensor(rgb)
        if rgb.numel() != n * H * W * 3 or rgb.shape[-1] != 3:
            raise ValueError(f"rgb: {tuple(rgb.shape)} does not match {n} frames of {H} x {W} x 3")
        rgb = rgb.reshape(n, H * W, 3).float()
    return depth.float(), rgb


def bounds_from_frames(depth, c2w, intrinsics, margin=0.04 + 4.0 / 512, depth_trunc=float("inf")):
    """Axis-aligned bounding box (lo [3], hi [3], float64 tensors on the host) of the back-projected valid depth points
    (0 < d <= depth_trunc, finite) of the frames, grown by ``margin`` on every side (default: the default truncation plus one default
    voxel) -- how a caller sizes the dense box of ``TSDFVolume``.  Pixel centres sit at integer (u, v): a pixel with depth d is the
    camera-frame point ((u - cx) / fx * d, (v - cy) / fy * d, d).  Raises ValueError when no frame has a valid depth."""
    depth, _ = _stack_frames(depth, None)
    n, H, W = depth.shape
    dev = depth.device
    P = torch.as_tensor(_as_numpy(c2w, np.float64)).reshape(-1, 4, 4).to(dev)
    K = torch.as_tensor(_intrinsics4(intrinsics, n)).to(dev)
    if P.shape[0] != n:
        raise ValueError(f"c2w: {P.shape[0]} poses for {n} frames")
    u = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    v = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    lo = torch.full((3,), float("inf"), dtype=torch.float64, device=dev)
    hi = -lo
    for k in range(n):
        fx, fy, cx, cy = K[k if K.shape[0] > 1 else 0]
        d = depth[k].double()
        ok = (d > 0) & (d <= depth_trunc) & torch.isfinite(d)
        if not bool(ok.any()):
            continue
        cam = torch.stack([((u - cx) / fx * d)[ok], ((v - cy) / fy * d)[ok], d[ok]], -1)
        world = cam @ P[k, :3, :3].t() + P[k, :3, 3]
        lo = torch.minimum(lo, world.min(0).values)
        hi = torch.maximum(hi, world.max(0).values)
    if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        raise ValueError("bounds_from_frames: no valid depth in any frame")
    return (lo - margin).cpu(), (hi + margin).cpu()


class TSDFVolume:
    """A dense TSDF volume over the box [lo, hi]: ceil((hi - lo) / voxel_length) voxels per axis, voxel (x, y, z) centred at
    lo + voxel_length * (index + 0.5); ``tsdf`` and ``weight`` [nx, ny, nz] fp32 and, with ``color``, ``colour`` [3, nx, ny, nz]
    (planar, Section 10).  Raises ValueError above 2^31 voxels, before anything is allocated."""

    def __init__(self, lo, hi, voxel_length=4.0 / 512, sdf_trunc=0.04, color=True, device="cuda"):
        lo = [float(x) for x in _as_numpy(lo, np.float64).reshape(3)]
        hi = [float(x) for x in _as_numpy(hi, np.float64).reshape(3)]
        if not (all(math.isfinite(x) for x in lo + hi) and all(h > l for l, h in zip(lo, hi))):
            raise ValueError("TSDFVolume: lo and hi must be finite with hi > lo on every axis")
        if not (math.isfinite(voxel_length) and voxel_length > 0 and math.isfinite(sdf_trunc) and sdf_trunc > 0):
            raise ValueError("TSDFVolume: voxel_length and sdf_trunc must be finite and positive")
        ext = [h - l for l, h in zip(lo, hi)]
        dims = [max(1, int(math.ceil(e / voxel_length - 1e-9))) for e in ext]
        if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            fit = (ext[0] * ext[1] * ext[2] / MAX_VOXELS) ** (1.0 / 3.0)
            while math.prod(max(1, int(math.ceil(e / fit - 1e-9))) for e in ext) > MAX_VOXELS:
                fit *= 1.001
            raise ValueError(f"TSDFVolume: {dims[0]} x {dims[1]} x {dims[2]} voxels exceed 2^31; a voxel_length of {fit:.6g} "
                             "or more fits this box")
        self.dims = tuple(dims)
        self.origin = tuple(float(np.float32(x)) for x in lo)          # as the kernel sees it
        self.voxel_length = float(np.float32(voxel_length))
        self.sdf_trunc = float(np.float32(sdf_trunc))
        self.device = torch.device(device)
        self.tsdf = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.colour = torch.zeros((3,) + self.dims, dtype=torch.float32, device=self.device) if color else None

    def reset(self):
        self.tsdf.zero_()
        self.weight.zero_()
        if self.colour is not None:
            self.colour.zero_()

    def _desc(self):
        nx, ny, nz = self.dims
        return TsdfVolumeDesc(self.tsdf.data_ptr(), self.weight.data_ptr(), self.colour.data_ptr() if self.colour is not None else None,
                              nx, ny, nz, (ctypes.c_float * 3)(*self.origin), self.voxel_length, self.sdf_trunc)

    @property
    def centre0(self):
        """centre of voxel (0, 0, 0) in fp32 arithmetic, as Section 10 forms it"""
        vl, h = np.float32(self.voxel_length), np.float32(0.5)
        return tuple(float(np.float32(o) + vl * h) for o in self.origin)

    @torch.no_grad()
    def integrate(self, depth, rgb, c2w, intrinsics, depth_trunc=float("inf"), batch=32):
        """Fuse one frame or a stack, in order.  depth [H, W] / [n, H, W] (z-depth in the volume's units; 0, negative, NaN = no
        measurement), rgb [.., H, W, 3] or [n, H * W, 3] in [0, 1] (required by a volume with colour), c2w [4, 4] / [n, 4, 4]
        camera-to-world, intrinsics 4 x 4 or (fx, fy, cx, cy), one or one per frame; torch (host or device) or numpy.  The poses
        are inverted in float64 on the host and rounded to fp32.  ``batch`` frames go through the kernel per pass over the
        volume; any batch size gives the same bits."""
        depth, rgb = _stack_frames(depth, rgb)
        n, H, W = depth.shape
        if self.colour is not None and rgb is None:
            raise ValueError("integrate: this volume has colour; pass rgb (or build it with color=False)")
        w2c, _ = world_to_camera(c2w)
        if w2c.shape[0] != n:
            raise ValueError(f"c2w: {w2c.shape[0]} poses for {n} frames")
        K = _intrinsics4(intrinsics, n).astype(np.float32)
        if not (depth_trunc > 0):
            raise ValueError("depth_trunc must be positive")
        dev = self.device
        w2c_d = torch.from_numpy(w2c).to(dev)
        K_d = torch.from_numpy(np.ascontiguousarray(K)).to(dev)
        per_frame = K.shape[0] > 1
        desc = self._desc()
        st = torch.cuda.current_stream(dev).cuda_stream
        batch = max(1, int(batch))
        zmax = torch.empty(33 * min(batch, n), dtype=torch.float32, device=dev)      # the kernel's workspace (Section 10)
        for lo in range(0, n, batch):
            m = min(batch, n - lo)
            d = depth[lo:lo + m].to(dev).contiguous()
            c = rgb[lo:lo + m].to(dev).contiguous() if self.colour is not None else None
            check(lib.nsa_tsdf_integrate(ctypes.byref(desc), d.data_ptr(), c.data_ptr() if c is not None else None,
                                         w2c_d[lo:].data_ptr(), K_d[lo:].data_ptr() if per_frame else K_d.data_ptr(), int(per_frame),
                                         m, H, W, float(depth_trunc), zmax.data_ptr(), st))
        return self

    def surface_volume(self, min_weight=1):
        """tsdf where weight >= min_weight, NaN elsewhere: what marching cubes meshes (it skips cells with a non-finite corner)."""
        return torch.where(self.weight >= min_weight, self.tsdf, torch.full_like(self.tsdf, float("nan")))

    @torch.no_grad()
    def sample_colour(self, points):
        """Colour [m, 3] of the volume at device points [m, 3] (Section 10: trilinear over the observed voxel centres)."""
        if self.colour is None:
            raise ValueError("sample_colour: this volume has no colour")
        pts = points.to(self.device).float().contiguous()
        out = torch.empty_like(pts)
        desc = self._desc()
        check(lib.nsa_tsdf_sample_colour(ctypes.byref(desc), pts.data_ptr() if pts.numel() else None, pts.shape[0],
                                         out.data_ptr() if pts.numel() else None, torch.cuda.current_stream(self.device).cuda_stream))
        return out

    @torch.no_grad()
    def extract_mesh(self, min_weight=1, smooth=None, decimate=None, fill_holes=None, split=None):
        """The zero level of the observed volume: the ``inference.marching_cubes`` dict (verts, normals, faces), plus ``colors`` when
        the volume has colour -- what ``inference.write_ply`` and ``mesh_eval.mesh_metrics`` take.  ``smooth``: a dict of
        ``mesh_smooth.smooth`` keywords, applied after the colours are sampled on the true level set (the depth noise of the
        frames is on that surface); None leaves the mesh as marching cubes made it.  ``decimate``: a dict of
        ``mesh_decimate.decimate`` keywords, applied last; None collapses nothing.  ``fill_holes``: a dict of
        ``mesh_fill.fill_holes`` keywords, applied after the colours and before ``smooth`` and ``decimate``; None fills nothing.
        ``split``: True or a dict of ``mesh_repair.split_nonmanifold`` keywords, applied before ``decimate``: the mesh is cut into a
        2-manifold there (thin structures give marching cubes edges with four faces); None cuts nothing."""
        if split is not None and not isinstance(split, (bool, dict)):
            raise ValueError("extract_mesh: split must be None, a bool or a dict of mesh_repair.split_nonmanifold keywords")
        if fill_holes is not None and not isinstance(fill_holes, dict):
            raise ValueError("extract_mesh: fill_holes must be None or a dict of mesh_fill.fill_holes keywords")
        if decimate is not None and not isinstance(decimate, dict):
            raise ValueError("extract_mesh: decimate must be None or a dict of mesh_decimate.decimate keywords")
        if smooth is not None and not isinstance(smooth, dict):
            raise ValueError("extract_mesh: smooth must be None or a dict of mesh_smooth.smooth keywords")
        from .inference import marching_cubes
        mesh = marching_cubes(self.surface_volume(min_weight), 0.0, (self.voxel_length,) * 3, self.centre0)
        if self.colour is not None:
            mesh["colors"] = self.sample_colour(mesh["verts"])
        if fill_holes is not None:
            from .mesh_fill import fill_holes as fill_mesh
            mesh = fill_mesh(mesh, **fill_holes)
        if smooth is not None:
            from .mesh_smooth import smooth as smooth_mesh
            mesh = smooth_mesh(mesh, **smooth)
        if split:
            from .mesh_repair import split_nonmanifold
            mesh = split_nonmanifold(mesh, **(split if isinstance(split, dict) else {}))
        if decimate is not None:
            from .mesh_decimate import decimate as decimate_mesh
            mesh = decimate_mesh(mesh, **decimate)
        return mesh


# ------------------------------------------------------------------------------------------------------------------- 7-Scenes
def list_7scenes(seq_dir, frames=None):
    """Frame stems (path without the .pose.txt / .color.png / .depth.png suffix) of a 7-Scenes sequence directory in frame order;
    ``frames``: None = all, N = the first N."""
    stems = sorted(p[:-len(".pose.txt")] for p in glob.glob(os.path.join(seq_dir, "frame-*.pose.txt")))
    if not stems:
        raise FileNotFoundError(f"{seq_dir}: no frame-*.pose.txt")
    return stems if frames is None else stems[:int(frames)]


def read_7scenes(stems, color=True):
    """-> (depth [n, H, W] float32 metres with 0 = no measurement, rgb [n, H, W, 3] float32 in [0, 1] or None, c2w [n, 4, 4] float64).
    The depth PNGs hold uint16 millimetres; 0 and 65535 mean no measurement."""
    from PIL import Image
    depth, rgb, pose = [], [], []
    for s in stems:
        raw = np.array(Image.open(s + ".depth.png")).astype(np.int64)
        if raw.ndim != 2:
            raise ValueError(f"{s}.depth.png: not a single-channel image")
        d = raw.astype(np.float32) / np.float32(1000.0)
        d[(raw <= 0) | (raw >= 65535)] = 0.0
        depth.append(d)
        if color:
            rgb.append(np.asarray(Image.open(s + ".color.png").convert("RGB"), dtype=np.float32) / np.float32(255.0))
        pose.append(np.loadtxt(s + ".pose.txt", dtype=np.float64).reshape(4, 4))
    return np.stack(depth), (np.stack(rgb) if color else None), np.stack(pose)


def fuse_7scenes(seq_dir, frames=None, voxel_length=4.0 / 512, sdf_trunc=0.04, depth_trunc=float("inf"), color=True, batch=32,
                 min_weight=1, device="cuda"):
    """What preprocess/get_mesh_7scenes.py does for one sequence directory: every frame (camera 585 / 585 / 320 / 240) fused into a
    TSDF volume, and the coloured mesh of its zero level.  The box is the bounding box of the frames' depth points plus truncation
    and one voxel (a first pass over the depth files).  Frames whose pose is not finite (the data set marks lost tracking that way)
    are left out.  Returns the mesh dict of ``TSDFVolume.extract_mesh``."""
    stems = list_7scenes(seq_dir, frames)
    chunks = [stems[i:i + batch] for i in range(0, len(stems), batch)]
    lo = np.full(3, np.inf)
    hi = -lo
    for ch in chunks:
        d, _, pose = read_7scenes(ch, color=False)
        ok = np.isfinite(pose).all((1, 2))
        if not ok.any() or not (d[ok] > 0).any():
            continue
        a, b = bounds_from_frames(d[ok], pose[ok], SCENES7_CAMERA, sdf_trunc + voxel_length, depth_trunc)
        lo, hi = np.minimum(lo, a.numpy()), np.maximum(hi, b.numpy())
    if not np.isfinite(lo).all():
        raise ValueError(f"{seq_dir}: no frame with a finite pose and a valid depth")
    vol = TSDFVolume(lo, hi, voxel_length, sdf_trunc, color, device)
    for ch in chunks:
        d, c, pose = read_7scenes(ch, color=color)
        ok = np.isfinite(pose).all((1, 2))
        if ok.any():
            vol.integrate(d[ok], c[ok] if color else None, pose[ok], SCENES7_CAMERA, depth_trunc, batch)
    return vol.extract_mesh(min_weight)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.tsdf",
                                 description="Fuse the depth frames of one 7-Scenes sequence directory into a coloured mesh.")
    ap.add_argument("seq_dir")
    ap.add_argument("--out", required=True, help="PLY to write")
    ap.add_argument("--frames", type=int, default=None, help="use the first N frames (default: all)")
    ap.add_argument("--voxel", type=float, default=4.0 / 512)
    ap.add_argument("--trunc", type=float, default=0.04)
    args = ap.parse_args(argv)
    mesh = fuse_7scenes(args.seq_dir, args.frames, args.voxel, args.trunc)
    write_ply(args.out, mesh)
    print(f"{args.out}: {mesh['verts'].shape[0]} vertices, {mesh['faces'].shape[0]} faces")


if __name__ == "__main__":
    main()
