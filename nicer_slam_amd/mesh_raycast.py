"""Rays against a triangle mesh on the device (include/nicer_slam_amd.h Section 17, csrc/mesh_raycast.hip): the exact
first hit of each ray, in float64, by a watertight test -- no ray slips between two faces that share an edge.

* ``cast_rays``: (t, face, barycentrics) of arbitrary rays against a mesh dict or a ``mesh_eval.TriIndex``.
* ``camera_rays``: the rays of a pinhole camera, for a whole image or for sampled pixels, with camera-space z = 1: t is a z-depth.
* ``render_depth``: depth, face id and normal images with the shapes and hole conventions of ``mesh_render.render_mesh`` -- and
  WITHOUT its near-plane departure: a face that straddles the camera is cut at ``near`` ray by ray, not dropped whole.  The camera
  may stand inside a room of a few large faces.
* ``depth_at``: the same three at sampled pixels only -- the shape of the training loops' ray batches.
* ``occluded``: whether something lies between pairs of points; ``mesh_render.visible_faces(method="raycast")`` is built on it.
* ``python -m nicer_slam_amd.mesh_raycast MESH.ply --poses P --intrinsics fx fy cx cy --size H W --out DIR [--near N] [--sim3 T.npy]``
  writes ``%06d.npy`` (float32 depth, 0 = hole) and ``%06d.depth.png`` (uint16 millimetres, 0 = hole) per pose.

numpy in, numpy out; torch in, torch out.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import functools
import math
import os
import sys

import numpy as np
import torch

from .mesh_args import mesh_dict_tensors, need_gpu
from .mesh_eval import TriIndex
from .ply import read_ply
from .tsdf import _as_numpy, _intrinsics4

CHANNELS = ("depth", "face_id", "normal")
DEFAULT_NEAR = 0.01
TILE = 8                         # camera rays reach the kernel in TILE x TILE pixel blocks: a wave is one block


def _index(mesh_or_index, device="cuda"):
    """(TriIndex, was_numpy, original device) of a mesh dict or an index"""
    if isinstance(mesh_or_index, TriIndex):
        return mesh_or_index, False, mesh_or_index.device
    need_gpu("mesh_raycast")
    m, was_numpy, orig = mesh_dict_tensors(mesh_or_index, device)
    return TriIndex(m["verts"], m["faces"]), was_numpy, orig


def _rays(x, name, dev):
    # (not mesh_args.checked_points: rays may be arrays or live on another device, and are moved to the index's)
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: needs shape [m, 3], got {tuple(t.shape)}")
    return t.to(dev).float().contiguous()


def _check_call(origins, dirs, tmin, tmax, cull):
    if np.shape(origins) != np.shape(dirs) or len(np.shape(origins)) != 2 or np.shape(origins)[1] != 3:
        raise ValueError(f"rays: origins {tuple(np.shape(origins))} and dirs {tuple(np.shape(dirs))} must both be [m, 3]")
    if math.isnan(float(tmin)) or math.isnan(float(tmax)):
        raise ValueError("tmin and tmax must not be NaN")
    if cull not in (None, "back", "front"):
        raise ValueError(f"cull must be None, 'back' or 'front', got {cull!r}")


@torch.no_grad()
def cast_rays(mesh_or_index, origins, dirs, tmin=0.0, tmax=math.inf, any_hit=False, cull=None, counts=False, brute=False,
              device="cuda"):
    """``TriIndex.raycast`` for a mesh dict (``verts`` [V, 3], ``faces`` [F, 3]; numpy or torch) or an index, and rays as arrays or
    tensors [m, 3]: (t float64, face int64, bary [m, 3] float64), or bool [m] with ``any_hit``; ``counts=True`` appends the nodes
    visited and the faces tested per ray.  numpy comes back for numpy rays, torch on the rays' own device otherwise."""
    _check_call(origins, dirs, tmin, tmax, cull)
    ix, _, _ = _index(mesh_or_index, device)
    as_numpy = not torch.is_tensor(origins)
    out = ix.raycast(_rays(origins, "origins", ix.device), _rays(dirs, "dirs", ix.device), tmin, tmax, any_hit, cull, counts, brute)
    single = not isinstance(out, tuple)
    out = (out,) if single else out
    out = tuple(x.cpu().numpy() for x in out) if as_numpy else tuple(x.to(origins.device) for x in out)
    return out[0] if single else out


def _camera(c2w, intrinsics, size):
    P = _as_numpy(c2w, np.float64)
    if P.shape != (4, 4):
        raise ValueError("c2w: one [4, 4] camera-to-world matrix")
    K = _intrinsics4(intrinsics, 1)[0]
    H, W = int(size[0]), int(size[1])
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError("size: (H, W) with 1 <= H, W <= 16384")
    if not (np.isfinite(P).all() and np.isfinite(K).all() and K[0] != 0 and K[1] != 0):
        raise ValueError("camera: pose and intrinsics must be finite, fx and fy non-zero")
    return P, K, H, W


def _camera_rays_torch(P, K, u, v, dev):
    """fp32 (origins, dirs) [k, 3] on ``dev`` for float64 pixel coordinates u, v [k] there: d = R ((u - cx) / fx, (v - cy) / fy, 1),
    formed in float64 -- (R_k0 x + R_k1 y) + R_k2 -- and rounded once"""
    x, y = (u - float(K[2])) / float(K[0]), (v - float(K[3])) / float(K[1])
    d = torch.stack([(float(P[k, 0]) * x + float(P[k, 1]) * y) + float(P[k, 2]) for k in range(3)], 1)
    o = torch.tensor(P[:3, 3].tolist(), dtype=torch.float64, device=dev).expand_as(d)
    return o.float().contiguous(), d.float().contiguous()


def camera_rays(c2w, intrinsics, size, pixels=None, device=None):
    """(origins, dirs) fp32 [H * W, 3] in row-major pixel order, or [k, 3] for ``pixels`` [k, 2] = (column, row), which need not be
    integers: pixel centres at integer (column, row), x right, y down, z forward -- the conventions of ``tsdf`` and ``mesh_render``.
    A direction has camera-space z = 1, so the t of a hit is its z-depth.  numpy unless ``device`` names a torch device."""
    P, K, H, W = _camera(c2w, intrinsics, size)
    dev = torch.device("cpu" if device is None else device)
    if pixels is None:
        r, c = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                              indexing="ij")
        u, v = c.reshape(-1), r.reshape(-1)
    else:
        px = pixels if torch.is_tensor(pixels) else torch.from_numpy(np.asarray(pixels))
        if px.dim() != 2 or px.shape[1] != 2:
            raise ValueError("pixels: [k, 2] (column, row)")
        px = px.to(dev).double()
        u, v = px[:, 0], px[:, 1]
    o, d = _camera_rays_torch(P, K, u, v, dev)
    return (o.numpy(), d.numpy()) if device is None else (o, d)


@functools.lru_cache(maxsize=8)
def _tile_order(H, W, dev):
    """the permutation of the row-major pixels that lists them TILE x TILE block by block"""
    r, c = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    key = ((r // TILE) * ((W + TILE - 1) // TILE) + c // TILE) * (TILE * TILE) + (r % TILE) * TILE + c % TILE
    return torch.argsort(key.reshape(-1))


def _face_normals(ix, face, dirs, flip_to_camera):
    """fp32 unit normals [m, 3] of the faces hit (0 where none), turned against the ray with ``flip_to_camera``"""
    hit = face >= 0
    f = ix.faces[face.clamp(min=0)].long()
    a, b, c = (ix.verts[f[:, k]].double() for k in range(3))
    n = torch.linalg.cross(b - a, c - a)
    n = n / n.norm(dim=1, keepdim=True).clamp(min=1e-300)
    if flip_to_camera:
        n = torch.where(((n * dirs.double()).sum(1) > 0)[:, None], -n, n)
    return torch.where(hit[:, None], n, torch.zeros_like(n)).float()


def _shade(ix, o, d, near, channels, flip_to_camera):
    t, face, _ = ix.raycast(o, d, tmin=near)
    out = {}
    if "depth" in channels:
        out["depth"] = torch.where(face >= 0, t, torch.zeros_like(t))
    if "face_id" in channels:
        out["face_id"] = face.to(torch.int32)
    if "normal" in channels:
        out["normal"] = _face_normals(ix, face, d, flip_to_camera)
    return out


def _channels(channels):
    bad = [c for c in channels if c not in CHANNELS]
    if bad:
        raise ValueError(f"channels: unknown {bad}; choose from {CHANNELS}")
    return tuple(channels)


def _near(near):
    if not (0 <= float(near) < 1e30):
        raise ValueError("near must be >= 0")
    return float(near)


@torch.no_grad()
def render_depth(mesh, c2w, intrinsics, size, near=DEFAULT_NEAR, channels=CHANNELS, flip_to_camera=True, device="cuda"):
    """Ray-cast images of ``mesh`` (a dict as for ``mesh_render.render_mesh``, or a TriIndex) from ``c2w`` ([4, 4] or [n, 4, 4]):
    a dict of [n, H, W (, 3)] images with ``render_mesh``'s conventions --
      ``depth``    float64 z-depth of the first hit at or beyond ``near`` along the pixel's ray, 0 where nothing is hit
      ``face_id``  int32, -1 where nothing is hit
      ``normal``   fp32 world-space unit normal of the face hit, turned towards the camera with ``flip_to_camera``
    ``near`` is the rays' tmin: a face that reaches behind the camera is cut there, ray by ray -- there is no clipping departure.
    Depth is the float64 t of header Section 17, exact for the fp32 ray of the pixel."""
    channels, near = _channels(channels), _near(near)
    ix, was_numpy, orig = _index(mesh, device)
    P = _as_numpy(c2w, np.float64)
    P = P[None] if P.ndim == 2 else P
    if P.ndim != 3 or P.shape[1:] != (4, 4) or P.shape[0] == 0:
        raise ValueError("c2w: [4, 4] or [n, 4, 4] camera-to-world matrices")
    Ks = _intrinsics4(intrinsics, P.shape[0])
    H, W = int(size[0]), int(size[1])
    _camera(P[0], Ks[0], size)
    order = _tile_order(H, W, ix.device)
    parts = []
    for i in range(P.shape[0]):
        o, d = camera_rays(P[i], Ks[i if Ks.shape[0] > 1 else 0], size, device=ix.device)
        r = _shade(ix, o[order], d[order], near, channels, flip_to_camera)
        img = {}
        for k, x in r.items():
            full = torch.empty_like(x)
            full[order] = x
            img[k] = full.reshape((H, W) + tuple(x.shape[1:]))
        parts.append(img)
    out = {k: torch.stack([p[k] for p in parts]) for k in channels}
    return {k: (x.cpu().numpy() if was_numpy else x.to(orig)) for k, x in out.items()}


@torch.no_grad()
def depth_at(mesh, c2w, intrinsics, pixels, near=DEFAULT_NEAR, flip_to_camera=True, device="cuda"):
    """(depth [k] float64, face [k] int64, normal [k, 3] fp32) at ``pixels`` [k, 2] = (column, row) of the camera ``c2w`` [4, 4]:
    ``render_depth``'s three channels for sampled pixels only, without touching the rest of the image."""
    near = _near(near)
    ix, was_numpy, orig = _index(mesh, device)
    was_numpy = was_numpy and not torch.is_tensor(pixels)
    o, d = camera_rays(c2w, intrinsics, (1, 1), pixels, device=ix.device)
    r = _shade(ix, o, d, near, CHANNELS, flip_to_camera)
    out = (r["depth"], r["face_id"].long(), r["normal"])
    return tuple(x.cpu().numpy() for x in out) if was_numpy else tuple(x.to(orig if orig is not None else ix.device) for x in out)


@torch.no_grad()
def occluded(mesh, origins, targets, rel=1e-3, device="cuda"):
    """bool [m]: whether the mesh is hit on the way from ``origins`` [m, 3] (or one point [3]) to ``targets`` [m, 3] -- an any-hit
    query over t in [0, 1 - rel] along target - origin, so that a target ON the surface is not hidden by its own face.  A pair with
    a non-finite coordinate, or with origin == target, is not occluded."""
    if not (0.0 <= float(rel) < 1.0):
        raise ValueError("rel must lie in [0, 1)")
    ix, _, _ = _index(mesh, device)
    as_numpy = not torch.is_tensor(targets)
    tg = _rays(targets, "targets", ix.device)
    og = origins if torch.is_tensor(origins) else torch.from_numpy(np.ascontiguousarray(np.asarray(origins)))
    og = og.to(ix.device).float()
    og = og.reshape(1, 3).expand_as(tg).contiguous() if og.numel() == 3 else _rays(og, "origins", ix.device)
    if og.shape != tg.shape:
        raise ValueError(f"occluded: {og.shape[0]} origins for {tg.shape[0]} targets")
    hit = ix.raycast(og, tg - og, 0.0, 1.0 - float(rel), any_hit=True)
    return hit.cpu().numpy() if as_numpy else hit.to(targets.device)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_raycast", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--poses", required=True, help="camera-to-world poses: .npy [n, 4, 4], text, or a directory of *.pose.txt")
    ap.add_argument("--intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"), required=True)
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), required=True)
    ap.add_argument("--out", required=True, help="directory for %%06d.npy (float32 depth) and %%06d.depth.png (uint16 millimetres)")
    ap.add_argument("--near", type=float, default=DEFAULT_NEAR)
    ap.add_argument("--sim3", metavar="T.npy", help="4x4 similarity applied to the mesh first")
    a = ap.parse_args(argv)
    if a.size[0] < 1 or a.size[1] < 1:
        ap.error("image sizes must be positive")
    if not a.near >= 0:
        ap.error("--near must be >= 0")
    return a


def main(argv=None):
    from PIL import Image
    from .mesh_clean import transform_mesh            # (a cycle: mesh_clean -> mesh_topology -> this module)
    from .mesh_render import read_poses               # (a cycle: mesh_render is built on this module)
    a = parse_args(argv)
    try:
        mesh = read_ply(a.mesh)
        if a.sim3:
            mesh = transform_mesh(mesh, np.load(a.sim3))
        poses = read_poses(a.poses)
        ix, _, _ = _index(mesh)
        os.makedirs(a.out, exist_ok=True)
        for i, P in enumerate(poses):
            d = render_depth(ix, P, a.intrinsics, a.size, a.near, ("depth",))["depth"][0].float().cpu().numpy()
            np.save(os.path.join(a.out, f"{i + 1:06d}.npy"), d)
            mm = np.rint(np.clip(d * 1000.0, 0.0, 65534.0)).astype(np.uint16)
            Image.fromarray(mm).save(os.path.join(a.out, f"{i + 1:06d}.depth.png"))
        print(f"{a.out}: {len(poses)} depth images")
    except (ValueError, OSError) as e:
        print(f"mesh_raycast: {e}", file=sys.stderr)
        raise SystemExit(2)


if __name__ == "__main__":
    main()
