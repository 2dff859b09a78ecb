"""Z-buffered images of a triangle mesh on the device, and what follows from them (include/nicer_slam_amd.h Section 12):

* ``render_mesh``: depth, face id, face normal, interpolated vertex colour and a headlight shade of a mesh (and point sets) from one
  pose or a stack -- what code/utils/viz.py leaves to open3d's OpenGL window.
* ``visible_faces`` / ``cull_mesh``: the faces some camera of a trajectory saw (vertices tested against the mesh's own depth images),
  compacted with ``mesh_clean.select_faces`` -- the usual visibility culling before a mesh is scored.
* ``depth_l1``: mean absolute difference of the mesh's depth images and sensor depth frames.
* ``camera_actor`` / ``trajectory_points`` / ``fly_through``: viz.py's point sets and its saved renderings, one PNG per frame.
* ``python -m nicer_slam_amd.mesh_render MESH.ply --poses P --intrinsics fx fy cx cy --size H W --out DIR [--sim3 T.npy]
  [--gt-poses P] [--cull OUT.ply --mode any --rel R] [--depth-l1 DEPTH_DIR] [--raycast] [--follow]``

Rasterisation and visibility have no CPU path: a missing GPU is an error.
"""
import argparse
import ctypes
import glob
import os
import sys

import numpy as np
import torch

from ._native import RasterViews, check, lib
from .mesh_args import checked_faces, mesh_dict_tensors, need_gpu, ptr, restore_dict, stream, workspace
from .mesh_clean import select_faces, transform_mesh
from .mesh_eval import TriIndex
from .mesh_raycast import occluded, render_depth
from .ply import read_ply, write_mesh_ply
from .tsdf import _as_numpy, _intrinsics4, world_to_camera

CHANNELS = ("depth", "face_id", "normal", "colour", "shaded")
MODES = {"any": 0, "all": 1, "frustum": 2}
N_TOTALS = 12
TOTALS = ("drawn", "bad_index", "depth", "guard", "degenerate", "backface", "atomics", "large_pairs", "items", "points_drawn",
          "points_skipped")
DEFAULT_NEAR = 0.01
METHODS = ("raster", "raycast")
DEFAULT_REL = 2.0 ** -6          # the smallest power of two for which "any" equals "frustum" on the closed room
LARGE_THRESHOLD = 256            # candidate pixel centres above which a face goes through the tile queue
QUEUE_CAPACITY = 1 << 20
PALETTE = ((1.0, 0.0, 0.0), (0.0, 0.0, 0.0))          # viz.py: estimated poses red, ground truth black
VIZ_SIZE = (990, 1760)


class _Scene:
    """the device copies one rasterisation needs: mesh, poses of every view, workspace"""

    def __init__(self, mesh, c2w, intrinsics, size, near, device="cuda"):
        self.H, self.W = int(size[0]), int(size[1])
        if not (1 <= self.H <= 16384 and 1 <= self.W <= 16384):
            raise ValueError("size: (H, W) with 1 <= H, W <= 16384")
        if not (0 < float(near) < 1e30):
            raise ValueError("near must be positive")
        self.near = float(near)
        w2c, _ = world_to_camera(c2w)
        self.n = w2c.shape[0]
        if self.n == 0:
            raise ValueError("c2w: no pose")
        K = _intrinsics4(intrinsics, self.n).astype(np.float32)
        self.per_view = K.shape[0] > 1
        need_gpu("mesh_render")
        m, self.was_numpy, self.orig = mesh_dict_tensors(mesh, device)
        self.dev = m["verts"].device
        self.verts = m["verts"].detach().float().contiguous()
        self.faces = checked_faces(m["faces"], "mesh").to(torch.int32).contiguous()
        self.colours = m["colors"].detach().float().contiguous() if "colors" in m else None
        self.w2c = torch.from_numpy(w2c).to(self.dev)
        self.K = torch.from_numpy(np.ascontiguousarray(K)).to(self.dev)
        self.ws = None

    def views(self, lo, m):
        return RasterViews(self.w2c[lo:].data_ptr(), self.K[lo:].data_ptr() if self.per_view else self.K.data_ptr(), m,
                           int(self.per_view), self.H, self.W, self.near)

    def raster(self, lo, m, points=None, point_size=4, cull_backface=False, large_threshold=LARGE_THRESHOLD,
               queue_capacity=QUEUE_CAPACITY):
        """-> (zbuf int64 [m, H, W] holding the uint64 keys, totals int64 [N_TOTALS]) for views lo .. lo + m"""
        if self.ws is None or self.ws.numel() < lib.nsa_mesh_raster_workspace(queue_capacity):
            self.ws = workspace(lib.nsa_mesh_raster_workspace(queue_capacity), self.dev)
        zbuf = torch.empty((m, self.H, self.W), dtype=torch.int64, device=self.dev)
        totals = torch.empty(N_TOTALS, dtype=torch.int64, device=self.dev)
        V, F = self.verts.shape[0], self.faces.shape[0]
        P = 0 if points is None else points.shape[0]
        v = self.views(lo, m)
        check(lib.nsa_mesh_raster(ptr(self.verts), V, ptr(self.faces), F, ptr(points), P, int(point_size), ctypes.byref(v),
                                  int(cull_backface), 1, int(large_threshold), self.ws.data_ptr(), int(queue_capacity), zbuf.data_ptr(),
                                  totals.data_ptr(), stream(self.dev)))
        return zbuf, totals

    def resolve(self, lo, m, zbuf, channels, flip_to_camera=True, point_colour=None, palette=None):
        V, F = self.verts.shape[0], self.faces.shape[0]
        shape = (m, self.H, self.W)
        out = {}
        if "face_id" in channels:
            out["face_id"] = torch.empty(shape, dtype=torch.int32, device=self.dev)
        if "depth" in channels:
            out["depth"] = torch.empty(shape, dtype=torch.float32, device=self.dev)
        if "normal" in channels:
            out["normal"] = torch.empty(shape + (3,), dtype=torch.float32, device=self.dev)
        if "colour" in channels:
            out["colour"] = torch.empty(shape + (3,), dtype=torch.float32, device=self.dev)
        if "shaded" in channels:
            out["shaded"] = torch.empty(shape, dtype=torch.float32, device=self.dev)
        P = 0 if point_colour is None else point_colour.shape[0]
        p = lambda k: out[k].data_ptr() if k in out else None
        v = self.views(lo, m)
        check(lib.nsa_mesh_raster_resolve(ptr(self.verts), V, ptr(self.faces), F, ptr(self.colours), ptr(point_colour), P, ptr(palette),
                                          0 if palette is None else palette.shape[0], ctypes.byref(v), zbuf.data_ptr(),
                                          int(flip_to_camera), p("face_id"), p("depth"), p("normal"), p("colour"), p("shaded"),
                                          stream(self.dev)))
        return out

    def visible(self, lo, m, zbuf, mode, rel, flags):
        V, F = self.verts.shape[0], self.faces.shape[0]
        v = self.views(lo, m)
        check(lib.nsa_mesh_visible(ptr(self.verts), V, ptr(self.faces), F, ctypes.byref(v), ptr(zbuf), MODES[mode], float(rel), ptr(flags),
                                   stream(self.dev)))


def _points_arg(points, dev):
    """None, an array [P, 3] (colour index 0) or (array [P, 3], colour index [P]) -> (points fp32, colour int32) on the device"""
    if points is None:
        return None, None
    idx = None
    if isinstance(points, (tuple, list)) and len(points) == 2 and np.ndim(points[1]) == 1:
        points, idx = points
    pts = torch.as_tensor(points).detach().to(dev).float().reshape(-1, 3).contiguous()
    idx = torch.zeros(pts.shape[0], dtype=torch.int32, device=dev) if idx is None else \
        torch.as_tensor(idx).to(dev).to(torch.int32).reshape(-1).contiguous()
    if idx.shape[0] != pts.shape[0]:
        raise ValueError(f"points: {idx.shape[0]} colour indices for {pts.shape[0]} points")
    return pts, idx


@torch.no_grad()
def render_mesh(mesh, c2w, intrinsics, size, near=DEFAULT_NEAR, channels=CHANNELS, points=None, batch=8, point_size=4,
                palette=PALETTE, cull_backface=False, flip_to_camera=True, large_threshold=LARGE_THRESHOLD,
                queue_capacity=QUEUE_CAPACITY, device="cuda"):
    """Images of ``mesh`` (the dict ``inference.read_ply`` / ``extract_mesh`` return: ``verts`` [V, 3], ``faces`` [F, 3], optional
    ``colors`` [V, 3]; torch on either side, or numpy) from ``c2w`` ([4, 4] or [n, 4, 4] camera-to-world; x right, y down, z forward),
    ``intrinsics`` (4 x 4, (fx, fy, cx, cy), or one per view) and ``size`` = (H, W).  Returns a dict of [n, H, W (, 3)] images, numpy
    for a numpy mesh and torch on the mesh's own device otherwise, always with the leading view axis:
      ``depth``    z-depth, 0 where nothing was drawn (``TSDFVolume.integrate``'s hole convention)
      ``face_id``  int32, -1 where nothing was drawn; a point shows as F + its index
      ``normal``   the world-space unit normal of the face, turned towards the camera with ``flip_to_camera``
      ``colour``   perspective-correct vertex colour (0 without ``colors``); a point shows ``palette[its colour index]``
      ``shaded``   the headlight term |n . v| (1 for a point)
      ``totals``   dict of per-call counts summed over the views (faces drawn and skipped by cause, atomics issued, ...)
    ``points``: [P, 3] or ([P, 3], colour index [P]) drawn as squares of ``point_size`` pixels into the same z-buffer.
    There is no near-plane clipping: a face with a vertex at or behind ``near`` is not drawn.  ``batch`` views share one pass over the
    faces; any batch size, ``large_threshold`` and ``queue_capacity`` give the same bits."""
    bad = [c for c in channels if c not in CHANNELS]
    if bad:
        raise ValueError(f"channels: unknown {bad}; choose from {CHANNELS}")
    sc = _Scene(mesh, c2w, intrinsics, size, near, device)
    pts, pidx = _points_arg(points, sc.dev)
    pal = torch.tensor(palette, dtype=torch.float32, device=sc.dev).reshape(-1, 3).contiguous() if pts is not None else None
    batch = max(1, int(batch))
    parts, totals = [], torch.zeros(N_TOTALS, dtype=torch.int64, device=sc.dev)
    for lo in range(0, sc.n, batch):
        m = min(batch, sc.n - lo)
        zbuf, t = sc.raster(lo, m, pts, point_size, cull_backface, large_threshold, queue_capacity)
        totals += t
        parts.append(sc.resolve(lo, m, zbuf, channels, flip_to_camera, pidx, pal))
    out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    out = restore_dict(out, sc.was_numpy, sc.orig)
    out["totals"] = dict(zip(TOTALS, (int(x) for x in totals.cpu())))
    return out


def _method(method):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    return method


def _visible_by_rays(sc, c2w, mode, rel):
    """bool [F]: ``visible_faces`` with the occlusion test itself in place of the depth images.  Per view, the vertices in front of
    ``near`` that project inside the image are found by the frustum test of ``"frustum"`` (the same kernel, run on one degenerate
    face per vertex); of those, a vertex is seen when nothing is hit on the way from the camera centre to it, up to 1 - rel of the way
    (``mesh_raycast.occluded``)."""
    F, V = sc.faces.shape[0], sc.verts.shape[0]
    flags = torch.zeros(F, dtype=torch.bool, device=sc.dev)
    if F == 0 or V == 0:
        return flags
    ok = ((sc.faces >= 0) & (sc.faces < V)).all(1)
    f = torch.where(ok[:, None], sc.faces, torch.zeros_like(sc.faces)).long()
    ix = TriIndex(sc.verts, sc.faces) if mode != "frustum" else None
    each = torch.arange(V, dtype=torch.int32, device=sc.dev)[:, None].expand(V, 3).contiguous()
    centres = torch.from_numpy(np.ascontiguousarray(_as_numpy(c2w, np.float64).reshape(-1, 4, 4)[:, :3, 3])).float().to(sc.dev)
    for i in range(sc.n):
        inside = torch.zeros(V, dtype=torch.uint8, device=sc.dev)
        v = sc.views(i, 1)
        check(lib.nsa_mesh_visible(sc.verts.data_ptr(), V, each.data_ptr(), V, ctypes.byref(v), None, MODES["frustum"], 0.0,
                                   inside.data_ptr(), stream(sc.dev)))
        seen = inside.bool()
        if ix is not None:
            idx = torch.nonzero(seen)[:, 0]
            hidden = occluded(ix, centres[i], sc.verts[idx], rel)
            seen[idx[hidden]] = False
        per_face = seen[f]
        flags |= ok & (per_face.all(1) if mode == "all" else per_face.any(1))
    return flags


@torch.no_grad()
def visible_faces(mesh, c2w, intrinsics, size, mode="any", rel=DEFAULT_REL, near=DEFAULT_NEAR, batch=32, device="cuda",
                  method="raster"):
    """bool [F]: the faces of ``mesh`` that some view sees.  A vertex is seen in a view when it lies in front of ``near``, projects
    inside the image and is not farther than (1 + rel) times the largest depth of the mesh's own depth image at the four pixel
    centres around it; a face is visible in a view when any (``"any"``) or all (``"all"``) of its vertices are seen there.
    ``"frustum"`` skips the depth comparison (and the rasterisation).  numpy in, numpy out; torch in, torch out.
    ``method="raycast"`` replaces the comparison with depth images by the occlusion test itself: a ray from the camera centre to the
    vertex, any hit within 1 - rel of the way hides it (``mesh_raycast.occluded``) -- independent of the image resolution, and of
    ``render_mesh``'s missing near-plane clipping."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {tuple(MODES)}, got {mode!r}")
    if not (0.0 <= float(rel) <= 1.0):
        raise ValueError("rel must lie in [0, 1]")
    _method(method)
    sc = _Scene(mesh, c2w, intrinsics, size, near, device)
    if method == "raycast":
        out = _visible_by_rays(sc, c2w, mode, min(float(rel), 0.5))
        return out.cpu().numpy() if sc.was_numpy else out.to(sc.orig)
    flags = torch.zeros(sc.faces.shape[0], dtype=torch.uint8, device=sc.dev)
    batch = max(1, int(batch))
    for lo in range(0, sc.n, batch):
        m = min(batch, sc.n - lo)
        zbuf = sc.raster(lo, m)[0] if mode != "frustum" else None
        sc.visible(lo, m, zbuf, mode, rel, flags)
    out = flags.bool()
    return out.cpu().numpy() if sc.was_numpy else out.to(sc.orig)


def cull_mesh(mesh, c2w, intrinsics, size, mode="any", rel=DEFAULT_REL, near=DEFAULT_NEAR, batch=32, device="cuda", method="raster"):
    """``mesh`` without the faces no view sees (``visible_faces``), compacted by ``mesh_clean.select_faces``: face and vertex order
    are kept."""
    return select_faces(mesh, visible_faces(mesh, c2w, intrinsics, size, mode, rel, near, batch, device, method))


@torch.no_grad()
def depth_l1(mesh, depth_frames, c2w, intrinsics, near=DEFAULT_NEAR, batch=8, device="cuda", method="raster"):
    """(mean |mesh depth - frame depth| over the pixels valid in both, their count): ``depth_frames`` [n, H, W] (or [H, W]) with the
    hole convention of ``TSDFVolume.integrate`` (valid: finite and > 0).  The differences are formed and summed in float64.
    (nan, 0) when no pixel is valid in both.  ``method="raycast"`` takes the mesh depth from ``mesh_raycast.render_depth``: faces that
    straddle the camera count."""
    _method(method)
    d = torch.as_tensor(depth_frames)
    if d.dim() == 2:
        d = d[None]
    if d.dim() != 3:
        raise ValueError("depth_frames: [H, W] or [n, H, W]")
    sc = _Scene(mesh, c2w, intrinsics, d.shape[1:], near, device)
    if sc.n != d.shape[0]:
        raise ValueError(f"c2w: {sc.n} poses for {d.shape[0]} frames")
    total = torch.zeros((), dtype=torch.float64, device=sc.dev)
    count = 0
    batch = max(1, int(batch))
    ix = None
    for lo in range(0, sc.n, batch):
        m = min(batch, sc.n - lo)
        if method == "raycast":
            if ix is None:
                ix = TriIndex(sc.verts, sc.faces)
                c2w_all, K_all = _as_numpy(c2w, np.float64).reshape(-1, 4, 4), _intrinsics4(intrinsics, sc.n)
            r = render_depth(ix, c2w_all[lo:lo + m], K_all[lo:lo + m] if K_all.shape[0] > 1 else K_all, (sc.H, sc.W), near,
                             ("depth",))["depth"].to(sc.dev)
        else:
            zbuf, _ = sc.raster(lo, m)
            r = sc.resolve(lo, m, zbuf, ("depth",))["depth"].double()
        g = d[lo:lo + m].to(sc.dev).double()
        ok = (r > 0) & torch.isfinite(g) & (g > 0)
        total += (r - g).abs()[ok].sum()
        count += int(ok.sum())
    return (float(total) / count if count else float("nan")), count


# --------------------------------------------------------------------------------------------------------------- viz.py's point sets
def _actor_segments():
    """The camera glyph of viz.py in the camera frame, restated from its geometry: a pyramid with its apex at the optical centre and
    a 2 x 2 base at depth 1.5 (four sides, the two diagonals of the base, four edges to the apex), and a roof-shaped "up" mark on
    the base's +y side from (-0.5, 1) over (0, 1.2) to (0.5, 1).  -> [12, 2, 3] segment end points."""
    z = 1.5
    corners = [(-1.0, -1.0, z), (1.0, -1.0, z), (1.0, 1.0, z), (-1.0, 1.0, z)]
    apex = (0.0, 0.0, 0.0)
    seg = [(corners[k], corners[(k + 1) % 4]) for k in range(4)]
    seg += [(corners[0], corners[2]), (corners[1], corners[3])]
    seg += [(corners[0], apex), (apex, corners[1]), (corners[2], apex), (apex, corners[3])]
    seg += [((-0.5, 1.0, z), (0.0, 1.2, z)), ((0.0, 1.2, z), (0.5, 1.0, z))]
    return np.asarray(seg, dtype=np.float64)


def unscaled_pose(c2w):
    """the pose with each of its first three columns normalised (a zero column is left alone), as viz.py shows poses"""
    P = np.array(_as_numpy(c2w, np.float64), dtype=np.float64).reshape(4, 4)
    for k in range(3):
        length = np.linalg.norm(P[:3, k])
        if length > 0:
            P[:, k] /= length
    return P


def camera_actor(c2w, scale=0.005, gt=False, samples=100):
    """(points float32 [12 * samples, 3] in the world, colour index [same] int32: 0 estimated (red), 1 ground truth (black)): the camera
    glyph at pose ``c2w``, every segment sampled at ``samples`` evenly spaced points with both ends."""
    seg = _actor_segments() * float(scale)
    t = np.linspace(0.0, 1.0, int(samples))[None, :, None]
    local = (seg[:, :1] * (1.0 - t) + seg[:, 1:] * t).reshape(-1, 3)
    P = unscaled_pose(c2w)
    world = local @ P[:3, :3].T + P[:3, 3]
    return world.astype(np.float32), np.full(len(world), 1 if gt else 0, dtype=np.int32)


def trajectory_points(c2w_list, gt=False, upto=None):
    """(points [m, 3] float32, colour index [m]): the camera centres of poses 1 .. upto - 1 (viz.py draws ``c2w_list[1:i, :3, 3]``)"""
    P = _as_numpy(c2w_list, np.float64).reshape(-1, 4, 4)
    pts = P[1:(len(P) if upto is None else int(upto)), :3, 3]
    return np.ascontiguousarray(pts, dtype=np.float32), np.full(len(pts), 1 if gt else 0, dtype=np.int32)


def behind_first(c2w, back=0.2):
    """viz.py's viewer: the first pose moved ``back`` along its own negative z axis"""
    P = np.array(_as_numpy(c2w, np.float64), dtype=np.float64).reshape(4, 4)
    z = P[:3, 2]
    P[:3, 3] -= back * z / np.linalg.norm(z)
    return P


def default_intrinsics(size, fov_deg=60.0):
    """a pinhole with a vertical field of view of ``fov_deg`` and the principal point at the image centre (open3d's default view)"""
    H, W = size
    f = 0.5 * H / np.tan(np.radians(fov_deg) / 2.0)
    return np.array([f, f, (W - 1) / 2.0, (H - 1) / 2.0])


def to_uint8(image):
    x = torch.as_tensor(image).detach().float().cpu().numpy()
    return np.rint(np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8)


def write_png(path, image):
    """[H, W] or [H, W, 3] in [0, 1] -> 8-bit PNG"""
    from PIL import Image
    Image.fromarray(to_uint8(image)).save(path)


def read_poses(path):
    """camera-to-world [n, 4, 4] float64 from a .npy ([n, 4, 4]), a text file of n rows of 16 (or 4 n rows of 4) values, or a directory
    of frame-*.pose.txt files (7-Scenes)"""
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "*.pose.txt"))) or sorted(glob.glob(os.path.join(path, "*.txt")))
        if not files:
            raise ValueError(f"{path}: no pose files")
        P = np.stack([np.loadtxt(f, dtype=np.float64).reshape(4, 4) for f in files])
    elif path.endswith(".npy"):
        P = np.load(path).astype(np.float64)
    else:
        P = np.loadtxt(path, dtype=np.float64)
    if P.size == 0 or P.size % 16:
        raise ValueError(f"{path}: not a list of 4 x 4 poses")
    P = P.reshape(-1, 4, 4)
    if not np.isfinite(P).all():
        raise ValueError(f"{path}: a pose is not finite")
    return P


def read_depth_dir(path, n):
    """the first n depth frames of a directory: *.depth.png (uint16 millimetres, 0 and 65535 = hole) or *.npy (metres)"""
    from PIL import Image
    pngs = sorted(glob.glob(os.path.join(path, "*.depth.png")))
    npys = sorted(glob.glob(os.path.join(path, "*.npy")))
    if len(pngs) >= n:
        out = []
        for f in pngs[:n]:
            raw = np.array(Image.open(f)).astype(np.int64)
            d = raw.astype(np.float32) / np.float32(1000.0)
            d[(raw <= 0) | (raw >= 65535)] = 0.0
            out.append(d)
        return np.stack(out)
    if len(npys) >= n:
        return np.stack([np.load(f).astype(np.float32) for f in npys[:n]])
    raise ValueError(f"{path}: fewer than {n} depth frames (*.depth.png or *.npy)")


@torch.no_grad()
def fly_through(mesh_or_paths, est_c2w, gt_c2w=None, sim3=None, out_dir=".", viewpoint="behind_first", size=VIZ_SIZE, intrinsics=None,
                near=DEFAULT_NEAR, cam_scale=0.05, point_size=4, background=1.0, device="cuda"):
    """viz.py's saved rendering: for frame i the mesh (one for all frames, or a list of PLY paths / mesh dicts, one per frame) moved by
    ``sim3``, the camera glyphs of the estimated (red) and ground-truth (black) pose i and both trajectories up to i, drawn as points
    into the same z-buffer, seen from ``viewpoint``: "behind_first" (0.2 behind the first estimated pose along its z axis, fixed) or
    "follow" (0.2 behind the current one).  The picture is the vertex colour times the headlight shade (grey without colours) on
    ``background``; one ``%06d.png`` per frame in ``out_dir``.  Returns the list of files."""
    if viewpoint not in ("behind_first", "follow"):
        raise ValueError("viewpoint must be 'behind_first' or 'follow'")
    est = _as_numpy(est_c2w, np.float64).reshape(-1, 4, 4)
    gt = None if gt_c2w is None else _as_numpy(gt_c2w, np.float64).reshape(-1, 4, 4)
    if gt is not None and len(gt) != len(est):
        raise ValueError(f"gt_c2w: {len(gt)} poses for {len(est)} estimated ones")
    per_frame = isinstance(mesh_or_paths, (list, tuple))
    if per_frame and len(mesh_or_paths) != len(est):
        raise ValueError(f"{len(mesh_or_paths)} meshes for {len(est)} poses")
    K = default_intrinsics(size) if intrinsics is None else intrinsics
    os.makedirs(out_dir, exist_ok=True)

    def load(m):
        m = read_ply(m) if isinstance(m, str) else m
        return transform_mesh(m, sim3) if sim3 is not None else m

    mesh = None if per_frame else load(mesh_or_paths)
    files = []
    for i in range(len(est)):
        cur = load(mesh_or_paths[i]) if per_frame else mesh
        sets = [camera_actor(est[i], cam_scale, False), trajectory_points(est, False, i + 1)]
        if gt is not None:
            sets += [camera_actor(gt[i], cam_scale, True), trajectory_points(gt, True, i + 1)]
        pts = np.concatenate([s[0] for s in sets])
        idx = np.concatenate([s[1] for s in sets])
        eye = behind_first(unscaled_pose(est[0] if viewpoint == "behind_first" else est[i]))
        r = render_mesh(cur, eye, K, size, near, ("colour", "shaded", "face_id"), (pts, idx), 1, point_size, device=device)
        fid = torch.as_tensor(r["face_id"][0])
        shade = torch.as_tensor(r["shaded"][0]).float()
        F = int(np.shape(cur["faces"])[0])
        base = torch.as_tensor(r["colour"][0]).float() if "colors" in cur else torch.full(tuple(fid.shape) + (3,), 0.8)
        base = base.to(shade.device)
        base = torch.where((fid >= F)[..., None].to(shade.device), torch.as_tensor(r["colour"][0]).float().to(shade.device), base)
        img = torch.where((fid >= 0)[..., None].to(shade.device), base * shade[..., None], torch.full_like(base, float(background)))
        path = os.path.join(out_dir, f"{i + 1:06d}.png")
        write_png(path, img)
        files.append(path)
    return files


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_render", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--poses", required=True, help="estimated camera-to-world poses: .npy [n, 4, 4], text, or a directory of *.pose.txt")
    ap.add_argument("--intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"), required=True,
                    help="the camera of the poses (used by --cull and --depth-l1)")
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"), required=True, help="its image size")
    ap.add_argument("--out", help="directory for the fly-through PNGs (viewer: 990 x 1760, 60 degrees)")
    ap.add_argument("--sim3", metavar="T.npy", help="4x4 similarity applied to the mesh first")
    ap.add_argument("--gt-poses")
    ap.add_argument("--cull", metavar="OUT.ply", help="write the mesh culled to what the poses saw")
    ap.add_argument("--mode", choices=tuple(MODES), default="any")
    ap.add_argument("--rel", type=float, default=DEFAULT_REL)
    ap.add_argument("--near", type=float, default=DEFAULT_NEAR)
    ap.add_argument("--depth-l1", metavar="DEPTH_DIR", help="print the depth L1 against the frames of this directory")
    ap.add_argument("--raycast", action="store_true", help="--cull and --depth-l1 by casting rays (method='raycast')")
    ap.add_argument("--follow", action="store_true", help="the viewer follows the current pose")
    ap.add_argument("--viewer-size", type=int, nargs=2, metavar=("H", "W"), default=list(VIZ_SIZE))
    a = ap.parse_args(argv)
    if not (a.out or a.cull or a.depth_l1):
        ap.error("nothing to do: give --out, --cull or --depth-l1")
    if a.size[0] < 1 or a.size[1] < 1 or a.viewer_size[0] < 1 or a.viewer_size[1] < 1:
        ap.error("image sizes must be positive")
    if not (0.0 <= a.rel <= 1.0):
        ap.error("--rel must lie in [0, 1]")
    if not a.near > 0:
        ap.error("--near must be positive")
    return a


def main(argv=None):
    a = parse_args(argv)
    try:
        mesh = read_ply(a.mesh)
        if a.sim3:
            mesh = transform_mesh(mesh, np.load(a.sim3))
        poses = read_poses(a.poses)
        gt = read_poses(a.gt_poses) if a.gt_poses else None
        if a.depth_l1:
            frames = read_depth_dir(a.depth_l1, len(poses))
            if tuple(frames.shape[1:]) != tuple(a.size):
                raise ValueError(f"{a.depth_l1}: frames of {frames.shape[1:]} for --size {a.size}")
            l1, count = depth_l1(mesh, frames, poses, a.intrinsics, a.near, method="raycast" if a.raycast else "raster")
            print(f"depth L1 {l1:.6f} over {count} pixels")
        if a.cull:
            culled = cull_mesh(mesh, poses, a.intrinsics, a.size, a.mode, a.rel, a.near, method="raycast" if a.raycast else "raster")
            print(f"{a.cull}: kept {culled['faces'].shape[0]} of {mesh['faces'].shape[0]} faces, "
                  f"{culled['verts'].shape[0]} of {mesh['verts'].shape[0]} vertices")
            write_mesh_ply(a.cull, culled)
        if a.out:
            files = fly_through(mesh, poses, gt, None, a.out, "follow" if a.follow else "behind_first", tuple(a.viewer_size), near=a.near)
            print(f"{a.out}: {len(files)} images")
    except (ValueError, OSError) as e:
        print(f"mesh_render: {e}", file=sys.stderr)
        raise SystemExit(2)


if __name__ == "__main__":
    main()
