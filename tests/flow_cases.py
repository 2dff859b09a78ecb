"""Inputs of the flow ground-truth tests (tests/test_flow_cues_cpu.py, tests/test_flow_cues_gpu.py): an analytic scene with a
foreground rectangle, so that both views of a pair hide part of what the other sees, and the pose pairs it is seen from.

Scene (world = the first "lateral" camera's frame): the back plane 0.2 x + 0.1 y + z = 2 and, in front of it, the rectangle
|x| < 0.3, |y| < 0.25 at z = 1.  Cameras look along +z; fx = fy = 60, principal point at the image centre."""
import functools

import numpy as np

PLANE_N = np.array([0.2, 0.1, 1.0])
PLANE_D = 2.0
RECT = (0.3, 0.25, 1.0)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def pose(angle_y, t):
    P = np.eye(4)
    P[:3, :3] = rot_y(angle_y)
    P[:3, 3] = t
    return P


POSE_PAIRS = {
    "lateral": (pose(0.0, (0.0, 0.0, 0.0)), pose(-0.08, (0.25, 0.02, 0.0))),
    "forward": (pose(0.05, (-0.1, 0.0, 0.0)), pose(-0.03, (0.1, 0.03, 0.25))),
}
SIZES = {"base": (48, 64), "odd": (37, 53)}


def intrinsics(H, W):
    return np.array([60.0, 60.0, (W - 1) / 2.0, (H - 1) / 2.0])


def render_depth(c2w, H, W):
    """z-depth [H, W] float32 of the scene from camera c2w (float64 ray casting, rounded once)."""
    fx, fy, cx, cy = intrinsics(H, W)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    d = d_cam @ c2w[:3, :3].T
    o = c2w[:3, 3]
    s_plane = (PLANE_D - PLANE_N @ o) / (d @ PLANE_N)
    s_rect = (RECT[2] - o[2]) / d[..., 2]
    hit = o + s_rect[..., None] * d
    on = (np.abs(hit[..., 0]) < RECT[0]) & (np.abs(hit[..., 1]) < RECT[1]) & (s_rect > 0) & (s_rect < s_plane)
    return np.where(on, s_rect, s_plane).astype(np.float32)


def punch_holes(depth):
    """A copy with blocks and single pixels of 0, -1, NaN and +inf (the same places in every frame)."""
    d = depth.copy()
    H, W = d.shape[-2:]
    d[..., 3:9, 5:14] = 0.0
    d[..., H // 2:H // 2 + 4, W // 2 - 3:W // 2 + 6] = np.nan
    d[..., H - 7:H - 2, 2:7] = -1.0
    d[..., 1:5, W - 8:W - 1] = np.inf
    for k, bad in enumerate((0.0, -1.0, np.nan, np.inf)):
        d[..., (7 * k + 11) % H, (13 * k + 17) % W] = bad
        d[..., H - 1 - (5 * k) % H, (3 * k) % W] = bad
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> dict(depth [n, H, W] fp32, c2w [n, 4, 4], K [4], H, W, pairs [(i, j) directed, both directions of each unordered pair]).
    The analytic pairs: "lateral", "forward" (48 x 64), "lateral_odd", "forward_odd" (37 x 53), "lateral_holes", "identity"."""
    base, _, variant = name.partition("_")
    H, W = SIZES["odd" if variant == "odd" else "base"]
    if base == "identity":
        P = POSE_PAIRS["forward"][0]
        c2w = np.stack([P, P.copy()])
    else:
        c2w = np.stack(POSE_PAIRS[base])
    depth = np.stack([render_depth(P, H, W) for P in c2w])
    if variant == "holes":
        depth = punch_holes(depth)
    return dict(depth=depth, c2w=c2w, K=intrinsics(H, W), H=H, W=W, pairs=[(0, 1), (1, 0)])


ANALYTIC = ("lateral", "forward", "lateral_odd", "forward_odd")
ALL_CASES = ANALYTIC + ("lateral_holes", "identity")


@functools.lru_cache(maxsize=None)
def many_edges():
    """Seven edges with repeated frames over the four cameras of both pose pairs at 37 x 53, per-frame intrinsics."""
    H, W = SIZES["odd"]
    c2w = np.stack(POSE_PAIRS["lateral"] + POSE_PAIRS["forward"])
    depth = punch_holes(np.stack([render_depth(P, H, W) for P in c2w]))
    K = np.stack([intrinsics(H, W) * s for s in (1.0, 1.05, 0.95, 1.0)])
    src = [0, 1, 2, 3, 0, 3, 1]
    dst = [1, 0, 3, 2, 3, 0, 1]
    Km = np.tile(np.eye(4), (4, 1, 1))                   # (four rows of four would read as ONE 4 x 4 matrix: pass the matrices)
    Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2] = K.T
    return dict(depth=depth, c2w=c2w, K=K, K_matrices=Km, H=H, W=W, src=src, dst=dst)


@functools.lru_cache(maxsize=None)
def random_flows(P=3, seed=5):
    """Random fp32 flows up to 8 px at 37 x 53, and validity maps with a tenth of the pixels invalid, for the consistency kernel alone.
    The last pair is white noise (nearly everything occluded, many landings outside the image); the others are smooth random fields
    with bwd = -fwd plus noise around the rule's threshold, so that both outcomes are common."""
    H, W = SIZES["odd"]
    g = np.random.default_rng(seed)
    fwd = (g.uniform(-8, 8, (P, H, W, 2))).astype(np.float32)
    bwd = (g.uniform(-8, 8, (P, H, W, 2)) * g.uniform(0, 1, (P, H, W, 1))).astype(np.float32)
    v, u = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    for p in range(P - 1):
        a = g.uniform(0, 2 * np.pi, 4)
        f = np.stack([5.0 * np.sin(2.0 * u + 1.5 * v + a[0]) + 3.0 * np.cos(3.0 * v + a[1]),
                      4.0 * np.cos(2.5 * u - v + a[2]) + 4.0 * np.sin(2.0 * u + a[3])], -1)
        fwd[p] = f.astype(np.float32)
        bwd[p] = (-f + g.uniform(-0.55, 0.55, (H, W, 2))).astype(np.float32)
    fv = g.uniform(size=(P, H, W)) > 0.1
    bv = g.uniform(size=(P, H, W)) > 0.1
    return fwd, bwd, fv, bv


@functools.lru_cache(maxsize=None)
def three_frames():
    """Three frames of the scene at 48 x 64 (the keyframes "0", "10", "20" of the end-to-end test): depth as the renderer would see it,
    and a copy with holes as a sensor would deliver it."""
    H, W = SIZES["base"]
    c2w = np.stack(POSE_PAIRS["lateral"] + (pose(0.04, (-0.15, -0.02, 0.1)),))
    depth = np.stack([render_depth(P, H, W) for P in c2w])
    return dict(depth=depth, depth_holes=punch_holes(depth), c2w=c2w, K=intrinsics(H, W), H=H, W=W)


def hidden_behind_rectangle(c2w_src, c2w_dst, depth_src, K, shrink=0.04):
    """[H, W] bool: the pixel of the source frame shows the back plane, and the straight line from the target camera to that point
    passes through the rectangle shrunk by ``shrink`` on every side (about 2.4 pixels at fx = 60, z = 1) -- the part of the
    rectangle's shadow that any sound occlusion test must mask, clear of the silhouette where the bilinear taps mix both surfaces."""
    fx, fy, cx, cy = K
    H, W = depth_src.shape
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = depth_src.astype(np.float64)
    cam = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], -1)
    world = cam @ c2w_src[:3, :3].T + c2w_src[:3, 3]
    on_plane = np.abs(world @ PLANE_N - PLANE_D) < 1e-5
    o = c2w_dst[:3, 3]
    s = (RECT[2] - o[2]) / (world[..., 2] - o[2])                       # where the line o -> world crosses z = 1 (world at s = 1)
    hit = o + s[..., None] * (world - o)
    return on_plane & (s > 0) & (s < 1) & (np.abs(hit[..., 0]) < RECT[0] - shrink) & (np.abs(hit[..., 1]) < RECT[1] - shrink)
