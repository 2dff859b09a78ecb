"""Time the ray cast against a mesh on one MI355X, beside the rasteriser that produces the same images:
one 480 x 640 view of a marching-cubes sphere (128^3 by default) through mesh_raycast.render_depth and through
mesh_render.render_mesh, and a 1024-pixel mesh_raycast.depth_at batch beside the whole frame one would otherwise rasterise to read
those pixels; the tree build, its bytes, and the nodes visited and faces tested per ray (the kernel's own counts).  The index of the
ray cast is built once outside the timed window, as a tracking or mapping loop would hold it; the rasteriser has no index to build.
Device events, warm-up first, medians of `reps` runs with their spread; the two sides alternate within one process.
usage: python tools/bench_raycast.py [reps=20] [resolution=128] [out=profiles/raycast_bench.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from nicer_slam_amd import inference, mesh_raycast, mesh_render
from nicer_slam_amd.mesh_eval import TriIndex

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
RES = int(sys.argv[2]) if len(sys.argv) > 2 else 128
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "raycast_bench.json")
H, W = 480, 640


def mc_sphere(res, r=0.5, bound=1.0):
    ax = torch.linspace(-bound, bound, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - r).float().cuda()
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol, 0.0, (step,) * 3, (-bound,) * 3)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def timed_pair(a, b, reps=REPS):
    """medians and (min, max) in ms of a() and b(), alternating, after one warm-up of each"""
    out = []
    for fn in (a, b):
        fn()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((a, b)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms[k].append(t0.elapsed_time(t1))
    for m in ms:
        out.append({"median ms": float(np.median(m)), "min ms": float(min(m)), "max ms": float(max(m))})
    return out


def main():
    assert torch.cuda.is_available(), "bench_raycast.py needs an MI355X"
    m = mc_sphere(RES)
    mesh = {"verts": m["verts"], "faces": m["faces"]}
    out = {"device": torch.cuda.get_device_name(0), "resolution": RES, "faces": int(m["faces"].shape[0]), "view": [H, W], "reps": REPS}
    c2w = look_at((1.6, 0.9, 0.7), (0.0, 0.0, 0.0))
    K = (700.0, 700.0, (W - 1) / 2.0, (H - 1) / 2.0)                     # the sphere fills most of the frame's height
    ix = TriIndex(mesh["verts"], mesh["faces"])

    def build():
        ix._ray = None
        ix._ray_tree()

    build()
    torch.cuda.synchronize()
    out["tree build"] = timed_pair(build, build)[0]
    out["tree layout"] = ix.ray_layout()

    cast, drawn = timed_pair(lambda: mesh_raycast.render_depth(ix, c2w, K, (H, W), channels=("depth", "face_id", "normal")),
                             lambda: mesh_render.render_mesh(mesh, c2w, K, (H, W), channels=("depth", "face_id", "normal")))
    out["full frame render_depth"], out["full frame render_mesh"] = cast, drawn
    out["full frame render_depth / render_mesh"] = cast["median ms"] / drawn["median ms"]
    o, d = mesh_raycast.camera_rays(c2w, K, (H, W), device="cuda")
    order = mesh_raycast._tile_order(H, W, o.device)
    kernel, rows = timed_pair(lambda: ix.raycast(o[order], d[order], tmin=0.01), lambda: ix.raycast(o, d, tmin=0.01))
    out["full frame raycast alone, 8 x 8 tiles"], out["full frame raycast alone, row-major rays"] = kernel, rows
    t, face, _, nodes, tested = ix.raycast(o, d, tmin=0.01, counts=True)
    out["full frame rays"] = {"rays": int(o.shape[0]), "hit": int((face >= 0).sum()), "nodes visited/ray": float(nodes.double().mean()),
                              "faces tested/ray": float(tested.double().mean()), "faces tested/ray, max": int(tested.max()),
                              "usable faces": out["tree layout"]["usable faces"]}
    a = mesh_raycast.render_depth(ix, c2w, K, (H, W), channels=("depth", "face_id"))
    b = mesh_render.render_mesh(mesh, c2w, K, (H, W), channels=("depth", "face_id"))
    both = (a["face_id"][0] >= 0) & (b["face_id"][0] >= 0)
    out["full frame agreement"] = {"pixels hit in both": int(both.sum()),
                                   "same face": float((a["face_id"][0] == b["face_id"][0])[both].double().mean()),
                                   "max |depth difference|": float((a["depth"][0] - b["depth"][0].double())[both].abs().max())}

    g = torch.Generator().manual_seed(0)
    px = torch.stack([torch.randint(W, (1024,), generator=g), torch.randint(H, (1024,), generator=g)], 1).cuda()
    batch, frame = timed_pair(lambda: mesh_raycast.depth_at(ix, c2w, K, px),
                              lambda: mesh_render.render_mesh(mesh, c2w, K, (H, W), channels=("depth", "face_id", "normal")))
    out["1024-pixel depth_at"], out["the frame rasterised for them"] = batch, frame
    out["1024-pixel depth_at / rasterised frame"] = batch["median ms"] / frame["median ms"]
    po, pd = mesh_raycast.camera_rays(c2w, K, (H, W), px, device="cuda")
    alone, rays = timed_pair(lambda: ix.raycast(po, pd, tmin=0.01), lambda: mesh_raycast.camera_rays(c2w, K, (H, W), px, device="cuda"))
    out["1024 rays raycast alone"], out["1024 camera rays made in torch"] = alone, rays
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
