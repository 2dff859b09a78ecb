"""Time the ray cast against a mesh on one MI355X, beside the rasteriser that produces the same images:
one 480 x 640 view of a marching-cubes sphere (128^3 by default) through mesh_raycast.render_depth and through
mesh_render.render_mesh, and a 1024-pixel mesh_raycast.depth_at batch beside the whole frame one would otherwise rasterise to read
those pixels; the tree build, its bytes, and the nodes visited and faces tested per ray (the kernel's own counts).  The index of the
ray cast is built once outside the timed window, as a tracking or mapping loop would hold it; the rasteriser has no index to build.
Device events, warm-up first, medians of `reps` runs with their spread; the two sides alternate within one process.
usage: python tools/bench_raycast.py [reps=20] [resolution=128] [out=profiles/raycast_bench.json]"""
import sys

import torch

from benchlib import look_at, mc_sphere, median_min_max, positionals, time_pair, write_results
from nicer_slam_amd import mesh_raycast, mesh_render
from nicer_slam_amd.mesh_eval import TriIndex

H, W = 480, 640


def parse_args(argv):
    return positionals(argv, reps=(int, 20), resolution=(int, 128), out=(str, None))     # out: None is profiles/raycast_bench.json


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    REPS, RES = args.reps, args.resolution
    assert torch.cuda.is_available(), "bench_raycast.py needs an MI355X"

    def timed_pair(fa, fb):
        """median, min and max in ms of fa() and fb(), alternating, after one warm-up of each"""
        return [dict(zip(("median ms", "min ms", "max ms"), median_min_max(ms))) for ms in time_pair(fa, fb, REPS)]

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
    write_results(out, "raycast_bench.json", args.out)


if __name__ == "__main__":
    main()
