"""Time mesh rasterisation and visibility on two meshes at 680 x 1200: the model mesh of tools/bench_mesh.py and the TSDF
mesh of the analytic room of tools/bench_tsdf.py.  Per mesh: milliseconds per view and faces per second for the z-buffer pass at batches
of 1 / 8 / 32 views, with and without the large-face queue; resolve; a 1000-view ``visible_faces`` run; the 64-bit atomics issued per
view (= covered (face, pixel) pairs, counted by the kernel).  Device events, medians after a warm-up; kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  Also times the numpy oracle on a small case: the only runnable baseline.
usage: python tools/bench_mesh_render.py [--model-res 512] [--room-voxels 256] [--views 32] [--visible-views 1000] [--reps 5] [--json OUT]"""
import argparse
import json
import time

import numpy as np
import torch

from benchlib import ROOM_HALF, model_mesh, ring, time_events, write_results

H, W, FOCAL = 680, 1200, 600.0


def timed(fn, reps):
    """the upper middle sample of ``reps`` (the median for an odd count, such as the default)"""
    return sorted(time_events(fn, reps))[reps // 2]


def room_mesh(voxels, frames=64):
    import synthetic_sequence as ss
    from nicer_slam_amd.tsdf import TSDFVolume
    poses = ring(frames)
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 400.0
    K[0, 2], K[1, 2] = 319.5, 239.5
    c, d, _ = ss.render_analytic_room(torch.from_numpy(poses), K, 480, 640, "cuda", ROOM_HALF)
    vl = 1.44 / voxels
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl, color=False)
    vol.integrate(d.reshape(-1, 480, 640), None, poses, K)
    return vol.extract_mesh()


def bench(name, mesh, poses, args):
    from nicer_slam_amd import mesh_render as mr
    K = (FOCAL, FOCAL, (W - 1) / 2.0, (H - 1) / 2.0)
    F = int(mesh["faces"].shape[0])
    res = dict(mesh=name, V=int(mesh["verts"].shape[0]), F=F, image=[H, W], views=len(poses))
    sc = mr._Scene(mesh, poses, K, (H, W), mr.DEFAULT_NEAR)
    rows = {}
    for batch in (1, 8, 32):
        m = min(batch, sc.n)
        for label, thr in (("queue", mr.LARGE_THRESHOLD), ("one_lane_per_face_only", 0xFFFFFFFF)):
            ms = timed(lambda: sc.raster(0, m, large_threshold=thr), args.reps)
            rows[f"batch{batch}_{label}"] = dict(ms_per_view=ms / m, face_views_per_s=F * m / (ms * 1e-3))
    res["raster"] = rows
    zbuf, totals = sc.raster(0, min(32, sc.n))
    t = dict(zip(mr.TOTALS, (int(x) for x in totals.cpu())))
    res["totals_batch32"] = t
    res["atomics_per_view"] = t["atomics"] / min(32, sc.n)
    res["resolve_all_channels_ms_per_view"] = timed(lambda: sc.resolve(0, min(32, sc.n), zbuf, mr.CHANNELS), args.reps) / min(32, sc.n)
    res["resolve_depth_ms_per_view"] = timed(lambda: sc.resolve(0, min(32, sc.n), zbuf, ("depth",)), args.reps) / min(32, sc.n)
    many = np.concatenate([poses] * (args.visible_views // len(poses) + 1))[:args.visible_views]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vis = mr.visible_faces(mesh, many, K, (H, W))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res["visible_faces"] = dict(views=len(many), seconds=dt, ms_per_view=1e3 * dt / len(many), visible_share=float(vis.float().mean()),
                                face_views_per_s=F * len(many) / dt)
    # bytes the z-buffer pass must move: 12 B per face and 36 B of vertex gathers once per batch, 8 B per pixel of z-buffer per view
    res["bytes_per_view_batch32"] = (48 * F) / 32 + 8 * H * W
    return res


def oracle_baseline():
    import raster_ref as rr
    import tsdf_ref
    mesh = rr.room_mesh(8)
    poses = tsdf_ref.ring_poses(4)
    h, w = 120, 160
    K = tsdf_ref.shared_K4(h, w, 100.0)
    t0 = time.perf_counter()
    rr.raster(mesh["verts"], mesh["faces"], rr.w2c_rows(poses), K, h, w, 0.01)
    dt = time.perf_counter() - t0
    from nicer_slam_amd import mesh_render as mr
    sc = mr._Scene(mesh, poses, K[0], (h, w), 0.01)
    ms = timed(lambda: sc.raster(0, 4), 5)
    return dict(mesh="room 8 x 8 per wall", F=len(mesh["faces"]), image=[h, w], views=4, numpy_oracle_ms_per_view=1e3 * dt / 4,
                device_ms_per_view=ms / 4)


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model-res", type=int, default=512)
    ap.add_argument("--room-voxels", type=int, default=256)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--visible-views", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    return ap.parse_args(argv)


@torch.no_grad()
def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_render: needs a GPU")
    poses = ring(args.views).astype(np.float64)
    out = dict(device=torch.cuda.get_device_name(0), results=[])
    if args.room_voxels:
        out["results"].append(bench(f"tsdf room {args.room_voxels}^3", room_mesh(args.room_voxels), poses, args))
        print(json.dumps(out["results"][-1]), flush=True)
    if args.model_res:
        out["results"].append(bench(f"model {args.model_res}^3", model_mesh(args.model_res), poses, args))
        print(json.dumps(out["results"][-1]), flush=True)
    out["oracle_baseline"] = oracle_baseline()
    print(json.dumps(out["oracle_baseline"]), flush=True)
    if args.json:
        write_results(out, path=args.json, echo=False)            # (every row was printed as it was made)


if __name__ == "__main__":
    main()
