"""Depth fusion on the device, measured: frames of the analytic room (tools/synthetic_sequence.render_analytic_room) fused into a
dense TSDF volume with colour by nicer_slam_amd.tsdf.TSDFVolume.  Needs a GPU; there is no fallback.

    python tools/bench_tsdf.py [--voxels 512 --frames 1000 --out FILE.json]

  (a) all frames in batches of 32: total time, voxel-frame updates per second (the updates are counted: every one adds 1 to a weight);
  (b) the state pass alone: a one-frame batch whose frame holds no measurement (every brick drops it: the state is read, nothing is
      written) and a one-frame batch of a real frame, as bytes per second against the streaming rate of the part;
  (c) batch sizes 1 / 8 / 32 / 128 over the same frames, alternated and repeated;
  (d) the same with culling compiled out, when the side-by-side library exists
      (NSA_BUILD_TAG=tsdfnocull NSA_EXTRA_HIPCC_FLAGS=-DNSA_X_TSDF_NOCULL python -m nicer_slam_amd.build), in a child process.
Frames are resident on the device before the clock starts; times are host clocks around work that ends in a synchronise.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

from benchlib import ROOM_HALF, ROOT, ring, time_host, write_results

STREAM_BW = 6.3e12          # bytes / s a float4 streaming copy reaches on an MI355X (8.0 TB/s HBM3E peak)


def timed(fn, repeat=1):
    """seconds of each of ``repeat`` runs of fn(), each ending in a device synchronise; no warm-up: (a) and (b) time first runs"""
    return [ms / 1e3 for ms in time_host(fn, repeat, warmup=False)]


def run(args):
    import synthetic_sequence as ss
    from nicer_slam_amd.tsdf import TSDFVolume
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: needs a GPU")
    N, n, H, W, focal = args.voxels, args.frames, 480, 640, 400.0
    vl = 1.44 / N
    poses = ring(n)
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    depth, rgb = [], []
    for lo in range(0, n, 50):
        c, d, _ = ss.render_analytic_room(torch.from_numpy(poses[lo:lo + 50]), K, H, W, "cuda", ROOM_HALF)
        depth.append(d.reshape(-1, H, W))
        rgb.append(c)
    depth, rgb = torch.cat(depth).contiguous(), torch.cat(rgb).contiguous()
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl)
    assert vol.dims == (N, N, N)
    cells = N ** 3
    res = dict(lib_tag=os.environ.get("NSA_LIB_TAG", ""), voxels=N, frames=n, image=[H, W], device=torch.cuda.get_device_name(0))

    def fuse(count, batch):
        vol.integrate(depth[:count], rgb[:count], poses[:count], K, batch=batch)

    # warm-up: every kernel once
    fuse(min(n, 8), 8)
    vol.reset()
    # (a)
    t = timed(lambda: fuse(n, 32))[0]
    updates = float(vol.weight.double().sum())
    res["a_all_frames_batch32"] = dict(seconds=t, updates=updates, updates_per_s=updates / t, nominal_voxel_frames_per_s=cells * n / t,
                                       updated_share_of_voxel_frames=updates / (cells * n), observed_voxels=float((vol.weight > 0).double().mean()))
    # (b)
    empty_d, empty_c = torch.zeros_like(depth[:1]), rgb[:1]
    t_empty = timed(lambda: vol.integrate(empty_d, empty_c, poses[:1], K, batch=1), 5)
    vol.reset()
    t_one = timed(lambda: fuse(1, 1), 1) + timed(lambda: fuse(1, 1), 4)
    touched = float((vol.weight > 0).double().sum())
    res["b_state_pass"] = dict(read_only_seconds=t_empty, read_only_bytes=20 * cells, read_only_share_of_stream=20 * cells / min(t_empty) / STREAM_BW,
                               one_frame_seconds=t_one, one_frame_bytes=20 * cells + 20 * touched,
                               one_frame_share_of_stream=(20 * cells + 20 * touched) / min(t_one[1:]) / STREAM_BW)
    # (c)
    count = min(n, args.batch_frames)
    rows = {b: [] for b in (1, 8, 32, 128)}
    for _ in range(args.repeat):
        for b in rows:
            vol.reset()
            rows[b] += timed(lambda: fuse(count, b))
    res["c_batch_sizes"] = dict(frames=count, seconds={str(b): v for b, v in rows.items()})
    return res


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--voxels", type=int, default=512)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--batch-frames", type=int, default=256, help="frames of the batch-size comparison (c)")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-child", action="store_true", help="skip (d)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    res = run(args)
    nocull = os.path.join(ROOT, "nicer_slam_amd", "lib", "libnicer_slam_amd_tsdfnocull.so")
    if not args.no_child and not os.environ.get("NSA_LIB_TAG"):
        if os.path.exists(nocull):
            cmd = [sys.executable, os.path.abspath(__file__), "--no-child"] + [f"--{k.replace('_', '-')}={getattr(args, k)}"
                                                                             for k in ("voxels", "frames", "batch_frames", "repeat")]
            r = subprocess.run(cmd, env=dict(os.environ, NSA_LIB_TAG="tsdfnocull"), capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"bench_tsdf: the run without culling failed\n{r.stdout}\n{r.stderr}")
            res["d_without_culling"] = json.loads(r.stdout.strip().splitlines()[-1])
        else:
            res["d_without_culling"] = "not measured: no side-by-side library built with -DNSA_X_TSDF_NOCULL"
    print(json.dumps(res))                                        # one line: the parent of a child run reads the last one
    if args.out:
        write_results(res, path=args.out, echo=False)


if __name__ == "__main__":
    main()
