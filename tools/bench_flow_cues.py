"""Time the flow ground truth from depth and poses: flow_cues.pair_cues at 680 x 1200 over the first 32 pairs of
pair_list(2000) (16 unordered pairs of the keyframes 0, 10, .., 70 of a synthetic sequence: a tilted plane behind a rectangle, seen
from a slowly moving camera), its two kernels on their own (the C entry points on preallocated device buffers, nothing of the host
in the window) with the bytes they have to move over the time, against the rate a device-to-device copy of 1 GiB reaches in the same
run, and the float64 torch restatement of the same rule (world-coordinate composition, grid_sample) on the same device for context.
Frames are resident on the device; device events around CALLS back-to-back calls, warm-up first, median of REPS.  Needs a GPU; there is no fallback.
usage: python tools/bench_flow_cues.py [reps=7] [out.json]"""
import sys

import numpy as np
import torch
import torch.nn.functional as F

from benchlib import median_min_max, positionals, time_events, write_results
from nicer_slam_amd import flow_cues as fc
from nicer_slam_amd._native import check, lib

CALLS = 20
H, W = 680, 1200
K4 = (600.0, 600.0, 599.5, 339.5)


def parse_args(argv):
    return positionals(argv, reps=(int, 7), out=(str, None))


def scene(n):
    """n camera-to-world poses drifting sideways and forwards, and the z-depth [n, H, W] fp32 they see (float64 on the device)."""
    fx, fy, cx, cy = K4
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"), torch.arange(W, dtype=torch.float64, device="cuda"),
                          indexing="ij")
    dirs = torch.stack([(u - cx) / fx, (v - cy) / fy, torch.ones_like(u)], -1)
    normal = torch.tensor([0.2, 0.1, 1.0], dtype=torch.float64, device="cuda")
    poses, depth = [], []
    for k in range(n):
        a = -0.02 * k
        P = np.eye(4)
        P[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        P[:3, 3] = [0.06 * k, 0.01 * k, 0.03 * k]
        Pd = torch.from_numpy(P).cuda()
        d = dirs @ Pd[:3, :3].T
        o = Pd[:3, 3]
        s_plane = (2.0 - normal @ o) / (d @ normal)
        s_rect = (1.0 - o[2]) / d[..., 2]
        hit = o + s_rect[..., None] * d
        on = (hit[..., 0].abs() < 0.3) & (hit[..., 1].abs() < 0.25) & (s_rect > 0) & (s_rect < s_plane)
        poses.append(P)
        depth.append(torch.where(on, s_rect, s_plane).float())
    return np.stack(poses), torch.stack(depth)


def torch_pipeline(depth, c2w, pairs, near=1e-3, alpha=0.01, beta=0.5):
    """The float64 restatement on the device: every unordered pair once, both flows through world coordinates, the rule through
    grid_sample; returns what pair_cues returns (flow fp32, occ uint8) for the same pairs."""
    fx, fy, cx, cy = K4
    P = torch.from_numpy(c2w).cuda()
    inv = torch.linalg.inv(P)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"), torch.arange(W, dtype=torch.float64, device="cuda"),
                          indexing="ij")
    uv = torch.stack([u, v], -1)

    def flow(i, j):
        raw = depth[i]
        ok = torch.isfinite(raw) & (raw > 0)
        d = torch.where(ok, raw, torch.ones_like(raw)).double()
        cam = torch.stack([(u - cx) / fx * d, (v - cy) / fy * d, d, torch.ones_like(d)], -1)
        tgt = (cam @ P[i].T) @ inv[j].T
        ok = ok & (tgt[..., 2] > near)
        z = torch.where(ok, tgt[..., 2], torch.ones_like(d))
        fl = torch.stack([fx * tgt[..., 0] / z + cx, fy * tgt[..., 1] / z + cy], -1) - uv
        return torch.where(ok[..., None], fl, torch.zeros_like(fl)).float(), ok

    def warp(field, fl):
        x = uv + fl
        grid = torch.stack([2.0 * x[..., 0] / (W - 1) - 1.0, 2.0 * x[..., 1] / (H - 1) - 1.0], -1)[None]
        return F.grid_sample(field[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]

    def occ(a, b, av, bv, thr):
        a64 = a.double()
        wb = warp(b.double().permute(2, 0, 1), a64).permute(1, 2, 0)
        w_inv = warp((~bv).double()[None], a64)[0]
        return ((a64 + wb).norm(dim=-1) > thr) | (w_inv > 1e-3) | ~av

    done, flows, occs = {}, [], []
    for i, j in pairs:
        key = (min(i, j), max(i, j))
        if key not in done:
            (fa, va), (fb, vb) = flow(*key), flow(key[1], key[0])
            thr = alpha * (fa.double().norm(dim=-1) + fb.double().norm(dim=-1)) + beta
            done[key] = ((fa, occ(fa, fb, va, vb, thr)), (fb, occ(fb, fa, vb, va, thr)))
        f, o = done[key][0 if i < j else 1]
        flows.append(f)
        occs.append(o)
    return torch.stack(flows), torch.stack(occs).to(torch.uint8)


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    REPS = args.reps

    def timed(fn, calls=CALLS):
        return dict(zip(("median_ms", "min_ms", "max_ms"), median_min_max(time_events(fn, REPS, calls))))

    pairs = [(i // 10, j // 10) for i, j in fc.pair_list(2000)[:32]]
    n = max(max(p) for p in pairs) + 1
    c2w, depth = scene(n)
    E, U, px = len(pairs), len({(min(p), max(p)) for p in pairs}), H * W
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "calls per rep": CALLS, "image": [H, W], "directed pairs": E,
           "unordered pairs": U, "frames": n}

    flow, occ = fc.pair_cues(depth, c2w, K4, pairs)
    ref_flow, ref_occ = torch_pipeline(depth, c2w, pairs)
    out["max |flow - float64 torch restatement rounded to fp32|"] = float((flow - ref_flow).abs().max())
    out["occlusion pixels differing from the restatement"] = int((occ != ref_occ).sum())
    out["occluded share"] = float(occ.float().mean())

    out["pair_cues"] = timed(lambda: fc.pair_cues(depth, c2w, K4, pairs))
    out["torch float64 restatement"] = timed(lambda: torch_pipeline(depth, c2w, pairs), calls=2)

    # the streaming rate of this device in this run: a 1 GiB device-to-device copy, read + written bytes over its time
    a, b = torch.zeros(1 << 28, device="cuda"), torch.zeros(1 << 28, device="cuda")
    t = timed(lambda: b.copy_(a))
    copy_bw = 2 * a.numel() * 4 / (t["median_ms"] * 1e-3)
    out["device-to-device copy of 1 GiB"] = dict(t, bytes_per_s=copy_bw)
    del a, b

    # the two kernels alone: the C entry points on buffers that are already on the device
    und = list(dict.fromkeys((min(p), max(p)) for p in pairs))
    lo, hi = [p[0] for p in und], [p[1] for p in und]
    src, dst = np.array(lo + hi), np.array(hi + lo)
    K_d = torch.tensor([K4], dtype=torch.float64, device="cuda")
    rel_d = torch.from_numpy(fc.relative_poses(c2w, src, dst)).cuda()
    src_d, dst_d = torch.from_numpy(src.astype(np.int32)).cuda(), torch.from_numpy(dst.astype(np.int32)).cuda()
    fl = torch.empty(2 * U, H, W, 2, device="cuda")
    ok = torch.empty(2 * U, H, W, dtype=torch.uint8, device="cuda")
    oc = torch.empty(2 * U, H, W, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    induced = lambda: check(lib.nsa_flowcue_induced(depth.data_ptr(), n, H, W, K_d.data_ptr(), 0, rel_d.data_ptr(), src_d.data_ptr(),
                                                    dst_d.data_ptr(), 2 * U, 1e-3, fl.data_ptr(), ok.data_ptr(), st))
    cons = lambda: check(lib.nsa_flowcue_consistency(fl[:U].data_ptr(), fl[U:].data_ptr(), ok[:U].data_ptr(), ok[U:].data_ptr(), U, H, W,
                                                     0.01, 0.5, oc[:U].data_ptr(), oc[U:].data_ptr(), st))
    t = timed(induced)
    t["bytes"] = 2 * U * px * 13                    # 4 B of depth in, 8 B of flow and 1 B of validity out, per pixel and edge
    t["bytes_per_s"] = t["bytes"] / (t["median_ms"] * 1e-3)
    t["share of the copy's rate"] = t["bytes_per_s"] / copy_bw
    out["kernel nsa_flowcue_induced, 2 x unordered pairs edges"] = t
    t = timed(cons)
    t["bytes"] = U * px * (16 + 2 + 2)              # both flows at the pixel, both validity bytes, both masks; the taps hit L2
    t["bytes_per_s"] = t["bytes"] / (t["median_ms"] * 1e-3)
    t["share of the copy's rate"] = t["bytes_per_s"] / copy_bw
    out["kernel nsa_flowcue_consistency, unordered pairs"] = t

    write_results(out, path=args.out)


if __name__ == "__main__":
    main()
