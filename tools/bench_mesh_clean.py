"""Time the mesh clean-up path: component labelling, statistics, compaction and keep_components end to end on the
512^3 mesh of tools/bench_mesh.py's model, on the same mesh with its vertex names randomly permuted (no index locality) and on a
mesh fused from tools/bench_tsdf.py's room.  Device events, warm-up first, medians; per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  The labelling entry point is also timed without the wrapper's read-back
of the totals.  When scipy is importable, the host route (device -> host copy of the faces + scipy.sparse.csgraph
.connected_components) is timed as the only runnable baseline; there is no earlier version of this capability to compare with.
usage: python tools/bench_mesh_clean.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from nicer_slam_amd import inference, mesh_clean as M
from nicer_slam_amd._native import lib, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
RES = int(sys.argv[2]) if len(sys.argv) > 2 else 512
TSDF_N = int(sys.argv[3]) if len(sys.argv) > 3 else 256
TSDF_FRAMES = int(sys.argv[4]) if len(sys.argv) > 4 else 100


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


def tsdf_mesh():
    import synthetic_sequence as ss
    from bench_tsdf import ROOM_HALF, ring
    from nicer_slam_amd.tsdf import TSDFVolume
    H, W, vl = 480, 640, 1.44 / TSDF_N
    poses = ring(TSDF_FRAMES)
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 400.0
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl)
    for lo in range(0, TSDF_FRAMES, 50):
        c, d, _ = ss.render_analytic_room(torch.from_numpy(poses[lo:lo + 50]), K, H, W, "cuda", ROOM_HALF)
        vol.integrate(d.reshape(-1, H, W), c, poses[lo:lo + 50], K, batch=32)
    return vol.extract_mesh()


def case(name, mesh, out):
    v, f = mesh["verts"].contiguous(), mesh["faces"].contiguous()
    V, F = v.shape[0], f.shape[0]
    r = {"V": V, "F": F}
    st = M.component_stats(v, f)
    r["components"] = st["n_components"]
    r["largest share of area"] = float(st["area"].max() / st["area"].sum())
    ws = torch.empty(lib.nsa_mesh_components_workspace(V), dtype=torch.uint8, device="cuda")
    vl = torch.empty(V, dtype=torch.int32, device="cuda")
    fl = torch.empty(F, dtype=torch.int32, device="cuda")
    totals = torch.empty(3, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    r["labelling kernels ms"] = timed(lambda: check(lib.nsa_mesh_components(f.data_ptr(), F, V, ws.data_ptr(), vl.data_ptr(),
                                                                           fl.data_ptr(), totals.data_ptr(), stream)))
    r["labelling MB moved at least"] = (12 * F + 4 * F + 3 * 4 * V) / 1e6      # faces once, face_label, parent + vertex_label r/w
    r["components() ms"] = timed(lambda: M.components(f, V))
    r["component_stats() ms"] = timed(lambda: M.component_stats(v, f))
    mask = (st["face_comp"] == int(st["area"].argmax()))
    r["select_faces() ms"] = timed(lambda: M.select_faces(mesh, mask))
    r["keep_components(largest) ms"] = timed(lambda: M.keep_components(mesh, "largest"))
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components

        def host():
            g = f.cpu().numpy().astype(np.int64)
            rows, cols = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
            return connected_components(sp.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)), directed=False)
        host()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            n, _ = host()
            t.append((time.perf_counter() - t0) * 1e3)
        assert n - int((vl < 0).sum()) == r["components"], (n, r["components"])
        r["host copy + scipy connected_components ms"] = float(np.median(t))
    except ImportError:
        r["host copy + scipy connected_components ms"] = None
    out[name] = r


def main():
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS}
    from bench_mesh import model
    mesh = inference.extract_mesh(model(), RES, (-1.0, 1.0), color=False)
    case(f"model mesh {RES}^3", mesh, out)
    V = mesh["verts"].shape[0]
    perm = torch.randperm(V, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(V, device="cuda")
    shuffled = {"verts": mesh["verts"][inv], "normals": mesh["normals"][inv], "faces": perm[mesh["faces"].long()].int()}
    case(f"model mesh {RES}^3, vertex names permuted", shuffled, out)
    case(f"tsdf room {TSDF_N}^3, {TSDF_FRAMES} frames", tsdf_mesh(), out)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
