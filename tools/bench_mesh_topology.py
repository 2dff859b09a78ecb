"""Time the mesh topology path: the edge table, the face components and the whole report on the 512^3 mesh of
tools/bench_mesh.py's model and on a mesh fused from tools/bench_tsdf.py's room.  Device events, warm-up first, medians; the two entry
points are timed without the wrappers' read-back of the totals as well.  The host route -- device -> host copy of the faces,
np.unique of the int64 edge keys, scipy.sparse.csgraph.connected_components over the faces -- is timed as the only runnable baseline;
there is no earlier version of this capability to compare with.  Results go to profiles/mesh_topology_bench.json.
usage: python tools/bench_mesh_topology.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from nicer_slam_amd import inference, mesh_topology as M
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


def host_route(f, V):
    """(E, boundary edges, components) the way a host program gets them"""
    g = f.cpu().numpy().astype(np.int64)
    a = g.reshape(-1)
    b = g[:, [1, 2, 0]].reshape(-1)
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    _, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    later = np.ones(len(order), bool)
    later[np.cumsum(count) - count] = False
    pos = np.nonzero(later)[0]
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    F = len(g)
    n, _ = connected_components(sp.coo_matrix((np.ones(len(pos), np.int8), (order[pos] // 3, order[pos - 1] // 3)), shape=(F, F)),
                                directed=False)
    return len(count), int((count == 1).sum()), n


def case(name, mesh, out):
    f = mesh["faces"].contiguous()
    V, F = mesh["verts"].shape[0], f.shape[0]
    H = 3 * F
    r = {"V": V, "F": F}
    rep = M.topology(mesh)
    r["report"] = rep
    dev = f.device
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    t = dict(edges=i32(H, 2), count=i32(H), fwd=i32(H), start=i32(H + 1), he=i32(H), fe=i32(F, 3))
    ws = torch.empty(lib.nsa_mesh_edges_workspace(V, F), dtype=torch.uint8, device=dev)
    totals = torch.empty(8, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    r["edge table kernels ms"] = timed(lambda: check(lib.nsa_mesh_edges(
        f.data_ptr(), F, V, None, ws.data_ptr(), t["edges"].data_ptr(), t["count"].data_ptr(), t["fwd"].data_ptr(),
        t["start"].data_ptr(), t["he"].data_ptr(), t["fe"].data_ptr(), totals.data_ptr(), stream)))
    bits = max(1, int(V).bit_length())
    passes = (bits + 7) // 8
    # per radix pass and key: the histogram reads the key (4 B), the scatter reads key + payload and writes both (16 B); in each of
    # the two stages the first pass reads no payload and the last writes no key
    r["radix passes"] = 2 * passes
    r["radix MB moved at least"] = 2 * (passes * (4 + 8 + 8) - 8) * H / 1e6
    r["edge table MB moved at least"] = r["radix MB moved at least"] + (12 * F + 2 * 16 * H + 5 * 4 * H) / 1e6
    ws2 = torch.empty(lib.nsa_mesh_face_components_workspace(F), dtype=torch.uint8, device=dev)
    label = i32(F)
    tot2 = torch.empty(2, dtype=torch.int64, device=dev)
    r["face components kernels ms"] = timed(lambda: check(lib.nsa_mesh_face_components(
        t["fe"].data_ptr(), t["start"].data_ptr(), t["he"].data_ptr(), F, ws2.data_ptr(), label.data_ptr(), tot2.data_ptr(), stream)))
    r["edge_table() ms"] = timed(lambda: M.edge_table(f, V))
    r["face_components() ms"] = timed(lambda: M.face_components(f, V))
    r["topology() ms"] = timed(lambda: M.topology(mesh))
    r["topology(weld=True) ms"] = timed(lambda: M.topology(mesh, weld=True))
    try:
        host_route(f, V)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            E, B, n = host_route(f, V)
            ts.append((time.perf_counter() - t0) * 1e3)
        assert (E, B) == (rep["n_edges"], rep["n_boundary"]), (E, B, rep)
        if rep["n_contributing"] == F:                            # (the host route takes every face as it is)
            assert n == rep["n_components"], (n, rep)
        r["host copy + np.unique + scipy connected_components ms"] = float(np.median(ts))
    except ImportError:
        r["host copy + np.unique + scipy connected_components ms"] = None
    out[name] = r


def main():
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS}
    from bench_mesh import model
    case(f"model mesh {RES}^3", inference.extract_mesh(model(), RES, (-1.0, 1.0), color=False), out)
    import bench_mesh_clean                                       # (reads the same command line)
    case(f"tsdf room {TSDF_N}^3, {TSDF_FRAMES} frames", bench_mesh_clean.tsdf_mesh(), out)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_topology_bench.json"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
