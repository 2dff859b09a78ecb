"""Time the mesh topology path: the edge table, the face components and the whole report on the 512^3 mesh of
tools/bench_mesh.py's model and on a mesh fused from tools/bench_tsdf.py's room.  Device events, warm-up first, medians; the two entry
points are timed without the wrappers' read-back of the totals as well.  The host route -- device -> host copy of the faces,
np.unique of the int64 edge keys, scipy.sparse.csgraph.connected_components over the faces -- is timed as the only runnable baseline;
there is no earlier version of this capability to compare with.  Results go to profiles/mesh_topology_bench.json.
usage: python tools/bench_mesh_topology.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import sys

import numpy as np
import torch

from benchlib import median, median_ms, mesh_positionals, model_mesh, time_host, tsdf_mesh, write_results
from nicer_slam_amd import mesh_topology as M
from nicer_slam_amd._native import lib, check


def parse_args(argv):
    return mesh_positionals(argv)


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


def case(name, mesh, out, reps):
    timed = lambda fn: median_ms(fn, reps)
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
        E, B, n = host_route(f, V)
        assert (E, B) == (rep["n_edges"], rep["n_boundary"]), (E, B, rep)
        if rep["n_contributing"] == F:                            # (the host route takes every face as it is)
            assert n == rep["n_components"], (n, rep)
        r["host copy + np.unique + scipy connected_components ms"] = median(time_host(lambda: host_route(f, V), 3, warmup=False))
    except ImportError:
        r["host copy + np.unique + scipy connected_components ms"] = None
    out[name] = r


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    case(f"model mesh {a.resolution}^3", model_mesh(a.resolution), out, a.reps)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", tsdf_mesh(a.voxels, a.frames), out, a.reps)
    write_results(out, "mesh_topology_bench.json")


if __name__ == "__main__":
    main()
