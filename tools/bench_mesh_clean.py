"""Time the mesh clean-up path: component labelling, statistics, compaction and keep_components end to end on the
512^3 mesh of tools/bench_mesh.py's model, on the same mesh with its vertex names randomly permuted (no index locality) and on a
mesh fused from tools/bench_tsdf.py's room.  Device events, warm-up first, medians; per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  The labelling entry point is also timed without the wrapper's read-back
of the totals.  When scipy is importable, the host route (device -> host copy of the faces + scipy.sparse.csgraph
.connected_components) is timed as the only runnable baseline; there is no earlier version of this capability to compare with.
usage: python tools/bench_mesh_clean.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import sys

import numpy as np
import torch

from benchlib import median, median_ms, time_host, mesh_positionals, model_mesh, tsdf_mesh, write_results
from nicer_slam_amd import mesh_clean as M
from nicer_slam_amd._native import lib, check


def parse_args(argv):
    return mesh_positionals(argv)


def case(name, mesh, out, reps):
    timed = lambda fn: median_ms(fn, reps)
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
        n, _ = host()
        assert n - int((vl < 0).sum()) == r["components"], (n, r["components"])
        r["host copy + scipy connected_components ms"] = median(time_host(host, 3, warmup=False))
    except ImportError:
        r["host copy + scipy connected_components ms"] = None
    out[name] = r


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    mesh = model_mesh(a.resolution)
    case(f"model mesh {a.resolution}^3", mesh, out, a.reps)
    V = mesh["verts"].shape[0]
    perm = torch.randperm(V, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(V, device="cuda")
    shuffled = {"verts": mesh["verts"][inv], "normals": mesh["normals"][inv], "faces": perm[mesh["faces"].long()].int()}
    case(f"model mesh {a.resolution}^3, vertex names permuted", shuffled, out, a.reps)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", tsdf_mesh(a.voxels, a.frames), out, a.reps)
    write_results(out)


if __name__ == "__main__":
    main()
