"""Time the fan split on a mesh fused from tools/bench_tsdf.py's room, on that mesh clustered, and on that mesh folded
onto itself by index (vertex v renamed v mod V / 2: two sheets on every vertex, so that the split has work to do):
``split_nonmanifold`` and ``vertex_fans`` with their read-backs, the kernels of nsa_mesh_split_fans alone on a prepared edge table,
and ``mesh_topology.topology`` on the same mesh as the yardstick -- both are dominated by the same radix sort of 3 F keys (topology
sorts twice, the split once more on top of the edge table it needs).  Device events, warm-up first, medians.  Results go to
profiles/mesh_repair_bench.json.
usage: python tools/bench_mesh_repair.py [reps=5] [resolution (unused)] [tsdf voxels=256] [tsdf frames=100]
(the second positional is accepted and ignored: the command line is the other mesh benches', and this one has no model mesh)"""
import sys

import torch

from benchlib import median_ms, mesh_positionals, tsdf_mesh, write_results
from nicer_slam_amd import mesh_repair as R, mesh_simplify, mesh_topology as M
from nicer_slam_amd._native import lib, check


def parse_args(argv):
    return mesh_positionals(argv)


def case(name, mesh, out, reps):
    timed = lambda fn: median_ms(fn, reps)
    f = mesh["faces"].contiguous()
    V, F = mesh["verts"].shape[0], f.shape[0]
    H = 3 * F
    r = {"V": V, "F": F}
    split, report = R.split_nonmanifold(mesh, return_report=True)
    r["report"] = report
    r["n_nonmanifold before"] = M.topology(mesh)["n_nonmanifold"]
    r["n_nonmanifold after"] = M.topology(split)["n_nonmanifold"]
    t, _ = M._edge_table(f, V, F, None)
    dev = f.device
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    corner_fan, vertex_fans, faces_out, new_source = i32(H), i32(V), i32(F, 3), i32(H)
    ws = torch.empty(lib.nsa_mesh_split_fans_workspace(V, F), dtype=torch.uint8, device=dev)
    totals = torch.empty(8, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    r["split_fans kernels ms"] = timed(lambda: check(lib.nsa_mesh_split_fans(
        f.data_ptr(), F, V, None, 0, t["edges"].data_ptr(), t["edge_count"].data_ptr(), t["edge_forward"].data_ptr(),
        t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(), t["face_edges"].data_ptr(), t["_totals"].data_ptr(), ws.data_ptr(),
        corner_fan.data_ptr(), vertex_fans.data_ptr(), faces_out.data_ptr(), new_source.data_ptr(), totals.data_ptr(), stream)))
    r["radix passes"] = (max(1, int(V).bit_length()) + 7) // 8
    r["edge_table() ms"] = timed(lambda: M.edge_table(f, V))
    r["vertex_fans() ms"] = timed(lambda: R.vertex_fans(mesh))
    r["split_nonmanifold() ms"] = timed(lambda: R.split_nonmanifold(mesh))
    r["topology() ms"] = timed(lambda: M.topology(mesh))
    out[name] = r


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    mesh = tsdf_mesh(a.voxels, a.frames)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", mesh, out, a.reps)
    extent = float((mesh["verts"].amax(0) - mesh["verts"].amin(0)).max())
    case("the same, clustered at extent / 96 (mean)", mesh_simplify.simplify(mesh, cell=extent / 96, placement="mean"), out, a.reps)
    half = (mesh["verts"].shape[0] + 1) // 2
    case("the same, folded by index (v mod V / 2)", dict(verts=mesh["verts"][:half].contiguous(), faces=mesh["faces"] % half), out, a.reps)
    write_results(out, "mesh_repair_bench.json")


if __name__ == "__main__":
    main()
