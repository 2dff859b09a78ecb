"""Time mesh decimation on the meshes of tools/bench_mesh_simplify.py -- the 512^3 mesh of tools/bench_mesh.py's model and
a mesh fused from tools/bench_tsdf.py's room -- at target_faces = F / 10 and F / 100.  Device events, warm-up first, medians of the
whole call; the rounds it took, the collapses per round and the wall time of every round of one run (read back included); the three
native calls of the first round (edge table, rings, round) timed on their own; and beside them mesh_simplify.simplify at the same
target: its time, and for both results the mean and the largest distance between the result and the input surface in both directions
through TriIndex.query (the vertices of one mesh against the surface of the other).  There is no earlier version and no reference
program, so nothing is compared in time but the two routes.  Results go to profiles/mesh_decimate_bench.json.
usage: python tools/bench_mesh_decimate.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import sys
import time

import numpy as np
import torch

from benchlib import event_window, median, median_ms, mesh_positionals, model_mesh, tsdf_mesh, write_results
from nicer_slam_amd import mesh_decimate as M, mesh_simplify
from nicer_slam_amd._native import lib, check
from nicer_slam_amd.mesh_eval import TriIndex

MAX_ROUNDS = 2000


def parse_args(argv):
    return mesh_positionals(argv)


def distances(result, mesh):
    """mean and max distance: the input's vertices to the result's surface, and the result's vertices to the input's surface"""
    fwd = TriIndex(result["verts"], result["faces"]).query(mesh["verts"])[0]
    back = TriIndex(mesh["verts"], mesh["faces"]).query(result["verts"])[0]
    return {"input -> result mean": float(fwd.mean()), "input -> result max": float(fwd.max()),
            "result -> input mean": float(back.mean()), "result -> input max": float(back.max()),
            "two-sided mean": 0.5 * (float(fwd.mean()) + float(back.mean())), "two-sided max": max(float(fwd.max()), float(back.max()))}


def first_round(v, f, reps):
    """ms of the three native calls of the first round on the whole mesh, each on its own (the state is made afresh every time)"""
    dev, V, F = v.device, v.shape[0], f.shape[0]
    s = torch.cuda.current_stream(dev).cuda_stream
    tb = M._Tables(V, F, dev)
    state = torch.empty(lib.nsa_mesh_decimate_state_bytes(V), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.nsa_mesh_decimate_workspace(V, F), dtype=torch.uint8, device=dev)
    log = torch.zeros(V, 4, dtype=torch.int64, device=dev)
    totals = torch.zeros(14, dtype=torch.int64, device=dev)
    fw = f.clone()

    def edges():
        check(lib.nsa_mesh_edges(fw.data_ptr(), F, V, None, tb.ws_edges.data_ptr(), tb.edges.data_ptr(), tb.edge_count.data_ptr(),
                                 tb.edge_forward.data_ptr(), tb.edge_start.data_ptr(), tb.edge_halfedges.data_ptr(),
                                 tb.face_edges.data_ptr(), tb.totals.data_ptr(), s))

    def rings():
        check(lib.nsa_mesh_ring(tb.edges.data_ptr(), tb.totals.data_ptr(), V, F, tb.ws_ring.data_ptr(), tb.ring_start.data_ptr(),
                                tb.ring.data_ptr(), tb.ring_edge.data_ptr(), s))

    def init():
        fw.copy_(f)
        tb.build(fw)
        check(lib.nsa_mesh_decimate_init(v.data_ptr(), None, V, fw.data_ptr(), F, tb.edge_count.data_ptr(), tb.edge_start.data_ptr(),
                                         tb.edge_halfedges.data_ptr(), tb.ring_start.data_ptr(), tb.ring.data_ptr(),
                                         tb.ring_edge.data_ptr(), None, 0, 1.0, ws.data_ptr(), state.data_ptr(), s))

    def round_():
        check(lib.nsa_mesh_decimate_round(V, fw.data_ptr(), F, tb.edges.data_ptr(), tb.edge_count.data_ptr(), tb.edge_start.data_ptr(),
                                          tb.edge_halfedges.data_ptr(), tb.totals.data_ptr(), tb.ring_start.data_ptr(), tb.ring.data_ptr(),
                                          tb.ring_edge.data_ptr(), 0, 1, F // 10, 0, 0.0, 0.04, 1e-3, 0, ws.data_ptr(), state.data_ptr(),
                                          log.data_ptr(), V, totals.data_ptr(), s))

    out = {"nsa_mesh_edges ms": median_ms(edges, reps), "nsa_mesh_ring ms": median_ms(rings, reps),
           "init ms (tables included)": median_ms(init, reps)}
    ms = []
    for _ in range(reps + 1):                                     # a round changes the state: a fresh one each time, outside the events
        init()
        torch.cuda.synchronize()
        ms.append(event_window(round_))
    out["nsa_mesh_decimate_round ms"] = median(ms[1:])
    return out


def case(name, mesh, out, reps):
    mesh = {k: mesh[k].contiguous() for k in ("verts", "faces")}
    v, f = mesh["verts"], mesh["faces"]
    r = {"V": v.shape[0], "F": f.shape[0], "first round": first_round(v, f.to(torch.int32), reps)}
    for div in (10, 100):
        target = f.shape[0] // div
        c = {"target": target}
        walls, takes = [], []
        mark = [time.perf_counter()]

        def on_round(t):
            now = time.perf_counter()
            walls.append(1e3 * (now - mark[0]))
            takes.append(t[9])
            mark[0] = now

        args = (v, f.to(torch.int32), None, None, target, None, "quadric", 1.0, 0.2, 1e-3, MAX_ROUNDS)
        M._decimate(*args)
        torch.cuda.synchronize()
        mark[0] = time.perf_counter()
        res = M._decimate(*args, on_round=on_round)
        c.update(rounds=res[5]["rounds"], collapses=res[5]["collapses"],
                 collapses_per_round={"first": takes[0], "median": float(np.median(takes)), "last": takes[-1], "max": max(takes)},
                 round_wall_ms={"first": walls[0], "median": float(np.median(walls)), "last": walls[-1], "sum": float(np.sum(walls))})
        c["decimate() ms"] = median_ms(lambda: M.decimate(mesh, target_faces=target, max_rounds=MAX_ROUNDS, normals=None), reps)
        dec = M.decimate(mesh, target_faces=target, max_rounds=MAX_ROUNDS, normals=None)
        c["decimate faces"] = int(dec["faces"].shape[0])
        c["decimate distances"] = distances(dec, mesh)
        c["simplify(target_faces=) ms"] = median_ms(lambda: mesh_simplify.simplify(mesh, target_faces=target), 3)
        sim = mesh_simplify.simplify(mesh, target_faces=target)
        c["simplify faces"] = int(sim["faces"].shape[0])
        c["simplify distances"] = distances(sim, mesh)
        r[f"F / {div}"] = c
    out[name] = r


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    case(f"model mesh {a.resolution}^3", model_mesh(a.resolution), out, a.reps)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", tsdf_mesh(a.voxels, a.frames), out, a.reps)
    write_results(out, "mesh_decimate_bench.json")


if __name__ == "__main__":
    main()
