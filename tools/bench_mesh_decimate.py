"""Time mesh decimation on the meshes of tools/bench_mesh_simplify.py -- the 512^3 mesh of tools/bench_mesh.py's model and
a mesh fused from tools/bench_tsdf.py's room -- at target_faces = F / 10 and F / 100.  Device events, warm-up first, medians of the
whole call; the rounds it took, the collapses per round and the wall time of every round of one run (read back included); the three
native calls of the first round (edge table, rings, round) timed on their own; and beside them mesh_simplify.simplify at the same
target: its time, and for both results the mean and the largest distance between the result and the input surface in both directions
through TriIndex.query (the vertices of one mesh against the surface of the other).  There is no earlier version and no reference
program, so nothing is compared in time but the two routes.  Results go to profiles/mesh_decimate_bench.json.
usage: python tools/bench_mesh_decimate.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from nicer_slam_amd import inference, mesh_decimate as M, mesh_simplify
from nicer_slam_amd._native import lib, check
from nicer_slam_amd.mesh_eval import TriIndex

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
RES = int(sys.argv[2]) if len(sys.argv) > 2 else 512
TSDF_N = int(sys.argv[3]) if len(sys.argv) > 3 else 256
TSDF_FRAMES = int(sys.argv[4]) if len(sys.argv) > 4 else 100
MAX_ROUNDS = 2000


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


def distances(result, mesh):
    """mean and max distance: the input's vertices to the result's surface, and the result's vertices to the input's surface"""
    fwd = TriIndex(result["verts"], result["faces"]).query(mesh["verts"])[0]
    back = TriIndex(mesh["verts"], mesh["faces"]).query(result["verts"])[0]
    return {"input -> result mean": float(fwd.mean()), "input -> result max": float(fwd.max()),
            "result -> input mean": float(back.mean()), "result -> input max": float(back.max()),
            "two-sided mean": 0.5 * (float(fwd.mean()) + float(back.mean())), "two-sided max": max(float(fwd.max()), float(back.max()))}


def first_round(v, f):
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

    out = {"nsa_mesh_edges ms": timed(edges), "nsa_mesh_ring ms": timed(rings), "init ms (tables included)": timed(init)}
    ms = []
    for _ in range(REPS + 1):                                     # a round changes the state: a fresh one each time, outside the events
        init()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        round_()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    out["nsa_mesh_decimate_round ms"] = float(np.median(ms[1:]))
    return out


def case(name, mesh, out):
    mesh = {k: mesh[k].contiguous() for k in ("verts", "faces")}
    v, f = mesh["verts"], mesh["faces"]
    r = {"V": v.shape[0], "F": f.shape[0], "first round": first_round(v, f.to(torch.int32))}
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
        c["decimate() ms"] = timed(lambda: M.decimate(mesh, target_faces=target, max_rounds=MAX_ROUNDS, normals=None))
        dec = M.decimate(mesh, target_faces=target, max_rounds=MAX_ROUNDS, normals=None)
        c["decimate faces"] = int(dec["faces"].shape[0])
        c["decimate distances"] = distances(dec, mesh)
        c["simplify(target_faces=) ms"] = timed(lambda: mesh_simplify.simplify(mesh, target_faces=target), reps=3)
        sim = mesh_simplify.simplify(mesh, target_faces=target)
        c["simplify faces"] = int(sim["faces"].shape[0])
        c["simplify distances"] = distances(sim, mesh)
        r[f"F / {div}"] = c
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
    with open(os.path.join(ROOT, "profiles", "mesh_decimate_bench.json"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
