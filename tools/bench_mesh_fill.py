"""Time hole filling on the meshes of tools/bench_mesh_topology.py -- the 512^3 mesh of tools/bench_mesh.py's model and a
mesh fused from tools/bench_tsdf.py's room, which its volume's box cuts open -- and on the model mesh with every 97th face masked out:
thousands of small loops, some of them pinched.  Device events, warm-up first, medians of the whole call (its two read backs
included) and of the three native calls on their own (edge table, loops, emit); where the star test holds loops
back, the same call with skip_folded=False beside it.  There is no earlier version and no runnable
reference program, so no time is gated; the table stands beside the host route, tests/fill_ref.py in numpy on the same machine (wall
clock, one run).  The device result is compared with the host's bit for bit while at it.  Results go to profiles/mesh_fill_bench.json.
usage: python tools/bench_mesh_fill.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from nicer_slam_amd import inference, mesh_fill as M, mesh_topology
from nicer_slam_amd._native import lib, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
RES = int(sys.argv[2]) if len(sys.argv) > 2 else 512
TSDF_N = int(sys.argv[3]) if len(sys.argv) > 3 else 256
TSDF_FRAMES = int(sys.argv[4]) if len(sys.argv) > 4 else 100
KW = dict(skip_folded=True)


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


def native_calls(v, f):
    """ms of the three native calls on the whole mesh, each on its own"""
    dev, V, F = v.device, v.shape[0], f.shape[0]
    s = torch.cuda.current_stream(dev).cuda_stream
    t, et = mesh_topology._edge_table(f, V, F, None)
    B = et["n_boundary"]
    out = {"nsa_mesh_edges ms (totals read back)": timed(lambda: mesh_topology._edge_table(f, V, F, None))}
    if B == 0:
        return out
    r = M._loops(v, f, None, None, None, V, F, None, None, 0, 64, True)
    ws = torch.empty(lib.nsa_mesh_fill_workspace(F, B), dtype=torch.uint8, device=dev)
    tot = torch.zeros(len(M.TOTALS), dtype=torch.int64, device=dev)
    ints, reals = torch.zeros(B, 9, dtype=torch.int64, device=dev), torch.zeros(B, 18, dtype=torch.float64, device=dev)
    item = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(5)]
    flags = torch.empty(B, dtype=torch.uint8, device=dev)

    def loops():
        check(lib.nsa_mesh_fill_loops(v.data_ptr(), None, V, f.data_ptr(), None, F, t["edge_count"].data_ptr(), t["edge_forward"].data_ptr(),
                                      t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(), t["face_edges"].data_ptr(),
                                      t["_totals"].data_ptr(), B, 0, 0, 0, 0.0, 0, 64, 1, ws.data_ptr(), item[0].data_ptr(),
                                      item[1].data_ptr(), flags.data_ptr(), item[2].data_ptr(), item[3].data_ptr(), item[4].data_ptr(),
                                      ints.data_ptr(), reals.data_ptr(), tot.data_ptr(), s))

    out["nsa_mesh_fill_loops ms"] = timed(loops)
    out["nsa_mesh_fill_emit ms"] = timed(lambda: M._emit(v, f, None, V, F, r))
    return out


def case(name, mesh, out):
    import fill_ref
    v, f = mesh["verts"].float().contiguous(), mesh["faces"].to(torch.int32).contiguous()
    mesh = {"verts": v, "faces": f}
    got, rep = M.fill_holes(mesh, return_report=True, **KW)
    r = {"V": v.shape[0], "F": f.shape[0], "totals": rep["totals"],
         "loop edges": {"max": max(rep["n"], default=0), "median": float(np.median(rep["n"])) if rep["n"] else 0.0},
         "rounds of each kind": fill_ref.n_rounds(rep["totals"]["n_boundary"]),
         "fill_holes() ms": timed(lambda: M.fill_holes(mesh, **KW)), "native calls": native_calls(v, f)}
    after = mesh_topology.topology(got)
    r["after"] = {k: after[k] for k in ("n_boundary", "n_boundary_loops", "is_watertight", "is_oriented")}
    if rep["totals"]["n_folded"]:                                 # what the star test holds back: the same call without it
        kept, rep2 = M.fill_holes(mesh, return_report=True, skip_folded=False)
        after = mesh_topology.topology(kept)
        r["skip_folded=False"] = {"totals": rep2["totals"], "rings": rep2["rings"],
                                  "fill_holes() ms": timed(lambda: M.fill_holes(mesh, skip_folded=False)),
                                  "after": {k: after[k] for k in ("n_boundary", "n_boundary_loops", "is_watertight", "is_oriented")}}
    host = {"verts": v.cpu().numpy(), "faces": f.cpu().numpy()}
    t0 = time.perf_counter()
    ref = fill_ref.fill_holes(host, **KW)
    r["host route (numpy) ms"] = 1e3 * (time.perf_counter() - t0)
    r["equals the host route bit for bit"] = bool(ref["totals"] == rep["totals"] and
                                                  got["verts"].cpu().numpy().tobytes() == ref["verts"].tobytes() and
                                                  np.array_equal(got["faces"].cpu().numpy(), ref["faces"]))
    out[name] = r


def main():
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS}
    from bench_mesh import model
    full = inference.extract_mesh(model(), RES, (-1.0, 1.0), color=False)
    case(f"model mesh {RES}^3", full, out)
    import bench_mesh_clean                                       # (reads the same command line)
    case(f"tsdf room {TSDF_N}^3, {TSDF_FRAMES} frames", bench_mesh_clean.tsdf_mesh(), out)
    keep = torch.arange(full["faces"].shape[0], device=full["faces"].device) % 97 != 96
    case(f"model mesh {RES}^3 without every 97th face", {"verts": full["verts"], "faces": full["faces"][keep]}, out)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_fill_bench.json"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
