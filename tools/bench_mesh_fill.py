"""Time hole filling on the meshes of tools/bench_mesh_topology.py -- the 512^3 mesh of tools/bench_mesh.py's model and a
mesh fused from tools/bench_tsdf.py's room, which its volume's box cuts open -- and on the model mesh with every 97th face masked out:
thousands of small loops, some of them pinched.  Device events, warm-up first, medians of the whole call (its two read backs
included) and of the three native calls on their own (edge table, loops, emit); where the star test holds loops
back, the same call with skip_folded=False beside it.  There is no earlier version and no runnable
reference program, so no time is gated; the table stands beside the host route, tests/fill_ref.py in numpy on the same machine (wall
clock, one run).  The device result is compared with the host's bit for bit while at it.  Results go to profiles/mesh_fill_bench.json.
With --method auto | min_area the same three meshes go through the minimum-area patches: the time of the call, of the
plan and of the tables-and-emit entry point on their own, and of the numpy statement tests/fill_area_ref.py on the same machine; the
device's faces are compared with the statement's; the room's row also says whether it is closed, which sign rule sign="auto" takes
afterwards, and the patch area beside the polar patch's of skip_folded=False.  Results go to profiles/mesh_fill_area_bench.json
(profiles/mesh_fill_area_bench_min_area.json for min_area).
usage: python tools/bench_mesh_fill.py [--method polar|auto|min_area] [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import json
import sys
import time

import numpy as np
import torch

from benchlib import median_ms, mesh_positionals, model_mesh, tsdf_mesh, write_results
from nicer_slam_amd import mesh_fill as M, mesh_topology
from nicer_slam_amd._native import lib, check

KW = dict(skip_folded=True)


def parse_args(argv):
    """the four positionals of the mesh benches, and --method M anywhere among them"""
    argv, method = list(argv), "polar"
    if "--method" in argv:
        at = argv.index("--method")
        method = argv[at + 1]
        del argv[at:at + 2]
    if method not in M.METHODS:
        raise SystemExit(f"--method must be one of {M.METHODS}")
    a = mesh_positionals(argv)
    a.method = method
    return a


def native_calls(v, f, reps):
    """ms of the three native calls on the whole mesh, each on its own"""
    timed = lambda fn: median_ms(fn, reps)
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


def patch_area(mesh, first_face):
    """the area of the faces from first_face on, in float64"""
    v, f = mesh["verts"].double(), mesh["faces"][first_face:].long()
    n = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return float(0.5 * n.norm(dim=1).sum())


def area_case(name, mesh, out, reps, METHOD):
    """one mesh through method=METHOD"""
    import fill_area_ref
    timed = lambda fn: median_ms(fn, reps)
    from nicer_slam_amd import mesh_sdf
    v, f = mesh["verts"].float().contiguous(), mesh["faces"].to(torch.int32).contiguous()
    mesh = {"verts": v, "faces": f}
    V, F, dev = v.shape[0], f.shape[0], v.device
    got, rep = M.fill_holes(mesh, return_report=True, method=METHOD)
    at = rep["area_totals"]
    r = {"V": V, "F": F, "method": METHOD, "totals": rep["totals"], "area_totals": at,
         "diagonal launches": max(at["max_n"] - 2, 0),
         "loop edges": {"max": max(rep["n"], default=0), "median": float(np.median(rep["n"])) if rep["n"] else 0.0},
         "area classes of the selected loops": {c: rep["area_class"].count(c) for c in M.AREA_CLASSES},
         "patch area": float(sum(a for a, c in zip(rep["area"].cpu().tolist(), rep["area_class"]) if c == "area_filled")),
         "fill_holes(method) ms": timed(lambda: M.fill_holes(mesh, method=METHOD)),
         "fill_holes() ms, polar": timed(lambda: M.fill_holes(mesh))}
    after = mesh_topology.topology(got)
    r["after"] = {k: after[k] for k in ("n_boundary", "n_boundary_loops", "is_watertight", "is_oriented")}
    r["sign rule of sign=auto, before -> after"] = [mesh_sdf.resolve_sign(mesh, "auto"), mesh_sdf.resolve_sign(got, "auto")]
    if rep["totals"]["n_boundary"]:
        lr = M._loops(v, f, None, None, None, V, F, None, None, 0, 64, True)
        mask = 1 << 5 if METHOD == "auto" else 1 | 1 << 5
        B, s = lr["B"], torch.cuda.current_stream(dev).cuda_stream
        ints, plan = torch.zeros(B, 6, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
        r["nsa_mesh_fill_area_plan ms"] = timed(lambda: check(lib.nsa_mesh_fill_area_plan(
            lr["_ints"].data_ptr(), lr["_totals"].data_ptr(), F, B, mask, 2048, ints.data_ptr(), plan.data_ptr(), s)))
        _, tabled, _, cells, max_n, plan_faces, rows, _ = (int(x) for x in plan.cpu())
        if tabled:
            nbytes = lib.nsa_mesh_fill_area_workspace(cells, rows)
            r["workspace MB"] = nbytes / 1e6
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            area, faces = torch.zeros(B, dtype=torch.float64, device=dev), torch.full((plan_faces, 3), -1, dtype=torch.int32, device=dev)
            final, t = torch.zeros(4, dtype=torch.int64, device=dev), lr["_edge"]

            def tables():
                check(lib.nsa_mesh_fill_area_plan(lr["_ints"].data_ptr(), lr["_totals"].data_ptr(), F, B, mask, 2048, ints.data_ptr(),
                                                  plan.data_ptr(), s))                 # (the tables entry rewrites the classes)
                check(lib.nsa_mesh_fill_area_tables(v.data_ptr(), V, f.data_ptr(), None, F, t["edges"].data_ptr(), t["_totals"].data_ptr(),
                                                    lr["_order"].data_ptr(), B, lr["_ints"].data_ptr(), lr["_totals"].data_ptr(),
                                                    ints.data_ptr(), cells, rows, max_n, plan_faces, 1e-12, ws.data_ptr(), area.data_ptr(),
                                                    faces.data_ptr(), final.data_ptr(), s))

            r["nsa_mesh_fill_area_plan + nsa_mesh_fill_area_tables ms"] = timed(tables)
    if rep["totals"]["n_folded"]:                                 # the polar patch the star test would have refused, beside it
        kept, rep2 = M.fill_holes(mesh, return_report=True, skip_folded=False)
        r["skip_folded=False, polar"] = {"patch area": patch_area(kept, F), "new faces": rep2["totals"]["n_new_faces"]}
    host = {"verts": v.cpu().numpy(), "faces": f.cpu().numpy()}
    t0 = time.perf_counter()
    ref = fill_area_ref.fill_holes(host, method=METHOD)
    r["host route (numpy) ms"] = 1e3 * (time.perf_counter() - t0)
    r["equals the host route"] = bool(ref["area_totals"] == at and np.array_equal(got["faces"].cpu().numpy(), ref["faces"]) and
                                      got["verts"].cpu().numpy().tobytes() == ref["verts"].tobytes() and
                                      np.array_equal(rep["area"].cpu().numpy().view(np.uint64), ref["area"].view(np.uint64)))
    out[name] = r
    print(name, json.dumps(r), flush=True)


def case(name, mesh, out, reps, method):
    if method != "polar":
        return area_case(name, mesh, out, reps, method)
    import fill_ref
    timed = lambda fn: median_ms(fn, reps)
    v, f = mesh["verts"].float().contiguous(), mesh["faces"].to(torch.int32).contiguous()
    mesh = {"verts": v, "faces": f}
    got, rep = M.fill_holes(mesh, return_report=True, **KW)
    r = {"V": v.shape[0], "F": f.shape[0], "totals": rep["totals"],
         "loop edges": {"max": max(rep["n"], default=0), "median": float(np.median(rep["n"])) if rep["n"] else 0.0},
         "rounds of each kind": fill_ref.n_rounds(rep["totals"]["n_boundary"]),
         "fill_holes() ms": timed(lambda: M.fill_holes(mesh, **KW)), "native calls": native_calls(v, f, reps)}
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


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    full = model_mesh(a.resolution)
    case(f"model mesh {a.resolution}^3", full, out, a.reps, a.method)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", tsdf_mesh(a.voxels, a.frames), out, a.reps, a.method)
    keep = torch.arange(full["faces"].shape[0], device=full["faces"].device) % 97 != 96
    case(f"model mesh {a.resolution}^3 without every 97th face", {"verts": full["verts"], "faces": full["faces"][keep]}, out, a.reps, a.method)
    write_results(out, {"polar": "mesh_fill_bench.json", "auto": "mesh_fill_area_bench.json"}.get(a.method, f"mesh_fill_area_bench_{a.method}.json"))


if __name__ == "__main__":
    main()
