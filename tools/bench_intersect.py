"""Time the self-intersection query on two meshes: the marching-cubes sphere of tools/bench_raycast.py (128^3: 38 012 faces)
and the TSDF room of tools/bench_mesh_clean.py after fill_holes(method="auto").  Device events, one warm-up, medians of 20: the build
of the tree, the count pass (states, walk, scan and totals) and the emit pass on their own, and the whole call with its read back and
sort; candidates per face and the share of each stage.  The comparison is this unit's own brute force on the first faces of the sphere
(a count at which all pairs finish well under a second): the ratio is reported, no threshold is set on it.  There is no earlier
version and no runnable reference program, so no time is gated.  Results go to profiles/intersect_bench.json.
usage: python tools/bench_intersect.py [reps=20] [resolution=128] [tsdf voxels=256] [tsdf frames=100] [brute faces=8192]"""
import json
import sys

import torch

from benchlib import mc_sphere, median_ms, mesh_positionals, tsdf_mesh, write_results
from nicer_slam_amd import mesh_fill, mesh_intersect as M
from nicer_slam_amd._native import check, lib
from nicer_slam_amd.mesh_eval import TriIndex


def parse_args(argv):
    return mesh_positionals(argv, reps=20, resolution=128, brute_faces=(int, 8192))


def passes(ix, reps, brute=False):
    """ms of the count and the emit entry points on their own, and the totals"""
    timed = lambda fn: median_ms(fn, reps)
    dev, F = ix.device, ix.F
    s = torch.cuda.current_stream(dev).cuda_stream
    buf, _ = ix._ray_tree()
    ws = torch.empty(lib.nsa_tri_isect_workspace(F), dtype=torch.uint8, device=dev)
    state = torch.empty(F, dtype=torch.uint8, device=dev)
    totals = torch.zeros(16, dtype=torch.int64, device=dev)
    mesh = (buf.data_ptr(), ix.verts.data_ptr(), ix.V, ix.faces.data_ptr(), F, None, M.BRUTE if brute else 0)
    count = lambda: check(lib.nsa_tri_isect_count(*mesh, ws.data_ptr(), state.data_ptr(), totals.data_ptr(), s))
    out = {"count pass ms": timed(count)}
    n = int(totals[0])
    pairs = torch.empty(max(n, 1), 2, dtype=torch.int64, device=dev)
    code = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    out["emit pass ms"] = timed(lambda: check(lib.nsa_tri_isect_emit(*mesh, ws.data_ptr(), state.data_ptr(), n, pairs.data_ptr(),
                                                                     code.data_ptr(), s))) if n else 0.0
    out["records"] = n
    return out


def case(name, mesh, out, reps):
    v, f = mesh["verts"].contiguous(), mesh["faces"].contiguous()
    r = {"V": int(v.shape[0]), "F": int(f.shape[0])}

    def build():
        ix = TriIndex(v, f)
        ix._ray_tree()
        return ix
    r["index and tree build ms"] = median_ms(build, max(3, reps // 4))
    ix = build()
    r.update(passes(ix, reps))
    r["whole call ms (read back, sort, flags)"] = median_ms(lambda: ix.self_intersections(), reps)
    rep = ix.self_intersections(return_report=True)[3]
    r["report"] = rep
    r["candidates per face"] = rep["n_candidates"] / max(1, rep["n_faces"])
    c = max(1, rep["n_candidates"])
    r["stage shares"] = {"float64 filter": rep["n_stage1"] / c, "256-bit integers": rep["n_exact"] / c, "host": rep["n_host"] / c}
    out[name] = r
    print(name, json.dumps(r))
    return ix


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"reps": a.reps}
    sphere = mc_sphere(a.resolution)
    case(f"marching-cubes sphere {a.resolution}^3", sphere, out, a.reps)
    small = TriIndex(sphere["verts"].contiguous(), sphere["faces"][:a.brute_faces].contiguous())
    tree, brute = passes(small, a.reps), passes(small, a.reps, brute=True)
    t, b = tree["count pass ms"] + tree["emit pass ms"], brute["count pass ms"] + brute["emit pass ms"]
    out[f"first {small.F} faces of the sphere"] = {"tree": tree, "brute": brute, "brute / tree": b / t}
    print("brute force", json.dumps(out[f"first {small.F} faces of the sphere"]))
    room = mesh_fill.fill_holes(tsdf_mesh(a.voxels, a.frames), method="auto", normals="none")
    case("tsdf room, holes filled (method auto)", room, out, a.reps)
    print("->", write_results(out, "intersect_bench.json", echo=False))    # (every row was printed as it was made)


if __name__ == "__main__":
    main()
