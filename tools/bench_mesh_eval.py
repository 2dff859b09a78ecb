"""Time the mesh-evaluation path: nearest-neighbour index build and query at 200k x 200k and with 1M targets,
sample_surface at 200k points, one ICP run from the 512^3 mesh of tools/bench_mesh.py's model onto a copy moved by a known small
rigid transform, and mesh_metrics end to end.  Device events, warm-up first, medians; per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  The mean number of candidate points per query is estimated from the
grid's occupancy (points in the 3x3x3 cells around a target's cell, averaged over targets).  When scipy is importable,
cKDTree build + query is timed as the host baseline.
usage: python tools/bench_mesh_eval.py [reps=5] [resolution=512]"""
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

from benchlib import median_ms, model_mesh, positionals, write_results
from nicer_slam_amd import mesh_eval as M


def parse_args(argv):
    return positionals(argv, reps=(int, 5), resolution=(int, 512))


def candidates(ix):
    """mean points in the 27 cells around a target's own cell (the first ring a query near the targets reads)"""
    _, _, R, counts = ix.grid()
    c = counts.float()[None, None]
    nb = F.conv3d(F.pad(c, (1, 1, 1, 1, 1, 1)), torch.ones(1, 1, 3, 3, 3, device=c.device))[0, 0]
    return float((c[0, 0] * nb).sum() / c.sum()), R.tolist()


def nn_case(name, t, q, out, reps):
    ix = M.NNIndex(t)
    out[name + " build ms"] = median_ms(lambda: M.NNIndex(t), reps)
    out[name + " query ms"] = median_ms(lambda: ix.query(q), reps)
    out[name + " candidates/query"], out[name + " grid"] = candidates(ix)


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    reps = args.reps
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    mesh = model_mesh(args.resolution)
    v, f = mesh["verts"], mesh["faces"]
    out["mesh V"], out["mesh F"] = int(v.shape[0]), int(f.shape[0])
    surf, _ = M.sample_surface(v, f, 200000, 0)
    surf2, _ = M.sample_surface(v, f, 200000, 1)
    nn_case("nn surface 200k x 200k", surf, surf2, out, reps)
    u = torch.rand(200000, 3, device="cuda", generator=g)
    nn_case("nn uniform 200k x 200k", u, torch.rand(200000, 3, device="cuda", generator=g), out, reps)
    big, _ = M.sample_surface(v, f, 1000000, 2)
    nn_case("nn surface 1M targets x 200k", big, surf2, out, reps)
    out["sample_surface 200k ms"] = median_ms(lambda: M.sample_surface(v, f, 200000, 0), reps)

    import eval_ref as E
    T = E.rigid([0.2, 1.0, -0.4], 2.0, [0.01, -0.005, 0.008])
    src = torch.from_numpy(E.transform(v.cpu().numpy().astype(np.float64), T).astype(np.float32)).cuda()
    res = {}
    out["icp ms"] = median_ms(lambda: res.update(M.icp_point_to_point(src, v, 0.1)), max(1, reps // 2))
    out["icp iterations"], out["icp fitness"] = res["iterations"], res["fitness"]
    out["icp max |T - T_true^-1|"] = float(np.abs(res["transformation"] - np.linalg.inv(T)).max())
    moved = {"verts": src, "faces": f}
    met = {}
    out["mesh_metrics ms"] = median_ms(lambda: met.update(M.mesh_metrics(moved, mesh)), max(1, reps // 2))
    out["mesh_metrics accuracy"], out["mesh_metrics completion"] = met["accuracy"], met["completion"]

    try:
        from scipy.spatial import cKDTree
        a, b = surf.cpu().numpy(), surf2.cpu().numpy()
        t0 = time.perf_counter()
        cKDTree(a).query(b)
        out["host cKDTree build+query 200k x 200k ms"] = (time.perf_counter() - t0) * 1e3
    except ImportError:
        out["host cKDTree build+query 200k x 200k ms"] = None
    write_results(out)


if __name__ == "__main__":
    main()
