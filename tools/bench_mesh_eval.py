"""Time the mesh-evaluation path: nearest-neighbour index build and query at 200k x 200k and with 1M targets,
sample_surface at 200k points, one ICP run from the 512^3 mesh of tools/bench_mesh.py's model onto a copy moved by a known small
rigid transform, and mesh_metrics end to end.  Device events, warm-up first, medians; per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  The mean number of candidate points per query is estimated from the
grid's occupancy (points in the 3x3x3 cells around a target's cell, averaged over targets).  When scipy is importable,
cKDTree build + query is timed as the host baseline.
usage: python tools/bench_mesh_eval.py [reps=5] [resolution=512]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

from nicer_slam_amd import inference, mesh_eval as M

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
RES = int(sys.argv[2]) if len(sys.argv) > 2 else 512


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


def candidates(ix):
    """mean points in the 27 cells around a target's own cell (the first ring a query near the targets reads)"""
    _, _, R, counts = ix.grid()
    c = counts.float()[None, None]
    nb = F.conv3d(F.pad(c, (1, 1, 1, 1, 1, 1)), torch.ones(1, 1, 3, 3, 3, device=c.device))[0, 0]
    return float((c[0, 0] * nb).sum() / c.sum()), R.tolist()


def nn_case(name, t, q, out):
    ix = M.NNIndex(t)
    out[name + " build ms"] = timed(lambda: M.NNIndex(t))
    out[name + " query ms"] = timed(lambda: ix.query(q))
    out[name + " candidates/query"], out[name + " grid"] = candidates(ix)


def main():
    out = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    from bench_mesh import model
    mesh = inference.extract_mesh(model(), RES, (-1.0, 1.0), color=False)
    v, f = mesh["verts"], mesh["faces"]
    out["mesh V"], out["mesh F"] = int(v.shape[0]), int(f.shape[0])
    surf, _ = M.sample_surface(v, f, 200000, 0)
    surf2, _ = M.sample_surface(v, f, 200000, 1)
    nn_case("nn surface 200k x 200k", surf, surf2, out)
    u = torch.rand(200000, 3, device="cuda", generator=g)
    nn_case("nn uniform 200k x 200k", u, torch.rand(200000, 3, device="cuda", generator=g), out)
    big, _ = M.sample_surface(v, f, 1000000, 2)
    nn_case("nn surface 1M targets x 200k", big, surf2, out)
    out["sample_surface 200k ms"] = timed(lambda: M.sample_surface(v, f, 200000, 0))

    import eval_ref as E
    T = E.rigid([0.2, 1.0, -0.4], 2.0, [0.01, -0.005, 0.008])
    src = torch.from_numpy(E.transform(v.cpu().numpy().astype(np.float64), T).astype(np.float32)).cuda()
    res = {}
    out["icp ms"] = timed(lambda: res.update(M.icp_point_to_point(src, v, 0.1)), reps=max(1, REPS // 2))
    out["icp iterations"], out["icp fitness"] = res["iterations"], res["fitness"]
    out["icp max |T - T_true^-1|"] = float(np.abs(res["transformation"] - np.linalg.inv(T)).max())
    moved = {"verts": src, "faces": f}
    met = {}
    out["mesh_metrics ms"] = timed(lambda: met.update(M.mesh_metrics(moved, mesh)), reps=max(1, REPS // 2))
    out["mesh_metrics accuracy"], out["mesh_metrics completion"] = met["accuracy"], met["completion"]

    try:
        from scipy.spatial import cKDTree
        a, b = surf.cpu().numpy(), surf2.cpu().numpy()
        t0 = time.perf_counter()
        cKDTree(a).query(b)
        out["host cKDTree build+query 200k x 200k ms"] = (time.perf_counter() - t0) * 1e3
    except ImportError:
        out["host cKDTree build+query 200k x 200k ms"] = None
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
