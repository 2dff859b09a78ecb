"""Time k nearest neighbours and cloud normals on [points] surface samples of a room-like mesh (a 4 x 3 x 2.5 box seen from
inside with two boxes standing in it) and on as many uniform points of the same box; queries are the cloud itself.  Device events or a
host clock around a synchronise, warm-up first, medians.  Reported per cloud:
  * NNIndex.query (one neighbour: the yardstick for what k costs) and nsa_nn_query_k at k = 1, 8, 30, 64, without and with a radius;
  * nsa_cloud_normals alone at k = 30 on the k-NN result, against device copies of the bytes it must read and write;
  * estimate_normals whole (index build, query, normals), and with a prebuilt index;
and once: the list capacities' LDS bytes, waves per SIMD (tools/kernel_resources.sh) and workgroups per CU.
Results go to profiles/cloud_normals_bench.json.
usage: python tools/bench_cloud_normals.py [reps=7] [points=200000]"""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import torch

from benchlib import ROOT, median, median_ms, positionals, time_host, write_results
from nicer_slam_amd import cloud_normals as C, mesh_eval as E
from nicer_slam_amd._native import check, lib

KS = (1, 8, 30, 64)
LDS_PER_CU = 160 * 1024


def parse_args(argv):
    return positionals(argv, reps=(int, 7), points=(int, 200000))


def box(lo, hi):
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 np.int32)
    return v, f


def room():
    parts = [box((0, 0, 0), (4, 3, 2.5)), box((0.5, 0.4, 0), (1.7, 1.0, 0.75)), box((2.6, 1.8, 0), (3.5, 2.8, 1.9))]
    verts, faces, base = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(f + base)
        base += len(v)
    return torch.from_numpy(np.concatenate(verts)).cuda(), torch.from_numpy(np.concatenate(faces)).cuda()


def capacities():
    """{capacity: LDS bytes, waves per SIMD, workgroups per CU} of k_nn_query_k from the compiler's remarks; {} without hipcc"""
    try:
        text = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), "mesh_eval"], capture_output=True, text=True,
                              timeout=300).stdout
    except (OSError, subprocess.TimeoutExpired):
        return {}
    out = {}
    for m in re.finditer(r"k_nn_query_k<(\d+)u>\s+vgpr\s+(\d+).*?lds\s+(\d+) occ (\d+)", text):
        cap, vgpr, lds, occ = (int(x) for x in m.groups())
        # one wave per workgroup: a CU holds what its LDS admits, and no more waves than 4 SIMDs times the compiler's occupancy
        out[f"capacity {cap}"] = {"vgpr": vgpr, "lds bytes per workgroup": lds, "waves per SIMD by registers and LDS": occ,
                                  "workgroups per CU": min(LDS_PER_CU // lds, 4 * occ)}
    return out


def case(name, pts, out, reps):
    timed = lambda fn: median_ms(fn, reps)                           # median ms by device events
    walled = lambda fn: median(time_host(fn, reps))                  # median ms by the host clock
    n = pts.shape[0]
    dev = pts.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    index = E.NNIndex(pts)
    r = {"points": n, "index build ms": walled(lambda: E.NNIndex(pts))}
    idx1 = torch.empty(n, dtype=torch.int32, device=dev)
    dist1 = torch.empty(n, device=dev)
    radius = 4.0 * (4 * 3 * 2.5 / n) ** (1 / 3) if name == "uniform" else 4.0 * math.sqrt(60.0 / n)
    for label, md in (("", math.inf), (f", radius {radius:.4f}", radius)):
        r["query ms" + label] = timed(lambda: check(lib.nsa_nn_query(index.buf.data_ptr(), n, pts.data_ptr(), n, md, idx1.data_ptr(),
                                                                     dist1.data_ptr(), stream)))
        for k in KS:
            idx = torch.empty(n, k, dtype=torch.int32, device=dev)
            dist = torch.empty(n, k, device=dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            r[f"knn k={k} ms" + label] = timed(lambda: check(lib.nsa_nn_query_k(index.buf.data_ptr(), n, pts.data_ptr(), n, k, md,
                                                                                idx.data_ptr(), dist.data_ptr(), count.data_ptr(), stream)))
            if md < math.inf:
                r[f"knn k={k} mean count" + label] = float(count.double().mean())
    r["knn k=1 over query"] = r["knn k=1 ms"] / r["query ms"]
    r["knn k=30 over query"] = r["knn k=30 ms"] / r["query ms"]
    _, idx, count = index._knn(pts, 30, math.inf)
    r["nsa_cloud_normals k=30 ms"] = timed(lambda: C.normals_from_neighbours(pts, idx, count, pts, None, True))
    r["nsa_cloud_normals k=30 ms, one viewpoint, no eigenvalues"] = timed(
        lambda: C.normals_from_neighbours(pts, idx, count, pts, torch.zeros(3, device=dev), False))
    bufs = [idx, count, pts, torch.empty(n, 3, device=dev), torch.empty(n, 3, dtype=torch.float64, device=dev)]
    dsts = [torch.empty_like(b) for b in bufs]

    def copies():
        for a, b in zip(dsts, bufs):
            a.copy_(b)
    r["bytes it reads and writes, the gathered points not counted"] = sum(b.numel() * b.element_size() for b in bufs)
    r["device copies of those bytes ms"] = timed(copies)
    r["estimate_normals k=30 whole ms"] = walled(lambda: C.estimate_normals(pts, 30))
    r["estimate_normals k=30 prebuilt index ms"] = walled(lambda: C.estimate_normals(pts, 30, index=index))
    normals, info = C.estimate_normals(pts, 30, info=True, index=index)
    r["valid fraction"] = float(info["valid"].double().mean())
    r["median surface variation"] = float(info["variation"][info["valid"]].median())
    again = C.estimate_normals(pts, 30)
    r["two runs give equal bits"] = bool(torch.equal(again.view(torch.int32), normals.view(torch.int32)))
    out[name] = r
    print(json.dumps({name: r}, indent=1), flush=True)


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_normals: needs a GPU")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    v, f = room()
    samples, _ = E.sample_surface(v, f, a.points, 1)
    case("room", samples.contiguous(), out, a.reps)
    g = torch.Generator(device="cuda").manual_seed(1)
    uniform = torch.rand(a.points, 3, device="cuda", generator=g) * torch.tensor([4.0, 3.0, 2.5], device="cuda")
    case("uniform", uniform.contiguous(), out, a.reps)
    out["k_nn_query_k list capacities"] = capacities()
    print(json.dumps(out["k_nn_query_k list capacities"], indent=1), flush=True)
    if a.points == 200000:                                        # (every row was printed as it was made)
        write_results(out, "cloud_normals_bench.json", echo=False)


if __name__ == "__main__":
    main()
