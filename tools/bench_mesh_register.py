"""Time point-to-plane registration at [rows] source rows -- area-weighted samples of a marching-cubes blob whose vertex
count is near the row count, moved by a small rigid motion -- against that mesh: its vertices with angle-weighted normals (cloud mode)
and its surface (surface mode).  Device events or a host clock around a synchronise, warm-up first, medians.  Reported per size:
  * one iteration of each mode split into the move (nsa_icp_transform), the query, the system (nsa_icp_plane_system) and the host step
    (the readback of 32 words, the 6x6 LDL^T, the update), and the whole iteration end to end;
  * baselines of the same split: the same rows composed of torch operations (time only: its sums have no fixed order), and one iteration
    of mesh_eval.icp_point_to_point (the difference of a two- and a one-iteration call);
  * the system launch against device copies of the bytes it must read (n * 56 B in cloud mode: the point, the index, the distance and
    the gathered target and normal), on buffers of the same sizes;
  * iterations, wall time and the error of the 4x4 of the three metrics run to convergence on the same pair.
Results go to profiles/mesh_register_bench.json.
usage: python tools/bench_mesh_register.py [reps=7] [rows=200000,2000000]"""
import json
import math
import sys

import numpy as np
import torch

from benchlib import median, median_ms, positionals, time_host, write_results
from nicer_slam_amd import _native, inference, mesh_eval as E, mesh_register as M, mesh_smooth
from nicer_slam_amd._native import check, lib

DEFAULT_ROWS = [200000, 2000000]
MAX_CORR = 0.1
MAX_GRID = 1280                      # marching cubes takes up to 2^31 samples: the 2 M case gets the finest blob that fits


def rigid(axis, deg, t):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(math.radians(deg)) * K + (1 - math.cos(math.radians(deg))) * K @ K
    T[:3, 3] = t
    return T


MOTION = rigid([0.2, 1.0, -0.4], 3.0, [0.03, -0.02, 0.025])


def parse_args(argv):
    return positionals(argv, reps=(int, 7), rows=(lambda s: [int(x) for x in s.split(",")], DEFAULT_ROWS))


def blob(res):
    """the three-sphere blob of the tests, fp32, by broadcasting"""
    ax = torch.linspace(-1, 1, res, device="cuda")
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    s = lambda c, r: torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r
    vol = torch.minimum(torch.minimum(s((0.2, 0, 0), 0.4), s((-0.35, 0.25, 0.1), 0.25)), s((0, -0.3, 0.35), 0.2))
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol.contiguous(), 0.0, (step,) * 3, (-1.0,) * 3)


def mesh_with_about(n_verts):
    v64 = blob(64)["verts"].shape[0]
    res = min(max(16, int(round(64 * math.sqrt(n_verts / v64)))), MAX_GRID)
    return blob(res), res


def composed_system(cur, idx, tgt, nrm):
    """the cloud-mode rows and their sums out of torch operations (L2); float64, whatever order torch picks"""
    ok = idx >= 0
    safe = idx.clamp_min(0).long()
    q, n = tgt[safe].double(), nrm[safe].double()
    d = cur - q
    r = (n * d).sum(1)
    J = torch.cat([torch.linalg.cross(cur, n), n], 1) * ok[:, None]
    r = r * ok
    A = J.T @ J
    b = J.T @ r
    return torch.cat([A.reshape(-1), b, (r * r).sum()[None], (d * d).sum(1)[ok].sum()[None], ok.sum()[None].double()]).cpu()


def case(n, out, reps):
    timed = lambda fn: median_ms(fn, reps)                           # median ms by device events
    walled = lambda fn, k=reps: median(time_host(fn, k))             # median ms by the host clock
    mesh, res = mesh_with_about(n)
    gv, gf = mesh["verts"].float().contiguous(), mesh["faces"].to(torch.int32).contiguous()
    r = {"rows": n, "grid": res, "target vertices": gv.shape[0], "target faces": gf.shape[0]}
    pts, _ = E.sample_surface(gv, gf, n, 2)
    src = E._transform(pts.double(), torch.from_numpy(MOTION).cuda()).float().contiguous()
    truth = np.linalg.inv(MOTION)
    nrm = mesh_smooth.vertex_normals({"verts": gv, "faces": gf}, "angle").contiguous()
    nn, tri = E.NNIndex(gv), E.TriIndex(gv, gf)
    dev = src.device
    stream = torch.cuda.current_stream(dev).cuda_stream

    cur = src.double()
    cur32 = torch.empty(n, 3, device=dev)
    M._move(cur, np.eye(4), cur32)
    corr = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    closest = torch.empty(n, 3, device=dev)
    system = M._System(n, dev)
    small = rigid([1, 0, 0], 1e-9, [0, 0, 0])                       # a move that leaves the rows where they are, to the eye

    def q_cloud():
        check(lib.nsa_nn_query(nn.buf.data_ptr(), nn.n, cur32.data_ptr(), n, MAX_CORR, corr.data_ptr(), dist.data_ptr(), stream))

    def q_surface():
        check(lib.nsa_tri_query_bounded(tri.buf.data_ptr(), tri.verts.data_ptr(), tri.V, tri.faces.data_ptr(), tri.F, cur32.data_ptr(), n,
                                        MAX_CORR * MAX_CORR, corr.data_ptr(), d2.data_ptr(), closest.data_ptr(), None, None, stream))

    def host_step():
        s = system.read()
        x = M.ldlt_solve(s["A"], s["b"])
        return M.update_matrix(x) if x is not None else None

    r["move ms"] = timed(lambda: M._move(cur, small, cur32))
    for mode, query, run in (("cloud", q_cloud, lambda: system.run(cur, _native.ICP_CLOUD, corr, (dist, gv, nrm), None, 0, 0.0)),
                             ("surface", q_surface, lambda: system.run(cur, _native.ICP_SURFACE, corr, None, (d2, closest, tri.verts, tri.faces), 0, 0.0))):
        m = {}
        m["query ms"] = timed(query)
        query()
        m["system ms"] = timed(run)
        run()
        torch.cuda.synchronize()
        m["host step ms (readback of 32 words, LDL^T, update)"] = walled(host_step)
        m["matched fraction"] = system.read()["k_corr"] / n

        def iteration():
            M._move(cur, small, cur32)
            query()
            run()
            host_step()
        m["one iteration end to end ms"] = walled(iteration)
        for name, kernel in (("huber", 1), ("tukey", 2)):
            k_run = (lambda kk: (lambda: system.run(cur, _native.ICP_CLOUD if mode == "cloud" else _native.ICP_SURFACE, corr,
                                                    (dist, gv, nrm) if mode == "cloud" else None,
                                                    None if mode == "cloud" else (d2, closest, tri.verts, tri.faces), kk, 0.01)))(kernel)
            m[f"system ms, {name}"] = timed(k_run)
        r[mode] = m

    # the system against copies of the bytes it must read
    q_cloud()
    bufs = [cur, corr, dist, torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)]
    dsts = [torch.empty_like(b) for b in bufs]
    nbytes = sum(b.numel() * b.element_size() for b in bufs)

    def copies():
        for a, b in zip(dsts, bufs):
            a.copy_(b)
    r["bytes the cloud system must read"] = nbytes
    r["device copies of those bytes ms (read and write)"] = timed(copies)
    r["cloud system over the copies"] = r["cloud"]["system ms"] / r["device copies of those bytes ms (read and write)"]
    r["cloud system GB/s of the bytes it must read"] = nbytes / 1e6 / r["cloud"]["system ms"]

    # baselines
    r["composed torch rows and sums ms (cloud, L2)"] = walled(lambda: composed_system(cur, corr, gv, nrm))
    p1 = walled(lambda: E.icp_point_to_point(src, gv, MAX_CORR, max_iter=1, index=nn))
    p2 = walled(lambda: E.icp_point_to_point(src, gv, MAX_CORR, max_iter=2, index=nn))
    r["icp_point_to_point, one iteration ms (2 iterations - 1)"] = p2 - p1
    r["composed torch move ms (mesh_eval._transform + .float())"] = timed(lambda: E._transform(cur, torch.from_numpy(small).to(dev)).float())

    # to convergence, the same pair
    conv = {}
    for name, fn in (("point", lambda: E.icp_point_to_point(src, gv, MAX_CORR, index=nn)),
                     ("plane", lambda: M.icp_point_to_plane(src, gv, nrm, MAX_CORR, index=nn)),
                     ("surface", lambda: M.icp_point_to_plane(src, tri, None, MAX_CORR))):
        res_ = fn()
        conv[name] = {"iterations": res_["iterations"], "wall ms": walled(fn, 3), "max abs error of the 4x4": float(np.abs(res_["transformation"] - truth).max()),
                      "fitness": res_["fitness"], "inlier rmse": res_["inlier_rmse"]}
    again = M.icp_point_to_plane(src, tri, None, MAX_CORR)
    conv["surface: two runs give equal bits"] = bool(np.array_equal(again["transformation"].view(np.uint64), res_["transformation"].view(np.uint64)))
    r["to convergence"] = conv
    out[f"{n} rows"] = r
    print(json.dumps({f"{n} rows": r}, indent=1), flush=True)


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_register: needs a GPU")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "max_corr": MAX_CORR}
    for n in a.rows:
        case(n, out, a.reps)
        torch.cuda.empty_cache()
    if a.rows == DEFAULT_ROWS:                                    # (every row was printed as it was made)
        write_results(out, "mesh_register_bench.json", echo=False)


if __name__ == "__main__":
    main()
