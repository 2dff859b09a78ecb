"""Time mesh smoothing on the two meshes of the other mesh benches -- the 512^3 mesh of tools/bench_mesh.py's model and
the mesh fused from tools/bench_tsdf.py's room.  Device events, warm-up first, medians.  Timed: the ring build (nsa_mesh_ring on a
finished edge table), the smoothing prologue, one step (the difference of a 21- and a 1-step call over 20), ``smooth()`` end to end for
10 Taubin pairs (edge table, ring, steps, angle normals, the read-back of the totals), ``vertex_normals`` for each weighting.
Comparison points, there being no reference program and no earlier version: the composed route on the same GPU -- ``torch.unique``
over the edge keys and one float64 ``index_add_`` per step, whose sums have no fixed order -- and the numpy statement of
tests/smooth_ref.py on the host.  A third mesh, a synthetic lattice of [lattice side]^2 vertices with random heights, is large enough
that the positions and neighbour lists do not fit the caches; the host oracle is left out there.  Results go to
profiles/mesh_smooth_bench.json.
usage: python tools/bench_mesh_smooth.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100] [lattice side=3000, 0: none]"""
import sys
import time

import torch

from benchlib import median_ms, mesh_positionals, model_mesh, tsdf_mesh, write_results
from nicer_slam_amd import mesh_smooth as M, mesh_topology as MT

TAUBIN = M.factors_of("taubin", 10)


def parse_args(argv):
    return mesh_positionals(argv, lattice=(int, 3000))


def composed_setup(f, V):
    a, b = f.long().reshape(-1), f[:, [1, 2, 0]].long().reshape(-1)
    key = torch.unique(torch.minimum(a, b) * V + torch.maximum(a, b))
    lo, hi = torch.div(key, V, rounding_mode="floor"), key % V
    src, dst = torch.cat([lo, hi]), torch.cat([hi, lo])
    deg = torch.zeros(V, dtype=torch.float64, device=f.device).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64, device=f.device))
    return src, dst, deg


def composed_steps(v, src, dst, deg, factors):
    """boundary "free", no mask, no clamp: the neighbour sums by index_add_ (float64 atomics, no fixed order)"""
    X = v.double()
    has = (deg > 0)[:, None]
    n = deg.clamp_min(1.0)[:, None]
    for fct in factors:
        S = torch.zeros_like(X).index_add_(0, dst, X[src])
        X = torch.where(has, X + fct * (S / n - X), X)
    return X.float()


def lattice(n, seed=2):
    """an n x n lattice of unit cells split along one diagonal, random heights: tests/smooth_ref.grid_mesh on the device"""
    dev = "cuda"
    k = torch.arange(n, device=dev)
    i, j = torch.meshgrid(k, k, indexing="ij")
    z = 0.3 * torch.rand(n, n, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)
    v = torch.stack([i.float(), j.float(), z], 2).reshape(-1, 3).contiguous()
    ci, cj = (x.reshape(-1) for x in torch.meshgrid(k[:-1], k[:-1], indexing="ij"))
    a, b, c, d = ci * n + cj, (ci + 1) * n + cj, (ci + 1) * n + cj + 1, ci * n + cj + 1
    f = torch.cat([torch.stack([a, b, c], 1), torch.stack([a, c, d], 1)]).to(torch.int32).contiguous()
    return dict(verts=v, faces=f)


def case(name, mesh, out, reps, host=True):
    timed = lambda fn: median_ms(fn, reps)
    v, f = mesh["verts"].float().contiguous(), mesh["faces"].contiguous()
    V, F = v.shape[0], f.shape[0]
    plain = dict(verts=v, faces=f)
    r = {"V": V, "F": F}
    t, totals = MT._edge_table(f, V, F, None)
    r["E"] = totals["n_edges"]
    r["boundary edges"] = totals["n_boundary"]
    r["edge_table() ms"] = timed(lambda: MT.edge_table(f, V))
    r["ring build ms"] = timed(lambda: M._ring(t, V, F, f.device))
    rings = M._ring(t, V, F, f.device)
    run = lambda factors, boundary="curve": M._smooth(v, V, F, t, rings, factors, boundary, None, None)
    r["smooth kernels, 0 steps (prologue + copy) ms"] = timed(lambda: run([]))
    one, many = timed(lambda: run([0.5])), timed(lambda: run([0.5] * 21))
    r["smooth kernels, 1 step ms"], r["smooth kernels, 21 steps ms"] = one, many
    step = (many - one) / 20.0
    r["one step ms"] = step
    out_v, state = run(TAUBIN)
    n_members = int(torch.diff(rings[0].long()).sum())                    # upper bound of the gathered entries (all live, free)
    # per vertex: its float64 position in and out, its count and offset; per neighbour: the index and the gathered float64 position
    r["step MB moved at least"] = (V * (24 + 24 + 8) + n_members * (4 + 24)) / 1e6
    r["step GB/s"] = r["step MB moved at least"] / 1e3 / (step / 1e3) if step > 0 else None
    # what must cross the memory interface when the caches serve every repeated gather: each position in once and out once
    r["step MB with every position fetched once"] = (V * (24 + 24 + 8) + n_members * 4) / 1e6
    r["step GB/s with every position fetched once"] = r["step MB with every position fetched once"] / step if step > 0 else None
    r["smooth() 10 taubin pairs, angle normals, end to end ms"] = timed(lambda: M.smooth(plain))
    r["smooth() 10 taubin pairs, normals=None, end to end ms"] = timed(lambda: M.smooth(plain, normals=None))
    _, r["report"] = M.smooth(plain, return_report=True)
    for w in ("angle", "area"):
        r[f"vertex_normals({w}) ms"] = timed(lambda: M.vertex_normals(plain, w))
    if "normals" in mesh:
        cos = (M.vertex_normals(plain, "angle") * mesh["normals"]).sum(1)
        r["cosine of recomputed and marching-cubes normals (min, median)"] = [float(cos.min()), float(cos.median())]
    # the composed route on the same GPU
    r["composed: torch.unique edges + degrees ms"] = timed(lambda: composed_setup(f, V))
    src, dst, deg = composed_setup(f, V)
    r["composed: 20 index_add_ steps ms"] = timed(lambda: composed_steps(v, src, dst, deg, TAUBIN))
    r["composed: one step ms"] = r["composed: 20 index_add_ steps ms"] / 20.0
    free = run(TAUBIN, "free")[0]
    r["max |composed - device| (boundary free)"] = float((composed_steps(v, src, dst, deg, TAUBIN) - free).abs().max())
    a, b = composed_steps(v, src, dst, deg, TAUBIN), composed_steps(v, src, dst, deg, TAUBIN)
    r["composed route bit-identical between two runs"] = bool(torch.equal(a, b))
    r["device bit-identical between two runs"] = bool(torch.equal(run(TAUBIN)[0], out_v))
    if not host:
        out[name] = r
        return
    # the numpy statement on the host
    import smooth_ref as S
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    t0 = time.perf_counter()
    ring = S.vertex_ring(hf, V)
    r["host oracle: edge table + ring s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref, _ = S.smooth_steps(hv, hf, TAUBIN, ring=ring)
    r["host oracle: 20 steps s"] = time.perf_counter() - t0
    r["device equals the host oracle bit for bit"] = bool(ref.tobytes() == out_v.cpu().numpy().tobytes())
    out[name] = r


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    case(f"model mesh {a.resolution}^3", model_mesh(a.resolution), out, a.reps)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", tsdf_mesh(a.voxels, a.frames), out, a.reps)
    if a.lattice:
        case(f"lattice {a.lattice}^2, random heights", lattice(a.lattice), out, a.reps, host=False)
    write_results(out, "mesh_smooth_bench.json")


if __name__ == "__main__":
    main()
