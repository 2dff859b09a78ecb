"""Time the closest-point-on-mesh path: TriIndex build and query for 200k surface samples against the 512^3 mesh of
tools/bench_mesh.py's model (queries: samples of the mesh itself, the same samples pushed off the surface by N(0, 0.01), and uniform
points of the bounding cube), the faces fully evaluated per query (the kernel's own count), the share of faces on the large list,
and mesh_metrics end to end in both modes; then the signed and the range-limited queries of DESIGN 4n on the same mesh and queries:
signed against unsigned, the uniform points under a band of 2, 5 and 20 cells, the adjacency build and its bytes, the incident faces
walked per query, and mesh_sdf_grid at 256^3 with a band of 4 voxels; then the winding numbers of DESIGN 4o: the tree build and its
bytes, the tree query at beta = 2 and 3 on the three query sets with the nodes accepted and the faces summed exactly per query, the
exact sum on the first 20000 of each, and mesh_sdf_grid(sign="winding") beside the "normal" one.  Device events, warm-up first, medians; per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  Baseline: a chunked torch float64 brute force on the same GPU at a size it
finishes in a few seconds (queries x faces given below), compared against the index on the same inputs.
usage: python tools/bench_mesh_closest.py [reps=5] [resolution=512] [out=profiles/mesh_closest_bench.json] [legs=all|winding]"""
import sys

import numpy as np
import torch

from benchlib import median_ms, model_mesh, positionals, write_results
from nicer_slam_amd import mesh_eval as M


def parse_args(argv):
    return positionals(argv, reps=(int, 5), resolution=(int, 512), out=(str, None),      # out: None is profiles/mesh_closest_bench.json
                       legs=(str, "all"))


def query_case(name, ix, q, out, reps):
    out[name + " query ms"] = median_ms(lambda: ix.query(q), reps)
    dist, _, _, n = ix.query(q, counts=True)
    n = n.double()
    out[name + " faces evaluated/query"] = {"mean": float(n.mean()), "median": float(n.median()), "max": int(n.max())}
    out[name + " mean distance"] = float(dist.mean())


def walked(ix, face, feature):
    """incident corners each query's pseudo-normal walked: the vertex's list, the shorter endpoint list of an edge, 0 inside a face
    (read from the adjacency buffer: start[V + 2] at its head, csrc/mesh_sdf.hip)"""
    adj, buf = ix.adjacency(True)
    start = buf[:4 * (ix.V + 2)].view(torch.int32).long()
    val = start[1:ix.V + 1] - start[:ix.V]
    ft = feature.long().clamp_min(0)
    names = adj.long()[face.clamp_min(0)]                                        # [m, 3]
    first = torch.tensor([0, 0, 1, 0, 2, 0, 1], device=face.device)[ft]         # per feature code: a corner, and the other end of an edge
    second = torch.tensor([0, 0, 1, 1, 2, 2, 2], device=face.device)[ft]
    n = torch.minimum(val[names.gather(1, first[:, None])[:, 0]], val[names.gather(1, second[:, None])[:, 0]])
    return torch.where((feature > 0) & (face >= 0), n, torch.zeros_like(n)).double()


def signed_case(name, ix, q, out, reps):
    out[name + " signed query ms"] = median_ms(lambda: ix.signed_query(q), reps)
    dist, face, _, feature = ix.signed_query(q)
    n = walked(ix, face, feature)
    out[name + " incident faces walked/query"] = {"mean": float(n.mean()), "max": int(n.max())}
    out[name + " share negative"] = float((dist < 0).double().mean())
    out[name + " features (interior, vertex, edge)"] = [float((feature == 0).double().mean()),
                                                        float(((feature == 1) | (feature == 2) | (feature == 4)).double().mean()),
                                                        float(((feature == 3) | (feature == 5) | (feature == 6)).double().mean())]


def sdf_rows(ix, surf, near, cube, out, reps):
    timed = lambda fn, n=reps: median_ms(fn, n)
    from nicer_slam_amd import mesh_sdf
    out["adjacency bytes"] = int(M.lib.nsa_tri_adjacency_workspace(ix.V, ix.F))

    def build():
        ix._adjacency.clear()
        ix.adjacency(True)

    out["adjacency build ms (weld included)"] = timed(build)
    signed_case("on surface 200k", ix, surf, out, reps)
    signed_case("near surface (sigma 0.01) 200k", ix, near, out, reps)
    h = max(ix.layout()["cell size"])
    for cells in (2, 5, 20):
        band = cells * h
        key = f"uniform in the cube 200k, band {cells} cells"
        out[key + " query ms"] = timed(lambda: ix.query(cube, max_dist=band))
        out[key + " signed query ms"] = timed(lambda: ix.signed_query(cube, max_dist=band))
        _, face, _, n_eval, n_cells = ix.query(cube, counts=True, max_dist=band)
        out[key + " within"] = float((face >= 0).double().mean())
        out[key + " faces evaluated/query"] = {"mean": float(n_eval.double().mean()), "max": int(n_eval.max())}
        out[key + " cells visited/query"] = {"mean": float(n_cells.double().mean()), "max": int(n_cells.max())}
    res = {}
    out["mesh_sdf_grid 256^3, band 4 voxels, ms"] = timed(lambda: res.update(g=mesh_sdf.mesh_sdf_grid(ix, 256, (-1.0, 1.0),
                                                                                                   band=4 * 2.0 / 255)), max(1, reps // 2))
    out["mesh_sdf_grid 256^3 share within the band"] = float(torch.isfinite(res["g"]).double().mean())


def winding_rows(ix, surf, near, cube, out, reps):
    timed = lambda fn, n=reps: median_ms(fn, n)
    import math
    from nicer_slam_amd import mesh_sdf
    out["winding tree bytes"] = int(M.lib.nsa_tri_winding_workspace(ix.F))

    def build():
        ix._winding = None
        ix._winding_tree()

    out["winding tree build ms"] = timed(build)
    out["winding tree layout"] = ix.winding_layout()
    for name, q in (("on surface 200k", surf), ("near surface (sigma 0.01) 200k", near), ("uniform in the cube 200k", cube)):
        for beta in (2.0, 3.0):
            key = f"{name} winding beta {beta:g}"
            out[key + " ms"] = timed(lambda: ix.winding(q, beta=beta))
            _, acc, ev = ix.winding(q, beta=beta, counts=True)
            out[key + " nodes accepted/query"] = {"mean": float(acc.double().mean()), "max": int(acc.max())}
            out[key + " faces summed/query"] = {"mean": float(ev.double().mean()), "max": int(ev.max())}
        sub = q[:20000].contiguous()
        out[f"{name[:-5]} 20k winding exact ms"] = timed(lambda: ix.winding(sub, beta=math.inf), max(1, reps // 2))
        exact = ix.winding(sub, beta=math.inf)
        for beta in (2.0, 3.0):
            out[f"{name[:-5]} 20k max |w(beta {beta:g}) - w exact|"] = float((ix.winding(sub, beta=beta) - exact).abs().max())
    res = {}
    for sign in ("normal", "winding"):
        out[f"mesh_sdf_grid 256^3, band 4 voxels, sign {sign}, ms"] = timed(
            lambda: res.update({sign: mesh_sdf.mesh_sdf_grid(ix, 256, (-1.0, 1.0), band=4 * 2.0 / 255, sign=sign)}), max(1, reps // 2))
    both = torch.isfinite(res["normal"])
    out["mesh_sdf_grid 256^3 share of band points where the two signs differ"] = float(
        ((res["normal"] < 0) != (res["winding"] < 0))[both].double().mean())


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    reps, timed = a.reps, lambda fn, n=a.reps: median_ms(fn, n)
    finish = lambda out: write_results(out, "mesh_closest_bench.json", a.out)
    out = {"reps": reps, "legs": a.legs}
    g = torch.Generator(device="cuda").manual_seed(0)
    mesh = model_mesh(a.resolution)
    v, f = mesh["verts"], mesh["faces"]
    out["mesh V"], out["mesh F"] = int(v.shape[0]), int(f.shape[0])
    out["index bytes"] = int(M.lib.nsa_tri_workspace(f.shape[0]))
    ix = M.TriIndex(v, f)
    surf, _ = M.sample_surface(v, f, 200000, 0)
    near = surf + 0.01 * torch.randn(surf.shape, device="cuda", generator=g)
    cube = torch.rand(200000, 3, device="cuda", generator=g) * 2 - 1
    if a.legs == "winding":
        winding_rows(ix, surf, near, cube, out, reps)
        return finish(out)
    out["build ms"] = timed(lambda: M.TriIndex(v, f))
    lay = ix.layout()
    out["layout"] = lay
    out["large-list share"] = lay["large faces"] / f.shape[0]
    out["skipped (index, non-finite, zero area)"] = list(ix.skipped)
    query_case("on surface 200k", ix, surf, out, reps)
    query_case("near surface (sigma 0.01) 200k", ix, near, out, reps)
    query_case("uniform in the cube 200k", ix, cube, out, reps)
    sdf_rows(ix, surf, near, cube, out, reps)
    winding_rows(ix, surf, near, cube, out, reps)

    # the torch float64 brute force of the tests, at a size it finishes in a few seconds; the index on the same inputs beside it
    from test_mesh_closest_gpu import _brute_torch
    small = model_mesh(128)
    sv, sf = small["verts"], small["faces"]
    sq = near[:16384].contiguous()
    out["brute force size"] = [int(sq.shape[0]), int(sf.shape[0])]
    res = {}
    out["torch float64 brute force ms"] = timed(lambda: res.update(b=_brute_torch(sq, sv, sf)), 1)
    six = M.TriIndex(sv, sf)
    out["index at the brute-force size: build ms"] = timed(lambda: M.TriIndex(sv, sf))
    out["index at the brute-force size: query ms"] = timed(lambda: six.query(sq))
    d2, face, _ = six.query(sq, squared=True)
    out["index equals the brute force"] = bool(np.array_equal(face.cpu().numpy(), res["b"][0])
                                               and np.array_equal(d2.cpu().numpy(), res["b"][1]))

    import eval_ref as E
    T = E.rigid([0.2, 1.0, -0.4], 2.0, [0.01, -0.005, 0.008])
    src = torch.from_numpy(E.transform(v.cpu().numpy().astype(np.float64), T).astype(np.float32)).cuda()
    moved = {"verts": src, "faces": f}
    for mode in ("samples", "mesh"):
        met = {}
        out[f"mesh_metrics surface={mode} ms"] = timed(lambda: met.update(M.mesh_metrics(moved, mesh, surface=mode)),
                                                       max(1, reps // 2))
        out[f"mesh_metrics surface={mode} accuracy, completion"] = [met["accuracy"], met["completion"]]
    finish(out)


if __name__ == "__main__":
    main()
