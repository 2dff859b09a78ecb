"""Time mesh simplification on the 512^3 mesh of tools/bench_mesh.py's model and on a mesh fused from tools/bench_tsdf.py's
room, at cells of 2, 4 and 8 voxels, and target_faces at F / 10.  Device events, warm-up first, medians; the two entry points are
timed without the wrapper's read-backs as well.  There is no earlier version and no reference program; the only runnable baseline is
the composed route on the same GPU -- torch.unique on the keys, index_add_ for the quadrics, torch.linalg.solve, torch.unique(dim=0) on
the triples -- which is timed beside it (it computes the same vertex and face counts; its sums have no fixed order).  Once per mesh
the downstream effect: the TriIndex build and one render_depth before and after.  Results go to profiles/mesh_simplify_bench.json.
usage: python tools/bench_mesh_simplify.py [reps=5] [resolution=512] [tsdf voxels=256] [tsdf frames=100]"""
import ctypes
import sys

import torch

from benchlib import look_at, median_ms, mesh_positionals, model_mesh, tsdf_mesh, write_results
from nicer_slam_amd import mesh_raycast, mesh_simplify as M
from nicer_slam_amd._native import lib, check
from nicer_slam_amd.mesh_eval import TriIndex


def parse_args(argv):
    return mesh_positionals(argv)


def composed(v, f, origin, h, eps=1e-3):
    """(V', F', verts) by stock torch operators; every face of the bench meshes contributes, which this route assumes"""
    o = torch.tensor(origin, dtype=torch.float64, device=v.device)
    vd, fl = v.double(), f.long()
    c = torch.floor((vd - o) / h).long()
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    used[fl.reshape(-1)] = True
    uniq, inv = torch.unique(key[used], return_inverse=True)
    K = uniq.numel()
    vc = torch.full((v.shape[0],), -1, dtype=torch.long, device=v.device)
    vc[used] = inv
    t = vc[fl]
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])]
    r = t.argmin(1, keepdim=True)
    rot = torch.gather(t, 1, (r + torch.arange(3, device=v.device)) % 3)
    faces = torch.unique(rot, dim=0)
    named = torch.unique(faces)
    cell = torch.stack([uniq >> 42, (uniq >> 21) & (M.GRID - 1), uniq & (M.GRID - 1)], 1)
    centre = o + (cell.double() + 0.5) * h
    members = vc[used]
    p = vd[used] - centre[members]
    mean = torch.zeros(K, 3, dtype=torch.float64, device=v.device).index_add_(0, members, p)
    mean /= torch.bincount(members, minlength=K)[:, None]
    A = torch.zeros(K, 9, dtype=torch.float64, device=v.device)
    b = torch.zeros(K, 3, dtype=torch.float64, device=v.device)
    for j in range(3):
        cl = vc[fl[:, j]]
        ctr = centre[cl]
        p0, p1, p2 = vd[fl[:, 0]] - ctr, vd[fl[:, 1]] - ctr, vd[fl[:, 2]] - ctr
        n = torch.linalg.cross(p1 - p0, p2 - p0)
        d = -(n * p0).sum(1, keepdim=True)
        A.index_add_(0, cl, (n[:, :, None] * n[:, None, :]).reshape(-1, 9))
        b.index_add_(0, cl, n * d)
    A = A.reshape(K, 3, 3)
    tr = A.diagonal(dim1=1, dim2=2).sum(1)
    mu = eps * tr
    ok = tr != 0
    x = mean.clone()
    eye = torch.eye(3, dtype=torch.float64, device=v.device)
    x[ok] = torch.linalg.solve(A[ok] + mu[ok, None, None] * eye, (-b[ok] + mu[ok, None] * mean[ok])[:, :, None])[:, :, 0].clamp(-h / 2, h / 2)
    verts = (centre + x)[named].float()
    return named.numel(), faces.shape[0], verts


def downstream(mesh, reps):
    """ms of a TriIndex build and of one 480 x 640 render_depth from inside the bounding box"""
    v, f = mesh["verts"], mesh["faces"]
    lo, hi = M._extent(v)
    mid = [(a + b) / 2 for a, b in zip(lo, hi)]
    c2w = look_at(mid, [mid[0] + 1.0, mid[1] + 0.3, mid[2] + 0.1])
    K = (400.0, 400.0, 319.5, 239.5)
    return {"TriIndex build ms": median_ms(lambda: TriIndex(v, f), reps),
            "render_depth 480x640 ms (tree build included)": median_ms(
                lambda: mesh_raycast.render_depth(mesh, c2w, K, (480, 640), channels=("depth",)), reps)}


def case(name, mesh, voxel, out, reps):
    timed = lambda fn: median_ms(fn, reps)
    v, f = mesh["verts"].contiguous(), mesh["faces"].contiguous()
    normals, colors = mesh.get("normals"), mesh.get("colors")
    V, F = v.shape[0], f.shape[0]
    r = {"V": V, "F": F, "voxel": voxel, "cells": {}}
    dev = v.device
    lo3, hi3 = M._extent(v)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    t = dict(vertex_cluster=i32(V), cluster_vertex=i32(V), out_cluster=i32(V), faces=i32(F, 3), face_origin=i32(F))
    ws = torch.empty(lib.nsa_mesh_cluster_workspace(V, F), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(lib.nsa_mesh_cluster_place_workspace(V, F), dtype=torch.uint8, device=dev)
    tot = torch.empty(9, dtype=torch.int64, device=dev)
    org = (ctypes.c_double * 3)(*lo3)
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda x: None if x is None else x.data_ptr()
    for k in (2, 4, 8):
        h = k * voxel
        n_cells = M._n_cells(lo3, hi3, h)[1]
        run_cluster = lambda n=n_cells: check(lib.nsa_mesh_cluster(
            v.data_ptr(), V, f.data_ptr(), F, org, h, n, ws.data_ptr(), t["vertex_cluster"].data_ptr(), t["cluster_vertex"].data_ptr(),
            t["out_cluster"].data_ptr(), t["faces"].data_ptr(), t["face_origin"].data_ptr(), tot.data_ptr(), stream))
        c = {"cluster kernels ms": timed(run_cluster), "cluster kernels ms, full 2^21 grid (8 key passes)": timed(lambda: run_cluster(M.GRID))}
        totals = dict(zip(M.TOTALS, (int(x) for x in tot.cpu())))
        c.update(totals)
        n_out = totals["n_verts"]
        ov = torch.empty(n_out, 3, device=dev)
        on = None if normals is None else torch.empty(n_out, 3, device=dev)
        oc = None if colors is None else torch.empty(n_out, 3, device=dev)
        for placement in (1, 0):
            c[f"place kernels ms ({M.PLACEMENTS[placement]})"] = timed(lambda: check(lib.nsa_mesh_cluster_place(
                v.data_ptr(), V, f.data_ptr(), F, ptr(normals), ptr(colors), org, h, 1e-3, placement, t["vertex_cluster"].data_ptr(),
                t["cluster_vertex"].data_ptr(), n_out, ws2.data_ptr(), ov.data_ptr(), ptr(on), ptr(oc), None, stream)))
        members = torch.bincount(t["vertex_cluster"][t["vertex_cluster"] >= 0].long())
        c["member vertices per cluster: median, max"] = [float(members.float().median()), int(members.max())]
        c["simplify() ms"] = timed(lambda: M.simplify(mesh, cell=h))
        c["simplify(placement='mean') ms"] = timed(lambda: M.simplify(mesh, cell=h, placement="mean"))
        n_v, n_f, cv = composed(v, f, lo3, h)
        assert (n_v, n_f) == (totals["n_verts"], totals["n_faces"]), (n_v, n_f, totals)
        got = M.simplify({"verts": v, "faces": f}, cell=h)["verts"]
        c["max |device - composed| / h"] = float((got - cv).abs().max() / h)
        c["composed torch route ms"] = timed(lambda: composed(v, f, lo3, h))
        c["composed / simplify()"] = c["composed torch route ms"] / c["simplify() ms"]
        r["cells"][f"{k} voxels"] = c
    target = F // 10
    r["target_faces"] = {"target": target, "simplify(target_faces=F/10) ms": median_ms(lambda: M.simplify(mesh, target_faces=target), 3)}
    small = M.simplify(mesh, target_faces=target, return_map=True)
    r["target_faces"].update(cell=small["cell"], cell_in_voxels=small["cell"] / voxel, **small["totals"])
    r["downstream before"] = downstream(mesh, reps)
    r["downstream after target_faces"] = downstream({k: small[k] for k in ("verts", "faces")}, reps)
    out[name] = r


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    case(f"model mesh {a.resolution}^3", model_mesh(a.resolution), 2.0 / (a.resolution - 1), out, a.reps)
    case(f"tsdf room {a.voxels}^3, {a.frames} frames", tsdf_mesh(a.voxels, a.frames), 1.44 / a.voxels, out, a.reps)
    write_results(out, "mesh_simplify_bench.json")


if __name__ == "__main__":
    main()
