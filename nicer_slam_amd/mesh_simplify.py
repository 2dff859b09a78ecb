"""Mesh simplification on the device: vertex clustering on a uniform grid with error-quadric placement (C ABI Section 19,
csrc/mesh_simplify.hip).

* ``simplify(mesh, cell=H)``: every grid cell of edge H keeps one vertex, placed where the planes of the faces around the cell meet
  (Lindstrom's quadric, pulled towards the mean of the cell's vertices instead of truncated, clamped to the cell), or at that mean
  (``placement="mean"``); faces that lose a corner to a neighbour's cell go, repeated faces go, normals and colours are averaged.
* ``simplify(mesh, target_faces=N)``: the cell size comes from a geometric bisection on the face count, which needs the integer half
  of the work only.
* ``cluster(faces, verts, cell, origin)``: that integer half on its own -- which vertex joins which cluster, which faces survive.
* ``python -m nicer_slam_amd.mesh_simplify IN.ply --out OUT.ply (--cell H | --faces N) [--placement mean|quadric] [--json]``.

The result is a function of the input alone and bit-reproducible.  numpy in, numpy out; torch in, torch out on the caller's device.
There is no CPU path: a missing GPU is an error.
"""
import argparse
import ctypes
import json
import math
import sys

import numpy as np
import torch

from ._native import lib, check
from .mesh_args import checked_mesh, need_gpu, ptr, stream, workspace
from .mesh_repair import split_nonmanifold
from .ply import read_ply, write_mesh_ply

TOTALS = ("n_clusters", "n_contributing", "n_used", "n_outside", "n_collapsed", "n_duplicate", "n_verts", "n_faces")
PLACEMENTS = ("mean", "quadric")
GRID = 1 << 21


def _extent(v):
    """(lo, hi) float64 lists of the finite vertices (zeros when there is none): one read back"""
    if v.shape[0] == 0:
        return [0.0] * 3, [0.0] * 3
    fin = torch.isfinite(v).all(1, keepdim=True)
    inf = torch.full_like(v, float("inf"))
    both = torch.stack([torch.where(fin, v, inf).amin(0), torch.where(fin, v, -inf).amax(0)]).double().cpu()
    if not bool(torch.isfinite(both).all()):
        return [0.0] * 3, [0.0] * 3
    return both[0].tolist(), both[1].tolist()


def _checked_cell(cell, name):
    h = float(cell)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError(f"{name}: cell must be finite and positive")
    return h


def _checked_origin(origin, name):
    o = [float(x) for x in (origin.tolist() if hasattr(origin, "tolist") else origin)]
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise ValueError(f"{name}: origin must be three finite numbers")
    return o


@torch.no_grad()
def _cluster(v, f, origin, h, n_cells=GRID):
    """the device arrays of nsa_mesh_cluster and the totals as a dict of ints (one read back: a synchronisation)"""
    dev, V, F = v.device, v.shape[0], f.shape[0]
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    t = dict(vertex_cluster=i32(V), cluster_vertex=i32(V), out_cluster=i32(V), faces=i32(F, 3), face_origin=i32(F))
    totals = dict.fromkeys(TOTALS, 0)
    if V == 0 or F == 0:
        t["vertex_cluster"].fill_(-1)
        t["cluster_vertex"].fill_(-1)
        return t, totals
    ws = workspace(lib.nsa_mesh_cluster_workspace(V, F), dev)
    tot = torch.empty(9, dtype=torch.int64, device=dev)
    org = (ctypes.c_double * 3)(*origin)
    check(lib.nsa_mesh_cluster(v.data_ptr(), V, f.data_ptr(), F, org, h, int(n_cells), ws.data_ptr(), t["vertex_cluster"].data_ptr(),
                               t["cluster_vertex"].data_ptr(), t["out_cluster"].data_ptr(), t["faces"].data_ptr(),
                               t["face_origin"].data_ptr(), tot.data_ptr(), stream(dev)))
    host = [int(x) for x in tot.cpu()]
    if host[8] != 0:
        raise RuntimeError(f"mesh_simplify: a sort order left its range (status {host[8]}); this is a bug")
    return t, dict(zip(TOTALS, host[:8]))


@torch.no_grad()
def _place(v, f, normals, colors, origin, h, eps, placement, t, n_out):
    dev, V, F = v.device, v.shape[0], f.shape[0]
    out = dict(verts=torch.empty(n_out, 3, device=dev), vertex_cell=torch.empty(n_out, 3, dtype=torch.int32, device=dev))
    if normals is not None:
        out["normals"] = torch.empty(n_out, 3, device=dev)
    if colors is not None:
        out["colors"] = torch.empty(n_out, 3, device=dev)
    if n_out == 0:
        return out
    ws = workspace(lib.nsa_mesh_cluster_place_workspace(V, F), dev)
    org = (ctypes.c_double * 3)(*origin)
    check(lib.nsa_mesh_cluster_place(v.data_ptr(), V, f.data_ptr(), F, ptr(normals), ptr(colors), org, h, float(eps),
                                     PLACEMENTS.index(placement), t["vertex_cluster"].data_ptr(), t["cluster_vertex"].data_ptr(), n_out,
                                     ws.data_ptr(), out["verts"].data_ptr(), ptr(out.get("normals")), ptr(out.get("colors")),
                                     out["vertex_cell"].data_ptr(), stream(dev)))
    return out


def cluster(faces, verts, cell, origin=None):
    """The combinatorial half of ``simplify`` (header Section 19, nsa_mesh_cluster) as a dict: ``vertex_cluster`` [V] int32 (the
    cluster of every vertex in ascending cell-key order, -1 for a vertex no contributing face names), ``faces`` [F', 3] int32 over the
    output vertices, ``face_origin`` [F'] int32 (strictly ascending), ``out_cluster`` [V'] int32 (the cluster of each output vertex),
    and the totals as ints: ``n_clusters``, ``n_contributing``, ``n_used``, ``n_outside``, ``n_collapsed``, ``n_duplicate``,
    ``n_verts``, ``n_faces``.  ``origin`` defaults to the per-axis minimum of the finite vertices; a vertex whose cell index falls
    outside [0, 2^21) on an axis is outside the grid and its faces do not contribute.  Reads the totals back once."""
    h = _checked_cell(cell, "cluster")
    if origin is not None:
        origin = _checked_origin(origin, "cluster")
    v, f, _, _, _, restore = checked_mesh({"verts": verts, "faces": faces}, "cluster", float_verts=True)
    o = _extent(v)[0] if origin is None else origin
    t, totals = _cluster(v, f, o, h)
    out = dict(vertex_cluster=restore(t["vertex_cluster"]), faces=restore(t["faces"][:totals["n_faces"]]),
               face_origin=restore(t["face_origin"][:totals["n_faces"]]), out_cluster=restore(t["out_cluster"][:totals["n_verts"]]))
    out.update(totals)
    return out


def _n_cells(origin, hi3, h):
    """(the grid's width in cells on its widest axis, a cell count per axis above every cell index: it only shortens the sorts)"""
    widest = max((hi3[k] - origin[k]) / h for k in range(3))
    return widest, (min(GRID, max(1, int(math.floor(max(widest, 0.0))) + 1)) if widest < GRID else GRID)


def _search(v, f, origin, lo3, hi3, target):
    """the cell size for ``target`` faces: hi = the bounding-box diagonal (no face survives), lo = hi / 2^20, 24 probes of sqrt(lo hi);
    hi moves down when the count is <= target, else lo moves up; the final hi.  The count is not monotone in the cell size: this
    rule is the definition."""
    dx, dy, dz = (hi3[k] - lo3[k] for k in range(3))
    hi = math.sqrt((dx * dx + dy * dy) + dz * dz)
    if not (math.isfinite(hi) and hi > 0.0):
        raise ValueError("simplify: target_faces needs a mesh with a finite, non-zero extent")
    lo = hi / 2.0 ** 20
    for _ in range(24):
        mid = math.sqrt(lo * hi)
        if _cluster(v, f, origin, mid, _n_cells(origin, hi3, mid)[1])[1]["n_faces"] <= target:
            hi = mid
        else:
            lo = mid
    return hi


def simplify(mesh, cell=None, target_faces=None, placement="quadric", origin=None, eps=1e-3, return_map=False, split=None):
    """Simplify ``mesh`` (a dict with ``verts`` [V, 3] and ``faces`` [F, 3], optionally ``normals`` and ``colors`` [V, 3]; numpy or
    torch) by vertex clustering (header Section 19): the same kind of dict with one vertex per occupied grid cell that a surviving
    face names, for ``write_ply``, ``TriIndex``, ``mesh_clean`` and ``mesh_topology`` as it is.

    Exactly one of ``cell`` (the grid's edge length) and ``target_faces`` (the largest face count not above it that a 24-step
    geometric bisection on the cell size finds) must be given.  ``placement``: "quadric" (the minimiser of the squared-area weighted
    plane distances of the faces around the cell, regularised towards the cell's mean vertex with weight ``eps`` times the
    quadric's trace, clamped to the cell) or "mean".  ``origin`` (three numbers) anchors the grid; default: the per-axis minimum of
    the finite vertices.  A grid wider than 2^21 cells on an axis is a ValueError.  A face with a non-finite vertex or an index
    outside [0, V) is dropped.  A sheet that collapses to zero thickness keeps its two sides (a triple and its reverse are different
    faces).  ``return_map=True`` adds ``vertex_cluster`` [V] (the cluster of each input vertex, -1 if unused), ``face_origin`` [F']
    (the input face of each output face), ``vertex_cell`` [V', 3], ``totals`` (a dict of ints) and ``cell`` (the cell size used).
    ``split``: None (default) leaves the result as clustering made it -- sheets closer than a cell merge, so it may have edges with
    more than two faces --; True or a dict of ``mesh_repair.split_nonmanifold`` keywords cuts it into a 2-manifold: the
    faces keep their place, the new vertices follow the clusters' (with ``return_map``, ``vertex_source`` [V''] names the cluster
    vertex each one copies and ``vertex_cell`` has their rows too).

    Synchronises for the extent of the vertices and once for the totals (``target_faces``: once per probe as well)."""
    name = "simplify"
    if (cell is None) == (target_faces is None):
        raise ValueError("simplify: give exactly one of cell and target_faces")
    if placement not in PLACEMENTS:
        raise ValueError(f"simplify: placement must be one of {PLACEMENTS}")
    eps = float(eps)
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError("simplify: eps must be finite and >= 0")
    if split is not None and not isinstance(split, (bool, dict)):
        raise ValueError("simplify: split must be None, a bool or a dict of mesh_repair.split_nonmanifold keywords")
    if cell is not None:
        h = _checked_cell(cell, name)
    elif int(target_faces) != target_faces or target_faces < 0:
        raise ValueError("simplify: target_faces must be a non-negative integer")
    if origin is not None:
        origin = _checked_origin(origin, name)
    v, f, _, _, extra, restore = checked_mesh(mesh, name, float_verts=True, attributes=("normals", "colors"), float_attributes=True)
    normals, colors = extra.get("normals"), extra.get("colors")
    lo3, hi3 = _extent(v)
    o = lo3 if origin is None else origin
    if cell is None:
        h = _search(v, f, o, lo3, hi3, int(target_faces))
    widest, n_cells = _n_cells(o, hi3, h)
    if not widest < GRID:
        raise ValueError(f"simplify: the grid would be {widest:.3g} cells wide; at most 2^21 per axis")
    t, totals = _cluster(v, f, o, h, n_cells)
    p = _place(v, f, normals, colors, o, h, eps, placement, t, totals["n_verts"])
    out = dict(verts=restore(p["verts"]), faces=restore(t["faces"][:totals["n_faces"]]))
    for k in ("normals", "colors"):
        if k in p:
            out[k] = restore(p[k])
    if return_map:
        out.update(vertex_cluster=restore(t["vertex_cluster"]), face_origin=restore(t["face_origin"][:totals["n_faces"]]),
                   vertex_cell=restore(p["vertex_cell"]), totals=totals, cell=h)
    if split:
        out = split_nonmanifold(out, **dict(split if isinstance(split, dict) else {}, return_report=False, return_map=return_map))
        if return_map:
            src = out["vertex_source"]
            out["vertex_cell"] = out["vertex_cell"][src.long() if torch.is_tensor(src) else src.astype(np.int64)]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_simplify", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--out", required=True, help="the PLY file to write")
    size = ap.add_mutually_exclusive_group(required=True)
    size.add_argument("--cell", type=float, help="edge length of the grid's cells")
    size.add_argument("--faces", type=int, help="target face count: the largest count not above it that the bisection finds")
    ap.add_argument("--placement", choices=PLACEMENTS, default="quadric")
    ap.add_argument("--json", action="store_true", help="print the totals as one JSON object")
    a = ap.parse_args(argv)
    need_gpu("mesh_simplify")
    try:
        r = simplify(read_ply(a.mesh), cell=a.cell, target_faces=a.faces, placement=a.placement, return_map=True)
    except (ValueError, OSError) as e:
        print(f"mesh_simplify: {e}", file=sys.stderr)
        raise SystemExit(2)
    write_mesh_ply(a.out, r)
    report = dict(r["totals"], cell=r["cell"])
    if a.json:
        print(json.dumps(report))
    else:
        print(f"cell {report['cell']:.6g}: {report['n_clusters']} clusters; faces {report['n_contributing']} contributing, "
              f"{report['n_collapsed']} collapsed, {report['n_duplicate']} duplicate -> {report['n_faces']} faces, "
              f"{report['n_verts']} vertices ({report['n_outside']} vertices outside the grid)")
    return report


if __name__ == "__main__":
    main()
