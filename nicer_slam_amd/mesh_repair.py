"""Mesh repair on the device: cutting a triangle mesh into a 2-manifold, one vertex per fan of faces (C ABI Section 26,
csrc/mesh_manifold.hip), and the inverse plumbing, welding.

* ``vertex_fans(mesh)``: how many fans of faces meet at every vertex, the fans found through regular edges only, and the totals: fans,
  singular vertices, pinch-only vertices, cut edges.
* ``is_manifold(mesh)``: no cut edge and no singular vertex.
* ``split_nonmanifold(mesh)``: the mesh with every vertex duplicated once per fan -- the "cutting" of Gueziec et al.  No edge of the
  result has more than two faces and every vertex has one fan; old vertices and every face keep their place; a new vertex carries the
  bits of its source.  ``cut_inconsistent`` cuts the edges that their two faces traverse the same way as well, ``labels`` the seams
  between labelled patches.
* ``weld(mesh)``: vertices with equal coordinates merged into the smallest index of their class; torch only.
* ``python -m nicer_slam_amd.mesh_repair IN.ply --out OUT.ply [--weld] [--cut-inconsistent] [--list] [--json]``.

Everything is integer work and exact.  numpy in, numpy out; torch in, torch out.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import json
import sys

import numpy as np
import torch

from ._native import lib, check, SPLIT_CUT_INCONSISTENT
from .mesh_args import as_tensor, checked_rows, cuda_faces, need_gpu, ptr, stream, workspace
from .mesh_eval import welded_faces
from .mesh_topology import _edge_table, _mesh_arrays
from .ply import read_ply, write_mesh_ply

TOTALS = ("n_contributing", "n_fans", "n_singular_verts", "n_pinch_only", "n_cut_edges", "n_new", "max_fans")
_ATTRIBUTES = ("verts", "normals", "colors")


def _checked_labels(labels, F, _dev, name):
    if labels is None:
        return None
    lab = as_tensor(labels)
    if lab.dim() != 1 or lab.shape[0] != F:
        raise ValueError(f"{name}: labels must be [F] = [{F}]")
    if lab.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8, torch.bool):
        raise ValueError(f"{name}: labels must be integers")
    if lab.numel() and lab.dtype == torch.int64 and (int(lab.min()) < -2 ** 31 or int(lab.max()) >= 2 ** 31):
        raise ValueError(f"{name}: label outside int32")
    return lab


@torch.no_grad()
def _split_fans(f, V, F, mask, labels, cut_inconsistent):
    """the device arrays of nsa_mesh_split_fans on the topology faces ``f`` and its totals as a dict of ints (two read backs: the edge
    table's totals and these)"""
    dev, H = f.device, 3 * F
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = dict(corner_fan=i32(H), vertex_fans=i32(V), faces=i32(F, 3), new_source=i32(H))
    totals = dict.fromkeys(TOTALS, 0)
    if F == 0:
        out["vertex_fans"].zero_()
        return out, totals
    if V + H >= 1 << 31:
        raise ValueError("split_nonmanifold: n_verts + 3 * n_faces must stay below 2^31")
    t, _ = _edge_table(f, V, F, mask)
    lab = labels.to(dev).to(torch.int32).contiguous() if labels is not None else None
    ws = workspace(lib.nsa_mesh_split_fans_workspace(V, F), dev)
    tot = torch.empty(8, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_split_fans(f.data_ptr(), F, V, ptr(lab),
                                  SPLIT_CUT_INCONSISTENT if cut_inconsistent else 0, t["edges"].data_ptr(), t["edge_count"].data_ptr(),
                                  t["edge_forward"].data_ptr(), t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(),
                                  t["face_edges"].data_ptr(), t["_totals"].data_ptr(), ws.data_ptr(), out["corner_fan"].data_ptr(),
                                  out["vertex_fans"].data_ptr() if V else None, out["faces"].data_ptr(), out["new_source"].data_ptr(),
                                  tot.data_ptr(), stream(dev)))
    host = [int(x) for x in tot.cpu()]
    if host[7] != 0:
        raise RuntimeError(f"split_nonmanifold: the union-find left its loop on a step cap (status {host[7]}); this is a bug")
    totals = dict(zip(TOTALS, host[:7]))
    out["new_source"] = out["new_source"][:totals["n_new"]]
    return out, totals


def split_fans(faces, n_verts, face_mask=None, cut_inconsistent=False, labels=None):
    """Header Section 26 as it stands, on ``faces`` [F, 3] over ``n_verts`` vertices: a dict of ``corner_fan`` [3 F], ``vertex_fans``
    [V], ``faces`` [F, 3], ``new_source`` [n_new] (int32; arrays for numpy faces) and the totals as ints."""
    f, V, F, mask, restore = cuda_faces(faces, n_verts, face_mask, "split_fans")
    lab = _checked_labels(labels, F, f.device, "split_fans")
    out, totals = _split_fans(f, V, F, mask, lab, bool(cut_inconsistent))
    r = {k: restore(x) for k, x in out.items()}
    r.update(totals)
    return r


def vertex_fans(mesh, weld=False, device="cuda"):
    """(fans [V] int32, totals): the number of fans of faces at every vertex of ``mesh`` (a dict with ``verts`` and ``faces``, numpy
    or torch) -- 0 unused, 1 regular, more: singular -- and a dict of ints: ``n_contributing``, ``n_fans``, ``n_singular_verts``,
    ``n_pinch_only`` (singular, with no cut edge incident: sheets that only touch there), ``n_cut_edges`` (edges with more than two
    faces), ``n_new`` (the vertices a split would add) and ``max_fans``.  ``weld=True`` names every vertex by its fp32 coordinates
    (``mesh_eval.welded_faces``) and masks the faces with a non-finite vertex, as ``mesh_topology.topology`` does; the counts are
    then indexed by that name."""
    f, V, F, mask, _, _ = _mesh_arrays(mesh, weld, device, "vertex_fans")
    out, totals = _split_fans(f, V, F, mask, None, False)
    fans = out["vertex_fans"]
    return (fans.cpu().numpy() if not torch.is_tensor(mesh["faces"]) else fans.to(mesh["faces"].device)), totals


def is_manifold(mesh, weld=False, device="cuda"):
    """whether ``mesh`` is a 2-manifold (with boundary) by index: no edge with more than two faces and no vertex with more than one
    fan"""
    _, totals = vertex_fans(mesh, weld, device)
    return totals["n_cut_edges"] == 0 and totals["n_singular_verts"] == 0


def _gather_rows(a, source):
    """``a`` [V, ...] followed by the rows ``source`` names: copies, so a new vertex has the bits of its source"""
    if torch.is_tensor(a):
        return torch.cat([a, a[source.to(a.device).long()]])
    a = np.asarray(a)
    return np.concatenate([a, a[source.cpu().numpy().astype(np.int64)]])


def split_nonmanifold(mesh, cut_inconsistent=False, labels=None, return_report=False, return_map=False, device="cuda"):
    """``mesh`` (a dict with ``verts`` [V, 3] and ``faces`` [F, 3], optionally ``normals`` and ``colors`` [V, ...]; numpy or torch) cut
    into a 2-manifold: a new dict of the same kind in which every vertex is duplicated once per fan of faces around it (header
    Section 26).  The first fan of a vertex keeps it; further fans get new vertices V, V + 1, ... in ascending (vertex, smallest corner
    of the fan) order, whose ``verts``, ``normals`` and ``colors`` are the bits of their source.  Old vertices, the face count and the
    position of every index stay; a face that does not contribute (an index outside [0, V), a repeated index) is copied with every
    index >= V written as -1.  No edge of the result has more than two faces, every vertex has one fan, and splitting the result
    again changes nothing.
    ``cut_inconsistent``: an edge whose two faces traverse it the same way is cut as well.  ``labels`` (integers [F]): an edge
    between faces of different labels is cut, so labelled patches come apart along their seams.
    ``return_report=True`` appends a dict of ints: ``vertex_fans``' totals plus ``n_verts_in`` and ``n_verts_out``;
    ``return_map=True`` adds ``vertex_source`` [V'] (the input vertex each output vertex copies) to the mesh."""
    name = "split_nonmanifold"
    if "verts" in mesh and "faces" in mesh and len(mesh["verts"].shape) == 2 and len(mesh["faces"].shape) == 2:
        checked_rows(mesh, mesh["verts"].shape[0], name)                   # (before the move to the device: no GPU needed to refuse)
        _checked_labels(labels, mesh["faces"].shape[0], None, name)
    f, V, F, _, _, _ = _mesh_arrays(mesh, False, device, name)
    lab = _checked_labels(labels, F, f.device, name)
    out, totals = _split_fans(f, V, F, None, lab, bool(cut_inconsistent))
    was_numpy = not torch.is_tensor(mesh["faces"])
    result = dict(mesh)
    faces = out["faces"]
    if was_numpy:
        result["faces"] = faces.cpu().numpy().astype(np.asarray(mesh["faces"]).dtype)
    else:
        result["faces"] = faces.to(mesh["faces"].device).to(mesh["faces"].dtype)
    source = out["new_source"]
    for k in _ATTRIBUTES:
        if mesh.get(k) is not None:
            result[k] = _gather_rows(mesh[k], source)
    if return_map:
        vs = torch.cat([torch.arange(V, dtype=torch.int32, device=source.device), source])
        result["vertex_source"] = vs.cpu().numpy() if was_numpy else vs.to(mesh["faces"].device)
    report = dict(totals, n_verts_in=V, n_verts_out=V + totals["n_new"])
    return (result, report) if return_report else result


@torch.no_grad()
def weld(mesh, return_report=False, return_map=False):
    """The inverse plumbing of ``split_nonmanifold``: vertices with equal fp32 coordinates (``mesh_eval.welded_faces``' names; -0 = +0; a
    non-finite vertex is merged with nothing) become one -- the smallest index of their class, the representative -- and the
    representatives that a surviving face uses, in ascending order, are the vertices of the result, with the representative's
    ``normals`` and ``colors``.  A face with an index outside [0, V), or with a repeated index after the merge, is dropped and
    counted.  torch only, wherever the mesh lives; numpy in, numpy out.  ``return_report=True`` appends a dict of ints (``n_verts_in``,
    ``n_verts_out``, ``n_faces_in``, ``n_faces_out``, ``n_dropped``); ``return_map=True`` adds ``vertex_source`` [V']."""
    if "verts" not in mesh or "faces" not in mesh:
        raise ValueError("weld: mesh needs 'verts' and 'faces'")
    was_numpy = not torch.is_tensor(mesh["faces"])
    v, f = as_tensor(mesh["verts"]), as_tensor(mesh["faces"])
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("weld: verts must be [V, 3] and faces [F, 3]")
    V, F, dev = v.shape[0], f.shape[0], v.device
    checked_rows(mesh, V, "weld")
    f = f.to(dev).long()
    idx = torch.arange(V, device=dev)
    name = welded_faces(v.detach().float(), idx.to(torch.int32)[:, None].expand(V, 3).contiguous())[:, 0].long() if V else idx
    finite = torch.isfinite(v).all(1) if V else idx.bool()
    name = torch.where(finite, name, V + idx)                                     # (a non-finite vertex: a class of its own)
    rep = torch.full((2 * V + 1,), V, dtype=torch.int64, device=dev).scatter_reduce_(0, name, idx, "amin")[name]
    ok = ((f >= 0) & (f < V)).all(1)
    g = rep[torch.where(ok[:, None], f, torch.zeros_like(f))] if V else f
    keep = ok & (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 2] != g[:, 0])
    g = g[keep]
    used = torch.unique(g)                                                         # ascending representatives
    new = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    new[used] = torch.arange(used.numel(), device=dev)
    faces = new[g].reshape(-1, 3)
    result = dict(mesh)
    if was_numpy:
        result["faces"] = faces.cpu().numpy().astype(np.asarray(mesh["faces"]).dtype)
    else:
        result["faces"] = faces.to(mesh["faces"].device).to(mesh["faces"].dtype)
    for k in _ATTRIBUTES:
        a = mesh.get(k)
        if a is not None:
            result[k] = a[used.to(a.device)] if torch.is_tensor(a) else np.asarray(a)[used.cpu().numpy()]
    if return_map:
        result["vertex_source"] = used.cpu().numpy() if was_numpy else used.to(mesh["faces"].device)
    report = dict(n_verts_in=V, n_verts_out=int(used.numel()), n_faces_in=F, n_faces_out=int(faces.shape[0]),
                  n_dropped=F - int(faces.shape[0]))
    return (result, report) if return_report else result


def format_report(r):
    return [f"faces {r['n_contributing']} contributing, fans {r['n_fans']}, at most {r['max_fans']} at one vertex",
            f"cut edges {r['n_cut_edges']}, singular vertices {r['n_singular_verts']} ({r['n_pinch_only']} of them a pinch only)",
            f"vertices {r['n_verts_in']} -> {r.get('n_verts_out', r['n_verts_in'])} ({r['n_new']} new)"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_repair", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--out", metavar="OUT.ply", help="the PLY file to write (not needed with --list)")
    ap.add_argument("--weld", action="store_true", help="merge vertices with equal coordinates first (mesh_repair.weld)")
    ap.add_argument("--cut-inconsistent", action="store_true", help="cut the edges that their two faces traverse the same way as well")
    ap.add_argument("--list", action="store_true", help="report only: count the fans, write nothing")
    ap.add_argument("--json", action="store_true", help="print the report as one JSON object")
    a = ap.parse_args(argv)
    if a.out is None and not a.list:
        ap.error("--out is required unless --list is given")
    need_gpu("mesh_repair")
    try:
        mesh = read_ply(a.mesh)
        report = {}
        if a.weld:
            mesh, w = weld(mesh, return_report=True)
            report.update(n_welded=w["n_verts_in"] - w["n_verts_out"], n_dropped=w["n_dropped"])
        out, r = split_nonmanifold(mesh, cut_inconsistent=a.cut_inconsistent, return_report=True)
        report.update(r)
        if a.list:
            del report["n_verts_out"]
        else:
            write_mesh_ply(a.out, out)
    except (ValueError, OSError) as e:
        print(f"mesh_repair: {e}", file=sys.stderr)
        raise SystemExit(2)
    report["is_manifold"] = r["n_cut_edges"] == 0 and r["n_singular_verts"] == 0
    if a.json:
        print(json.dumps(report))
    else:
        lines = format_report(report)
        if a.weld:
            lines.insert(0, f"welded {report['n_welded']} vertices away, dropped {report['n_dropped']} faces")
        if a.list:
            lines[-1] = f"vertices {report['n_verts_in']}: a split would add {report['n_new']}"
        print("\n".join(lines + ([] if a.list else [f"-> {a.out}"])))
    return report


if __name__ == "__main__":
    main()
