"""Hole filling on the device: boundary loops traced, ranked and patched (C ABI Section 23, csrc/mesh_fill.hip).

* ``fill_holes(mesh, max_edges=None, max_size=None, rings="auto", ...)``: the mesh with every hole that passes the limits closed by a
  polar patch -- rings of the loop shrunk towards its centroid, then a fan to the centre -- oriented like the faces around it.  Old
  vertices and faces keep their indices and bits; the new ones are appended.
* ``boundary_loops(mesh)``: the ordered vertex loops of the boundary, which ``mesh_topology.boundary_edges`` cannot give.
* ``python -m nicer_slam_amd.mesh_fill IN.ply --out OUT.ply [--max-edges N] [--max-size D] [--rings auto|K] [--fair N]
  [--keep-folded] [--method polar|min_area|auto] [--max-area-edges N] [--min-sin S] [--normals keep|angle|area|none] [--weld]
  [--list] [--json]``

A loop is a cycle of the successor relation "rotate about the end vertex inside the fan of faces to the next boundary half-edge"; no
atomics, float64 with every operation rounded on its own, and the result equals the numpy statement in tests/fill_ref.py bit for bit.
Two holes that touch in a vertex are one figure-eight loop (``pinched``), a boundary that runs into a non-manifold or inconsistent edge
is an open chain, a loop that is not star-shaped about its centroid is ``folded``: none of them gets a polar patch.  ``method="auto"``
gives the folded loops a minimum-area patch instead (header Section 24, csrc/mesh_fill_area.hip): no new vertex, n - 2
faces chosen by an interval dynamic programme, equal to tests/fill_area_ref.py bit for bit.  Filling is BY INDEX unless ``weld=True``.

numpy in, numpy out; torch in, torch out on the caller's device.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import json
import math
import sys

import torch

from . import _native
from ._native import lib, check
from .mesh_args import MAX_FACES_RINGS, as_tensor, checked_mesh, need_gpu, ptr, stream, workspace
from .mesh_eval import TriIndex
from .mesh_smooth import WEIGHTING, _vertex_normals, smooth
from .mesh_topology import _edge_table, _mesh_arrays
from .ply import read_ply, write_mesh_ply

CLASSES = _native.FILL_CLASSES
TOTALS = ("n_boundary", "n_loops", "n_filled", "n_nonfinite", "n_pinched", "n_too_many_edges", "n_too_large", "n_folded",
          "n_open_chain", "n_new_verts", "n_new_faces", "status")
INT_COLS = ("leader", "n", "start", "class", "rings", "new_verts", "new_faces", "vert_offset", "face_offset")
REAL_COLS = (("centre", 0, 3), ("color", 3, 6), ("box_lo", 6, 9), ("box_hi", 9, 12), ("size2", 12, 13), ("radius2", 13, 14),
             ("edge2", 14, 15), ("area_normal", 15, 18))
FLAG_BLOCKED, FLAG_PINCHED, FLAG_OPEN_CHAIN = 1, 2, 4
NORMALS = ("keep", "angle", "area", "none", None)
METHODS = ("polar", "min_area", "auto")
AREA_CLASSES = _native.FILL_AREA_CLASSES
AREA_TOTALS = ("n_selected", "n_area_filled", "n_area_too_many_edges", "n_no_triangulation", "n_area_faces", "n_cells", "max_n")
AREA_INT_COLS = ("class", "n", "table_offset", "plan_face_offset", "row_offset", "face_offset")
_MAX_AREA_EDGES = 16384
_MAX_RINGS = 65535


def _checked_args(max_edges, max_size, rings, max_rings, fair, lam, normals, method="polar", max_area_edges=2048, min_sin=1e-6,
                  skip_folded=True):
    """(rings as the C entry takes it: 0 for "auto")"""
    if method not in METHODS:
        raise ValueError(f"fill_holes: method must be one of {METHODS}, got {method!r}")
    if method == "auto" and not skip_folded:
        raise ValueError("fill_holes: method='auto' patches the loops that skip_folded=True leaves out; it needs skip_folded=True")
    if isinstance(max_area_edges, bool) or int(max_area_edges) != max_area_edges or not 1 <= max_area_edges <= _MAX_AREA_EDGES:
        raise ValueError(f"fill_holes: 1 <= max_area_edges <= {_MAX_AREA_EDGES}")
    if not (math.isfinite(float(min_sin)) and float(min_sin) >= 0.0):
        raise ValueError("fill_holes: min_sin must be finite and >= 0")
    if max_edges is not None and (isinstance(max_edges, bool) or int(max_edges) != max_edges or max_edges < 0):
        raise ValueError("fill_holes: max_edges must be a non-negative integer")
    if max_size is not None and not (math.isfinite(float(max_size)) and float(max_size) >= 0.0):
        raise ValueError("fill_holes: max_size must be finite and >= 0")
    if isinstance(max_rings, bool) or int(max_rings) != max_rings or not 1 <= max_rings <= _MAX_RINGS:
        raise ValueError(f"fill_holes: 1 <= max_rings <= {_MAX_RINGS}")
    if rings != "auto" and (isinstance(rings, (bool, str)) or int(rings) != rings or not 1 <= rings <= _MAX_RINGS):
        raise ValueError(f"fill_holes: rings must be 'auto' or an integer in [1, {_MAX_RINGS}]")
    if isinstance(fair, bool) or int(fair) != fair or fair < 0 or fair >= 1 << 30:
        raise ValueError("fill_holes: fair must be a count")
    if not 0.0 < float(lam) <= 1.0:
        raise ValueError("fill_holes: 0 < lam <= 1")
    if normals not in NORMALS:
        raise ValueError(f"fill_holes: normals must be one of {NORMALS}, got {normals!r}")
    return 0 if rings == "auto" else int(rings)


@torch.no_grad()
def _loops(v, f, names, mask, colors, V, F, max_edges, max_size, rings, max_rings, skip_folded):
    """nsa_mesh_fill_loops on device arrays: a dict of the item arrays [B], ``ints`` [L, 9], ``reals`` [L, 18], the device copies the
    emit call reads, and ``totals`` (ints).  Reads Section 18's totals back once, to size the B-long buffers and the round count, and
    the twelve totals of Section 23 once (two synchronisations)."""
    dev = v.device
    t, et = _edge_table(f if names is None else names, V, F, mask)
    B = et["n_boundary"]
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    r = dict(B=B, halfedges=i32(B), next=i32(B), flags=torch.empty(B, dtype=torch.uint8, device=dev), leader=i32(B), rank=i32(B),
             order=i32(B), ints=torch.zeros(B, len(INT_COLS), dtype=torch.int64, device=dev),
             reals=torch.zeros(B, 18, dtype=torch.float64, device=dev), totals=dict.fromkeys(TOTALS, 0))
    r["_ints"], r["_reals"], r["_order"], r["_edge"] = r["ints"], r["reals"], r["order"], t
    if F == 0 or B == 0:
        return r
    ws = workspace(lib.nsa_mesh_fill_workspace(F, B), dev)
    tot = torch.zeros(len(TOTALS), dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_fill_loops(v.data_ptr(), ptr(colors), V, f.data_ptr(), ptr(names), F, t["edge_count"].data_ptr(),
                                  t["edge_forward"].data_ptr(), t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(),
                                  t["face_edges"].data_ptr(), t["_totals"].data_ptr(), B, int(max_edges is not None), int(max_edges or 0),
                                  int(max_size is not None), 0.0 if max_size is None else float(max_size) * float(max_size), rings,
                                  int(max_rings), int(bool(skip_folded)), ws.data_ptr(), r["halfedges"].data_ptr(), r["next"].data_ptr(),
                                  r["flags"].data_ptr(), r["leader"].data_ptr(), r["rank"].data_ptr(), r["order"].data_ptr(),
                                  r["ints"].data_ptr(), r["reals"].data_ptr(), tot.data_ptr(), stream(dev)))
    r["_totals"] = tot
    host = dict(zip(TOTALS, (int(x) for x in tot.cpu())))
    if host["status"] != 0:
        raise RuntimeError(f"fill_holes: the loop tracing reported status {host['status']} (1: a rotation hit its step cap, 2: the "
                           "boundary half-edges do not add up to the edge table's count); this is a bug")
    L = host["n_loops"]
    r.update(totals=host, ints=r["ints"][:L], reals=r["reals"][:L], order=r["order"][:B - host["n_open_chain"]])
    return r


@torch.no_grad()
def _emit(v, f, colors, V, F, r):
    """nsa_mesh_fill_emit: (verts [V + NV, 3], colours or None, faces [F + NF, 3]) with the input as their prefix"""
    dev, NV, NF = v.device, r["totals"]["n_new_verts"], r["totals"]["n_new_faces"]
    if V + NV >= 1 << 31 or 3 * (F + NF) >= 1 << 31:
        raise ValueError("fill_holes: the filled mesh leaves the index range (n_verts < 2^31, 3 * n_faces < 2^31)")
    out_v = torch.cat([v, torch.zeros(NV, 3, dtype=torch.float32, device=dev)])
    out_c = None if colors is None else torch.cat([colors, torch.zeros(NV, 3, dtype=torch.float32, device=dev)])
    out_f = torch.cat([f, torch.full((NF, 3), -1, dtype=torch.int32, device=dev)])
    if NF:
        check(lib.nsa_mesh_fill_emit(v.data_ptr(), ptr(colors), V, f.data_ptr(), F,
                                     r["_order"].data_ptr(), r["B"], r["_ints"].data_ptr(), r["_reals"].data_ptr(),
                                     r["_totals"].data_ptr(), NV, NF, out_v[V:].data_ptr(),
                                     None if out_c is None else out_c[V:].data_ptr(), out_f[F:].data_ptr(), stream(dev)))
    return out_v, out_c, out_f


def _up256(x):
    return (x + 255) // 256 * 256


@torch.no_grad()
def _area(v, f, names, V, F, r, class_mask, max_area_edges, min_sin, tables=False):
    """Section 24 on the loops of ``_loops``: a dict of ``ints`` [L, 6] (AREA_INT_COLS), ``area`` [L], ``faces`` [n_area_faces, 3]
    int32 in the final numbering (the rows of loops without a triangulation dropped) and ``totals``; with ``tables`` also the views
    ``W``, ``J`` and ``mask`` [n_cells] of the workspace.  Reads the plan's totals back once, to size the tables, and the final
    totals once (two synchronisations); a call without a tabled loop stops after the first."""
    dev, B, L = v.device, r["B"], r["totals"]["n_loops"]
    ints = torch.zeros(B, len(AREA_INT_COLS), dtype=torch.int64, device=dev)
    ints[:, 0] = -1
    out = dict(ints=ints[:L], area=torch.zeros(L, dtype=torch.float64, device=dev), faces=torch.zeros(0, 3, dtype=torch.int32, device=dev),
               totals=dict.fromkeys(AREA_TOTALS, 0))
    if F == 0 or B == 0 or L == 0:
        return out
    plan = torch.zeros(8, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_fill_area_plan(r["_ints"].data_ptr(), r["_totals"].data_ptr(), F, B, class_mask, int(max_area_edges),
                                      ints.data_ptr(), plan.data_ptr(), stream(dev)))
    selected, tabled, too_many, cells, max_n, plan_faces, rows, _ = (int(x) for x in plan.cpu())
    out["totals"].update(n_selected=selected, n_area_too_many_edges=too_many, n_no_triangulation=selected - tabled - too_many,
                         n_cells=cells, max_n=max_n)
    if tabled == 0:
        return out
    ws = workspace(lib.nsa_mesh_fill_area_workspace(cells, rows), dev)
    area = torch.zeros(B, dtype=torch.float64, device=dev)
    faces = torch.full((plan_faces, 3), -1, dtype=torch.int32, device=dev)
    final = torch.zeros(4, dtype=torch.int64, device=dev)
    t = r["_edge"]
    check(lib.nsa_mesh_fill_area_tables(v.data_ptr(), V, f.data_ptr(), ptr(names), F,
                                        t["edges"].data_ptr(), t["_totals"].data_ptr(), r["_order"].data_ptr(), B, r["_ints"].data_ptr(),
                                        r["_totals"].data_ptr(), ints.data_ptr(), cells, rows, max_n, plan_faces,
                                        float(min_sin) * float(min_sin), ws.data_ptr(), area.data_ptr(), faces.data_ptr(),
                                        final.data_ptr(), stream(dev)))
    filled, too_many, no_tri, n_faces = (int(x) for x in final.cpu())
    if no_tri:                                               # (their rows are -1; dropping them gives the final numbering)
        faces = faces[faces[:, 0] >= 0].contiguous()
    assert faces.shape[0] == n_faces
    out["totals"].update(n_area_filled=filled, n_no_triangulation=no_tri, n_area_faces=n_faces)
    out.update(area=area[:L], faces=faces)
    if tables:
        o1, o2 = _up256(8 * cells), 2 * _up256(8 * cells) + _up256(24 * rows)
        o3 = o2 + _up256(4 * cells) + 2 * _up256(4 * rows)
        out.update(W=ws[:8 * cells].view(torch.float64), J=ws[o2:o2 + 4 * cells].view(torch.int32), mask=ws[o3:o3 + cells],
                   WT=ws[o1:o1 + 8 * cells].view(torch.float64))
    return out


def _arrays(mesh, name, weld, device):
    """(verts, faces, names or None, mask or None, colours or None, V, F, give)"""
    v, f, V, F, extra, give = checked_mesh(mesh, name, device, float_verts=True, attributes=("colors",), max_faces=MAX_FACES_RINGS)
    colors = extra.get("colors")
    names = mask = None
    if weld and F and V:
        names, _, _, mask, _, _ = _mesh_arrays({"verts": v, "faces": f}, True, v.device, name)
    return v, f, names, mask, colors, V, F, give


def _report(r, give, V, NV):
    out = {k: give(r[k]) for k in ("halfedges", "next", "flags", "rank", "order", "ints", "reals")}
    out["item_leader"] = give(r["leader"])
    ints = r["ints"].cpu()
    out.update({k: ints[:, i].tolist() for i, k in enumerate(INT_COLS)})
    out["class"] = [CLASSES[c] for c in out["class"]]
    out.update({k: give(r["reals"][:, a:b].reshape(-1) if b - a == 1 else r["reals"][:, a:b]) for k, a, b in REAL_COLS})
    out["totals"] = dict(r["totals"])
    mask = torch.zeros(V + NV, dtype=torch.bool, device=r["ints"].device)
    mask[V:] = True
    out["new_vertex"] = give(mask)
    return out


def _area_report(out, r, a, give, method):
    """the keys that ``method != "polar"`` adds to the report"""
    ints = a["ints"].cpu()
    cls, n = ints[:, 0].tolist(), ints[:, 1].tolist()
    polar = [method == "auto" and c == 0 for c in r["ints"][:, 3].tolist()]
    out["method"] = ["min_area" if c >= 0 else "polar" if p else None for c, p in zip(cls, polar)]
    out["area_class"] = [AREA_CLASSES[c] if c >= 0 else None for c in cls]
    out["area"] = give(a["area"])
    out["area_faces"] = [k - 2 if c == 0 else 0 for c, k in zip(cls, n)]
    out["area_face_offset"] = ints[:, 5].tolist()
    out["area_ints"] = give(a["ints"])
    out["area_totals"] = dict(a["totals"])
    return out


def _patch_intersections(out_v, out_f, F, rep, method):
    """per loop: the proper pairs of the filled mesh with exactly one face in the loop's patch"""
    L, FT = len(rep["n"]), out_f.shape[0]
    if FT == 0 or out_v.shape[0] == 0:
        return [0] * L
    label = torch.full((FT,), -1, dtype=torch.int64, device=out_f.device)
    n_polar = 0 if method == "min_area" else sum(rep["new_faces"])
    for l in range(L):
        if method != "min_area" and rep["new_faces"][l]:
            a = F + rep["face_offset"][l]
            label[a:a + rep["new_faces"][l]] = l
        if method != "polar" and rep["area_faces"][l]:
            a = F + n_polar + rep["area_face_offset"][l]
            label[a:a + rep["area_faces"][l]] = l
    pairs, _, _ = TriIndex(out_v.contiguous(), out_f.contiguous()).self_intersections(kinds=("proper",), between=None)
    la, lb = label[pairs[:, 0]], label[pairs[:, 1]]
    apart = la != lb
    hits = torch.cat([la[apart], lb[apart]])
    return torch.bincount(hits[hits >= 0], minlength=L).tolist()


def fill_holes(mesh, max_edges=None, max_size=None, rings="auto", max_rings=64, skip_folded=True, fair=0, lam=0.5, normals="keep",
               weld=False, return_report=False, device="cuda", method="polar", max_area_edges=2048, min_sin=1e-6, intersections=None):
    """``mesh`` (a dict with ``verts`` [V, 3] and ``faces`` [F, 3], optionally ``colors`` and ``normals`` [V, 3]; numpy or torch) with
    its holes filled (header Section 23): a new dict of the same kind; the input's vertices and faces are a prefix of the result's.
      max_edges     fill only loops of at most this many edges (``too_many_edges`` otherwise); None: no limit.
      max_size      fill only loops whose bounding-box diagonal is at most this length (``too_large``); None: no limit.
      rings         "auto": the patch of a loop of n edges has K rings of n vertices, K the smallest with K^2 * (mean squared edge
                    length) >= mean squared distance to the centroid, at most ``max_rings``; an integer forces K.
      skip_folded   leave out a loop that is not star-shaped about its centroid (some fan triangle faces against the others).
      fair          N > 0: ``mesh_smooth.smooth(method="laplacian", iterations=N, lam=lam)`` with every old vertex fixed, which
                    relaxes the patches alone.
      normals       "keep": the stored normals of the old vertices stay and the new vertices get angle-weighted ones (nothing when
                    the mesh stores none); "angle" / "area": ``mesh_smooth.vertex_normals`` of the result; "none" or None: none.
      method        "polar": the patches above alone.  "auto": the loops classed ``filled`` get their polar patch, the loops classed
                    ``folded`` a minimum-area patch (header Section 24); needs ``skip_folded=True``.  "min_area": every loop classed
                    ``filled`` or ``folded`` gets a minimum-area patch and no polar patch is made (the Section 23 columns of the
                    report then say what the polar patches would have been).  A minimum-area patch of a loop of n edges adds no
                    vertex and n - 2 faces, named like the boundary half-edges name their vertices, after the polar faces of the
                    call, in loop order; no chord of it is an edge the mesh already has; ``fair``, ``rings`` and the colour
                    interpolation do not touch it.  The limits above apply first.
      max_area_edges  a selected loop of more edges is ``area_too_many_edges`` and stays open (its table has n^2 cells); <= 16384.
      min_sin       a triangle whose squared area is not above (min_sin * longest edge^2)^2 / 4 is never chosen, so a collinear run
                    of boundary vertices gets no zero-area faces; a loop that cannot be triangulated without one, or without a
                    chord the mesh already has, is ``no_triangulation`` and stays open.
      weld          trace the loops on ``mesh_eval.welded_faces`` names, so that seams of repeated vertices are no boundary; the
                    patch names the duplicate its boundary half-edge names.
      intersections None, or "report" (with ``return_report=True``): the report gains ``proper_pairs``, per loop the number of
                    pairs of faces that meet properly (``mesh_intersect``, header Section 25) with one face in that loop's patch and
                    the other anywhere else in the result, old or new.  The mesh is not changed by it.
    Colours of new vertices are interpolated like their positions, between the loop's vertices and its mean colour.
    ``return_report=True`` appends a dict: per loop (ascending smallest half-edge) ``leader``, ``n``, ``start``, ``class``, ``rings``,
    ``new_verts``, ``new_faces``, ``vert_offset``, ``face_offset``, ``centre``, ``color``, ``box_lo``, ``box_hi``, ``size2``,
    ``radius2``, ``edge2``, ``area_normal`` (and the same as ``ints`` [L, 9] / ``reals`` [L, 18]); per boundary half-edge
    ``halfedges``, ``next``, ``flags`` (1 blocked | 2 pinched | 4 open chain), ``item_leader``, ``rank``, and ``order``; ``totals``;
    and the ``new_vertex`` mask.  With ``method != "polar"`` also per loop ``method`` ("polar", "min_area" or None), ``area_class``
    (``area_filled``, ``area_too_many_edges``, ``no_triangulation`` or None), ``area`` (the patch area W[0][n-1]), ``area_faces``,
    ``area_face_offset``, the same as ``area_ints`` [L, 6], and ``area_totals``.  Not built: dihedral-angle weights (Liepa),
    advancing-front triangulations, refinement of a patch to the surrounding edge density, fairing of patches without interior
    vertices, curvature-continuing fairing, the repair of a patch that ``intersections="report"`` finds crossing the mesh.  Reads the edge table's
    totals back once, to size the buffers of the B boundary half-edges and the round count, and this unit's twelve totals once (two
    synchronisations); Section 24 adds two more, the plan's totals and the final ones."""
    k_rings = _checked_args(max_edges, max_size, rings, max_rings, fair, lam, normals, method, max_area_edges, min_sin, skip_folded)
    if intersections not in (None, "report") or (intersections and not return_report):
        raise ValueError("fill_holes: intersections must be None or 'report', and 'report' needs return_report=True")
    v, f, names, mask, colors, V, F, give = _arrays(mesh, "fill_holes", weld, device)
    stored = mesh.get("normals")
    if normals == "keep" and stored is not None and tuple(stored.shape) != (V, 3):
        raise ValueError("fill_holes: normals must be [V, 3]")
    r = _loops(v, f, names, mask, colors, V, F, max_edges, max_size, k_rings, max_rings, skip_folded)
    if method == "min_area":
        out_v, out_c, out_f = v.clone(), None if colors is None else colors.clone(), f
    else:
        out_v, out_c, out_f = _emit(v, f, colors, V, F, r)
    if method != "polar":
        area = _area(v, f, names, V, F, r, 1 << 5 if method == "auto" else 1 | 1 << 5, max_area_edges, min_sin)
        out_f = torch.cat([out_f, area["faces"]])
        if V >= 1 << 31 or 3 * out_f.shape[0] >= 1 << 31:
            raise ValueError("fill_holes: the filled mesh leaves the index range (n_verts < 2^31, 3 * n_faces < 2^31)")
    NV = out_v.shape[0] - V
    if fair and NV:
        fixed = torch.ones(V + NV, dtype=torch.uint8, device=v.device)
        fixed[V:] = 0
        out_v = smooth({"verts": out_v, "faces": out_f}, method="laplacian", iterations=int(fair), lam=lam, fixed=fixed,
                       normals=None)["verts"]
    result = {k: x for k, x in mesh.items() if k not in ("verts", "faces", "colors", "normals")}
    result["verts"], result["faces"] = give(out_v), give(out_f)
    if out_c is not None:
        result["colors"] = give(out_c)
    if normals in WEIGHTING:
        result["normals"] = give(_vertex_normals(out_v.contiguous(), out_f.contiguous(), V + NV, F + out_f.shape[0] - F, normals))
    elif normals == "keep" and stored is not None:
        old = as_tensor(stored).to(v.device).float()
        new = _vertex_normals(out_v.contiguous(), out_f.contiguous(), V + NV, out_f.shape[0], "angle")[V:] if NV else old[:0]
        result["normals"] = give(torch.cat([old, new]))
    if return_report:
        rep = _report(r, give, V, NV)
        rep = rep if method == "polar" else _area_report(rep, r, area, give, method)
        if intersections:
            rep["proper_pairs"] = _patch_intersections(out_v, out_f, F, rep, method)
        return result, rep
    return result


def boundary_loops(mesh, weld=False, device="cuda"):
    """The ordered boundary loops of ``mesh``, a dict: ``loop_start`` [L + 1], ``vertices`` (the start vertices of the loops'
    half-edges in rank order, loop after loop; each loop runs the way its boundary half-edges run), ``halfedges`` likewise, ``class``
    (what ``fill_holes`` with its defaults would make of each loop) and ``n_open_chain``, the boundary half-edges on no loop."""
    v, f, names, mask, colors, V, F, give = _arrays(mesh, "boundary_loops", weld, device)
    r = _loops(v, f, names, mask, None, V, F, None, None, 0, 64, True)
    order = r["order"].long()
    n = r["ints"][:, 1]
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device=v.device), torch.cumsum(n, 0)])
    return dict(loop_start=give(start), vertices=give(f.reshape(-1)[order]), halfedges=give(r["order"]),
                **{"class": [CLASSES[c] for c in r["ints"][:, 3].tolist()]}, n_open_chain=r["totals"]["n_open_chain"])


def format_report(rep):
    t = rep["totals"]
    lines = [f"{t['n_boundary']} boundary half-edges: {t['n_loops']} loops ({t['n_filled']} filled), {t['n_open_chain']} on open chains; "
             f"+{t['n_new_verts']} vertices, +{t['n_new_faces']} faces"]
    skipped = ", ".join(f"{t['n_' + c]} {c}" for c in CLASSES[1:] if t["n_" + c])
    return lines[0] + (f"; skipped: {skipped}" if skipped else "")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_fill", description=__doc__.splitlines()[0])
    ap.add_argument("mesh", metavar="IN.ply")
    ap.add_argument("--out", default=None, metavar="OUT.ply")
    ap.add_argument("--max-edges", type=int, default=None, help="fill only loops of at most this many edges")
    ap.add_argument("--max-size", type=float, default=None, help="fill only loops whose bounding-box diagonal is at most this")
    ap.add_argument("--rings", default="auto", help="auto, or the number of rings of every patch")
    ap.add_argument("--fair", type=int, default=0, help="Laplacian steps over the new vertices")
    ap.add_argument("--keep-folded", action="store_true", help="fill loops that are not star-shaped as well")
    ap.add_argument("--method", choices=METHODS, default="polar", help="auto: minimum-area patches for the folded loops")
    ap.add_argument("--max-area-edges", type=int, default=2048, help="the longest loop that gets a minimum-area patch")
    ap.add_argument("--min-sin", type=float, default=1e-6, help="no patch triangle flatter than this")
    ap.add_argument("--normals", choices=("keep", "angle", "area", "none"), default="keep")
    ap.add_argument("--weld", action="store_true")
    ap.add_argument("--list", action="store_true", help="print one line per loop")
    ap.add_argument("--json", action="store_true", help="print the totals as one JSON object")
    a = ap.parse_args(argv)
    if a.out is None and not a.list:
        ap.error("give --out, --list or both")
    if a.rings != "auto":
        try:
            a.rings = int(a.rings)
        except ValueError:
            ap.error("--rings takes auto or an integer")
    need_gpu("mesh_fill")
    try:
        mesh = read_ply(a.mesh)
        r, rep = fill_holes(mesh, max_edges=a.max_edges, max_size=a.max_size, rings=a.rings, skip_folded=not a.keep_folded, fair=a.fair,
                            normals=a.normals, weld=a.weld, return_report=True, method=a.method, max_area_edges=a.max_area_edges,
                            min_sin=a.min_sin)
        if a.out is not None:
            write_mesh_ply(a.out, r)
    except (ValueError, OSError) as e:
        print(f"mesh_fill: {e}", file=sys.stderr)
        raise SystemExit(2)
    t = rep["totals"]
    if a.list and not a.json:
        for l in range(t["n_loops"]):
            extra = f", {rep['area_class'][l]}, area {float(rep['area'][l]):.6g}" if rep.get("area_class", [None] * (l + 1))[l] else ""
            print(f"loop {l}: {rep['n'][l]} edges, {rep['class'][l]}, {rep['rings'][l]} rings, size {math.sqrt(float(rep['size2'][l])):.6g}"
                  + extra)
    if "area_totals" in rep:
        t = dict(t, **rep["area_totals"])
    area_line = ""
    if "area_totals" in rep:
        at = rep["area_totals"]
        area_line = (f"; minimum-area patches: {at['n_area_filled']} of {at['n_selected']} loops, +{at['n_area_faces']} faces"
                     + (f", {at['n_area_too_many_edges']} over the edge cap" if at["n_area_too_many_edges"] else "")
                     + (f", {at['n_no_triangulation']} without a triangulation" if at["n_no_triangulation"] else ""))
    print(json.dumps(t) if a.json else format_report(rep) + area_line + (f" -> {a.out}" if a.out else ""))
    return t


if __name__ == "__main__":
    main()
