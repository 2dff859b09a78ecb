"""Mesh decimation on the device: parallel edge collapse with quadric error (C ABI Section 22, csrc/mesh_decimate.hip).

* ``decimate(mesh, target_faces=None, max_error=None, ...)``: the mesh with edges collapsed cheapest first until the face count or
  the error limit is reached.  Unlike ``mesh_simplify.simplify`` (vertex clustering) it is tied to no grid, keeps a flat wall at a
  few triangles while a thin part keeps its detail, and keeps the topology: the link condition holds at every collapse, so a closed
  manifold input gives a closed manifold output with the same Euler characteristic.
* ``python -m nicer_slam_amd.mesh_decimate IN.ply --out OUT.ply (--faces N | --max-error D) [--boundary quadric|fixed]
  [--min-cos C] [--normals angle|area|none] [--json]``

Collapses run in rounds of edges that are pairwise more than one edge apart, selected without atomics, so the result is a function of
the input alone; float64 with every operation rounded on its own, and the result equals the numpy statement in tests/decimate_ref.py
bit for bit.  Decimation is BY INDEX, like smoothing: weld a mesh whose seams repeat vertices first.

numpy in, numpy out; torch in, torch out on the caller's device.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import json
import math
import sys

import torch

from . import _native
from ._native import lib, check
from .mesh_args import MAX_FACES_RINGS, checked_mesh, need_gpu, ptr, stream, workspace
from .mesh_smooth import WEIGHTING, _vertex_normals
from .ply import read_ply, write_mesh_ply

BOUNDARY = {"quadric": _native.DECIMATE_BOUNDARY_QUADRIC, "fixed": _native.DECIMATE_BOUNDARY_FIXED}
NORMALS = ("angle", "area", None)
TOTALS = ("rounds", "collapses", "n_candidates", "rej_lock", "rej_error", "rej_link", "rej_fold", "n_selected", "n_faces", "n_verts",
          "status")


class _Tables:
    """the edge table (Section 18) and the rings (Section 21) of a face list, in buffers allocated once and refilled every round
    without a read back"""

    def __init__(self, V, F, dev):
        H = 3 * F
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
        self.V, self.F, self.dev = V, F, dev
        self.edges, self.edge_count, self.edge_forward = i32(H, 2), i32(H), i32(H)
        self.edge_start, self.edge_halfedges, self.face_edges = i32(H + 1), i32(H), i32(F, 3)
        self.totals = torch.empty(8, dtype=torch.int64, device=dev)
        self.ring_start, self.ring, self.ring_edge = i32(V + 1), i32(6 * F), i32(6 * F)
        self.ws_edges = workspace(lib.nsa_mesh_edges_workspace(V, F), dev)
        self.ws_ring = workspace(lib.nsa_mesh_ring_workspace(V, F), dev)

    def build(self, faces):
        s = stream(self.dev)
        check(lib.nsa_mesh_edges(faces.data_ptr(), self.F, self.V, None, self.ws_edges.data_ptr(), self.edges.data_ptr(),
                                 self.edge_count.data_ptr(), self.edge_forward.data_ptr(), self.edge_start.data_ptr(),
                                 self.edge_halfedges.data_ptr(), self.face_edges.data_ptr(), self.totals.data_ptr(), s))
        check(lib.nsa_mesh_ring(self.edges.data_ptr(), self.totals.data_ptr(), self.V, self.F, self.ws_ring.data_ptr(),
                                self.ring_start.data_ptr(), self.ring.data_ptr(), self.ring_edge.data_ptr(), s))


@torch.no_grad()
def _decimate(v, f, colors, fixed, target_faces, max_error, boundary, boundary_weight, min_cos, eps, max_rounds, on_round=None):
    """the rounds on device arrays: (out verts fp32 [V, 3], out colours or None, faces int32 [F, 3] rewritten, vertex_map int32 [V]
    by input index, log int64 [n, 4], totals dict).  One read back of 14 words per round."""
    dev, V, F = v.device, v.shape[0], f.shape[0]
    fw = f.clone()
    last = dict.fromkeys(TOTALS[2:8], 0)
    if V == 0 or F == 0:
        return v.clone(), None if colors is None else colors.clone(), fw, torch.arange(V, dtype=torch.int32, device=dev), \
            torch.zeros(0, 4, dtype=torch.int64, device=dev), dict(rounds=0, collapses=0, **last, status=0)
    tb = _Tables(V, F, dev)
    state = workspace(lib.nsa_mesh_decimate_state_bytes(V), dev)
    ws = workspace(lib.nsa_mesh_decimate_workspace(V, F), dev)
    log = torch.zeros(V, 4, dtype=torch.int64, device=dev)
    totals = torch.zeros(14, dtype=torch.int64, device=dev)
    s = stream(dev)
    tb.build(fw)
    check(lib.nsa_mesh_decimate_init(v.data_ptr(), ptr(colors), V, fw.data_ptr(), F, tb.edge_count.data_ptr(), tb.edge_start.data_ptr(),
                                     tb.edge_halfedges.data_ptr(), tb.ring_start.data_ptr(), tb.ring.data_ptr(), tb.ring_edge.data_ptr(),
                                     ptr(fixed), BOUNDARY[boundary], float(boundary_weight), ws.data_ptr(), state.data_ptr(), s))
    host = [int(x) for x in tb.totals.cpu()]
    if host[7] != 0:
        raise RuntimeError(f"decimate: the edge table reported status {host[7]}; this is a bug")
    n_faces, rounds, collapses, status = host[1], 0, 0, 0
    me2 = 0.0 if max_error is None else float(max_error) * float(max_error)
    mc2 = float(min_cos) * float(min_cos)
    while rounds < max_rounds and n_faces > 0:
        if target_faces is not None and n_faces <= target_faces:
            break
        if rounds:
            tb.build(fw)
        check(lib.nsa_mesh_decimate_round(V, fw.data_ptr(), F, tb.edges.data_ptr(), tb.edge_count.data_ptr(), tb.edge_start.data_ptr(),
                                          tb.edge_halfedges.data_ptr(), tb.totals.data_ptr(), tb.ring_start.data_ptr(),
                                          tb.ring.data_ptr(), tb.ring_edge.data_ptr(), rounds, int(target_faces is not None),
                                          int(target_faces or 0), int(max_error is not None), me2, mc2, float(eps),
                                          int(colors is not None), ws.data_ptr(), state.data_ptr(), log.data_ptr(), V,
                                          totals.data_ptr(), s))
        t = [int(x) for x in totals.cpu()]
        rounds += 1
        last = dict(zip(TOTALS[2:8], t[3:9]))
        n_faces, collapses, status = t[11], t[12], status | t[13]
        if on_round is not None:
            on_round(t)
        if t[9] == 0:
            break
    if status != 0:
        raise RuntimeError(f"decimate: a sort order left its range (status {status}); this is a bug")
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(V, 3, dtype=torch.float32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    check(lib.nsa_mesh_decimate_finish(v.data_ptr(), ptr(colors), V, state.data_ptr(), out.data_ptr(), ptr(out_c), vmap.data_ptr(), s))
    return out, out_c, fw, vmap, log[:collapses], dict(rounds=rounds, collapses=collapses, **last, status=status)


def _compact(verts, colors, fw, vmap):
    """the faces that still contribute in input order over the vertices they name in index order: (verts, colours, faces int32,
    vertex_map int32 by input vertex (-1: unused), face_origin int32)"""
    V = verts.shape[0]
    inside = ((fw >= 0) & (fw < V)).all(1)
    ok = inside & (fw[:, 0] != fw[:, 1]) & (fw[:, 1] != fw[:, 2]) & (fw[:, 2] != fw[:, 0])
    face_origin = torch.nonzero(ok).reshape(-1)
    kept = fw[face_origin].long()
    used = torch.zeros(V, dtype=torch.bool, device=verts.device)
    used[kept.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    root = vmap.long()
    vertex_map = torch.where(used[root], new[root], torch.full_like(root, -1)).to(torch.int32) if V else vmap
    return verts[used], None if colors is None else colors[used], new[kept].to(torch.int32).reshape(-1, 3), vertex_map, \
        face_origin.to(torch.int32)


def _checked_args(target_faces, max_error, boundary, boundary_weight, min_cos, eps, max_rounds, normals):
    if target_faces is None and max_error is None:
        raise ValueError("decimate: give target_faces, max_error or both")
    if target_faces is not None and (isinstance(target_faces, bool) or int(target_faces) != target_faces or target_faces < 0):
        raise ValueError("decimate: target_faces must be a non-negative integer")
    if max_error is not None and not (math.isfinite(float(max_error)) and float(max_error) >= 0.0):
        raise ValueError("decimate: max_error must be finite and >= 0")
    if boundary not in BOUNDARY:
        raise ValueError(f"decimate: boundary must be one of {tuple(BOUNDARY)}, got {boundary!r}")
    if not (math.isfinite(float(boundary_weight)) and float(boundary_weight) >= 0.0):
        raise ValueError("decimate: boundary_weight must be finite and >= 0")
    if not 0.0 <= float(min_cos) < 1.0:
        raise ValueError("decimate: 0 <= min_cos < 1")
    if not (math.isfinite(float(eps)) and float(eps) >= 0.0):
        raise ValueError("decimate: eps must be finite and >= 0")
    if isinstance(max_rounds, bool) or int(max_rounds) != max_rounds or max_rounds < 0 or max_rounds >= 1 << 31:
        raise ValueError("decimate: max_rounds must be a count")
    if normals not in NORMALS:
        raise ValueError(f"decimate: normals must be one of {NORMALS}, got {normals!r}")


def decimate(mesh, target_faces=None, max_error=None, boundary="quadric", boundary_weight=1.0, min_cos=0.2, eps=1e-3, fixed=None,
             max_rounds=256, normals="angle", return_map=False):
    """``mesh`` (a dict with ``verts`` [V, 3] and ``faces`` [F, 3], optionally ``colors`` [V, 3]; numpy or torch) decimated by edge
    collapse with quadric error (header Section 22): a new dict of the same kind.
      target_faces  stop at this face count: the result has N or N - 1 faces when the collapses allowed reach it.
      max_error     an edge may collapse only while the squared-area weighted RMS distance of the merged vertex to the planes it
                    stands for stays within this length.  At least one of the two is required; both may be given.
      boundary      "quadric": boundary edges hold their line with constraint planes of weight ``boundary_weight``; "fixed": their
                    vertices never move.
      min_cos       no face may turn by more than this cosine allows in one collapse (and none may turn over or vanish).
      eps           the placement is pulled towards the edge's midpoint with weight eps times the quadric's trace.
      fixed         [V] mask (anything non-zero holds the vertex) or None.
      max_rounds    the most rounds of independent collapses.
      normals       "angle" / "area": ``mesh_smooth.vertex_normals`` of the result; None: none.
    A non-finite vertex, the vertices of its faces and the ends of a non-manifold edge never take part; a face with an index outside
    [0, V) is dropped.  Surviving faces keep their input order, surviving vertices their index order, and a vertex that never moved
    its input bits.  ``return_map=True`` adds ``vertex_map`` [V] (the output vertex each input vertex was merged into, -1 if unused),
    ``face_origin`` [F'], ``log`` [n, 4] int64 rows (round, lo, hi, the bits of the float64 cost) in the order of collapse, and
    ``totals``: ``rounds``, ``collapses``, the last round's ``n_candidates``, ``rej_lock``, ``rej_error``, ``rej_link``, ``rej_fold`` and ``n_selected``,
    ``n_faces``, ``n_verts``, ``status``.  Out of scope: collapsing onto a locked vertex, attribute-aware and memoryless quadrics,
    repairing non-manifold input, merging the two sides of a sheet.  Reads fourteen words back per round (a synchronisation)."""
    _checked_args(target_faces, max_error, boundary, boundary_weight, min_cos, eps, max_rounds, normals)
    if not isinstance(mesh, dict) or "verts" not in mesh:
        raise ValueError("decimate: mesh needs 'verts' and 'faces'")
    mask = None
    if fixed is not None:
        mask = torch.as_tensor(fixed).reshape(-1)
        if mask.shape[0] != mesh["verts"].shape[0]:
            raise ValueError(f"decimate: fixed mask of {mask.shape[0]} for {mesh['verts'].shape[0]} vertices")
    v, f, _, _, extra, restore = checked_mesh(mesh, "decimate", float_verts=True, attributes=("colors",), float_attributes=True,
                                              max_faces=MAX_FACES_RINGS)
    colors = extra.get("colors")
    if mask is not None:
        mask = (mask.to(v.device) != 0).to(torch.uint8).contiguous()
    out, out_c, fw, vmap, log, totals = _decimate(v, f, colors, mask, None if target_faces is None else int(target_faces), max_error,
                                                  boundary, boundary_weight, min_cos, eps, int(max_rounds))
    verts, cols, faces, vertex_map, face_origin = _compact(out, out_c, fw, vmap)
    result = {k: x for k, x in mesh.items() if k not in ("verts", "faces", "colors", "normals")}
    result["verts"], result["faces"] = restore(verts), restore(faces)
    if cols is not None:
        result["colors"] = restore(cols)
    if normals in WEIGHTING:
        result["normals"] = restore(_vertex_normals(verts.contiguous(), faces.contiguous(), verts.shape[0], faces.shape[0], normals))
    if return_map:
        totals = dict(totals, n_faces=int(faces.shape[0]), n_verts=int(verts.shape[0]))
        result.update(vertex_map=restore(vertex_map), face_origin=restore(face_origin), log=restore(log),
                      totals={k: totals[k] for k in TOTALS})
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_decimate", description=__doc__.splitlines()[0])
    ap.add_argument("mesh", metavar="IN.ply")
    ap.add_argument("--out", required=True, metavar="OUT.ply")
    ap.add_argument("--faces", type=int, default=None, help="target face count")
    ap.add_argument("--max-error", type=float, default=None, help="largest weighted RMS distance to the collected planes")
    ap.add_argument("--boundary", choices=tuple(BOUNDARY), default="quadric")
    ap.add_argument("--min-cos", type=float, default=0.2)
    ap.add_argument("--normals", choices=("angle", "area", "none"), default="angle")
    ap.add_argument("--json", action="store_true", help="print the totals as one JSON object")
    a = ap.parse_args(argv)
    if a.faces is None and a.max_error is None:
        ap.error("give --faces, --max-error or both")
    need_gpu("mesh_decimate")
    try:
        r = decimate(read_ply(a.mesh), target_faces=a.faces, max_error=a.max_error, boundary=a.boundary, min_cos=a.min_cos,
                     normals=None if a.normals == "none" else a.normals, return_map=True)
        write_mesh_ply(a.out, r)
    except (ValueError, OSError) as e:
        print(f"mesh_decimate: {e}", file=sys.stderr)
        raise SystemExit(2)
    t = r["totals"]
    print(json.dumps(t) if a.json else
          f"{t['collapses']} collapses in {t['rounds']} rounds -> {t['n_faces']} faces, {t['n_verts']} vertices -> {a.out}")
    return t


if __name__ == "__main__":
    main()
