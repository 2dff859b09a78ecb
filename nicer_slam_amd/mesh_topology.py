"""Mesh topology on the device: the undirected edge table of a triangle mesh and what falls out of it (C ABI Section 18,
csrc/mesh_topology.hip).

* ``edge_table(faces, n_verts)``: the distinct edges in ascending (lo, hi) order with the number of half-edges on each, how many
  run lo -> hi, their ids in CSR form, and the edge id of every half-edge; with it the totals: boundary, non-manifold and
  inconsistently oriented edges, used vertices, boundary loops.
* ``topology(mesh)``: the report -- watertight? consistently oriented? Euler characteristic, holes, components joined across edges.
  It answers what ``mesh_sdf``'s ``sign="normal"`` assumes (a closed, oriented mesh); ``sign="auto"`` there asks it.
* ``face_components(faces, n_verts)``: components of faces joined across shared EDGES (trimesh's ``split``, except that a
  non-manifold edge joins too), where ``mesh_clean.components`` joins at shared vertices.
* ``face_adjacency`` (trimesh's: the face pairs of the edges with exactly two faces), ``boundary_edges``.
* ``python -m nicer_slam_amd.mesh_topology MESH.ply [--weld] [--json]`` prints the report.

Everything is integer work and exact.  numpy in, numpy out; torch in, torch out.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import json
import sys

import numpy as np
import torch

from ._native import lib, check

REPORT_KEYS = ("n_faces", "n_contributing", "n_used_verts", "n_edges", "n_boundary", "n_nonmanifold", "n_inconsistent",
               "n_boundary_loops", "n_components", "euler", "is_watertight", "is_oriented")
_TOTALS = ("n_edges", "n_contributing", "n_used_verts", "n_boundary", "n_nonmanifold", "n_inconsistent", "n_boundary_loops")
_MAX_FACES = (2 ** 31 - 1) // 3


def _need_gpu(name):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{name}: needs a GPU")


def _to_cuda(x, name, device="cuda"):
    """(CUDA tensor, was_numpy, original device) of an array or tensor"""
    if torch.is_tensor(x):
        if x.is_cuda:
            return x, False, x.device
        _need_gpu(name)
        return x.to(device), False, x.device
    _need_gpu(name)
    return torch.from_numpy(np.ascontiguousarray(x)).to(device), True, None


def _checked(faces, n_verts, face_mask, name, device="cuda"):
    """(faces int32 CUDA [F, 3], V, F, mask uint8 CUDA or None, restore): the checked arguments -- shapes and ranges first, on
    whatever device they live, then the move to the GPU -- and the function that gives a result tensor the caller's kind back"""
    was_numpy = not torch.is_tensor(faces)
    f = torch.from_numpy(np.ascontiguousarray(faces)) if was_numpy else faces
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{name}: faces must be [F, 3]")
    if f.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: faces must be int32 or int64")
    V, F = int(n_verts), f.shape[0]
    if V < 0 or V >= 1 << 31 or F > _MAX_FACES:
        raise ValueError(f"{name}: count out of range (0 <= n_verts < 2^31, 3 * n_faces < 2^31)")
    if f.dtype == torch.int64 and f.numel() and (int(f.min()) < -2 ** 31 or int(f.max()) >= 2 ** 31):
        raise ValueError(f"{name}: face index outside int32")
    mask = None
    if face_mask is not None:
        mask = torch.as_tensor(face_mask).reshape(-1)
        if mask.shape[0] != F:
            raise ValueError(f"{name}: mask of {mask.shape[0]} for {F} faces")
    orig = None if was_numpy else f.device
    f, _, _ = _to_cuda(f, name, device)
    f = f.to(torch.int32).contiguous()
    if mask is not None:
        mask = (mask.to(f.device) != 0).to(torch.uint8).contiguous()
    return f, V, F, mask, lambda t: t.cpu().numpy() if was_numpy else t.to(orig)


@torch.no_grad()
def _edge_table(f, V, F, mask):
    """the full-size device arrays of nsa_mesh_edges and the totals as a dict of ints (one read back: a synchronisation)"""
    dev, H = f.device, 3 * F
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    t = dict(edges=i32(H, 2), edge_count=i32(H), edge_forward=i32(H), edge_start=i32(H + 1), edge_halfedges=i32(H),
             face_edges=i32(F, 3))
    totals = dict.fromkeys(_TOTALS, 0)
    if F == 0:
        t["edge_start"].zero_()
        return t, totals
    ws = torch.empty(lib.nsa_mesh_edges_workspace(V, F), dtype=torch.uint8, device=dev)
    tot = torch.empty(8, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_edges(f.data_ptr(), F, V, mask.data_ptr() if mask is not None else None, ws.data_ptr(),
                             t["edges"].data_ptr(), t["edge_count"].data_ptr(), t["edge_forward"].data_ptr(),
                             t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(), t["face_edges"].data_ptr(),
                             tot.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    host = [int(x) for x in tot.cpu()]
    if host[7] != 0:
        raise RuntimeError(f"edge_table: the boundary union-find left its loop on a step cap (status {host[7]}); this is a bug")
    totals = dict(zip(_TOTALS, host[:7]))
    return t, totals


@torch.no_grad()
def _face_components(t, F, dev):
    label = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return label, 0
    ws = torch.empty(lib.nsa_mesh_face_components_workspace(F), dtype=torch.uint8, device=dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_face_components(t["face_edges"].data_ptr(), t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(), F,
                                       ws.data_ptr(), label.data_ptr(), tot.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    C, status = (int(x) for x in tot.cpu())
    if status != 0:
        raise RuntimeError(f"face_components: the labelling kernel left its loop on a step cap (status {status}); this is a bug")
    return label, C


def _slice(t, totals):
    E, Hc = totals["n_edges"], 3 * totals["n_contributing"]
    out = dict(edges=t["edges"][:E], edge_count=t["edge_count"][:E], edge_forward=t["edge_forward"][:E],
               edge_start=t["edge_start"][:E + 1], edge_halfedges=t["edge_halfedges"][:Hc], face_edges=t["face_edges"])
    out.update(totals)
    return out


def edge_table(faces, n_verts, face_mask=None):
    """The edge table of ``faces`` [F, 3] (int32 or int64) over ``n_verts`` vertices (header Section 18), as a dict of
    tensors (arrays for numpy faces) sliced to the E edges -- ``edges`` [E, 2], ``edge_count`` [E], ``edge_forward`` [E], ``edge_start`` [E + 1],
    ``edge_halfedges`` [3 F_c], ``face_edges`` [F, 3] (-1 for a face that does not contribute), all int32 -- plus the totals as
    ints: ``n_edges``, ``n_contributing``, ``n_used_verts``, ``n_boundary``, ``n_nonmanifold``, ``n_inconsistent``,
    ``n_boundary_loops``.  A face contributes when its indices lie in [0, n_verts), are pairwise distinct and ``face_mask`` [F]
    (None: all) is non-zero for it.  Reads the totals back once (a synchronisation)."""
    f, V, F, mask, restore = _checked(faces, n_verts, face_mask, "edge_table")
    return {k: restore(x) if torch.is_tensor(x) else x for k, x in _slice(*_edge_table(f, V, F, mask)).items()}


def face_components(faces, n_verts, face_mask=None):
    """(face_label [F] int32, n_components): the components of the contributing faces joined across shared edges (any edge with two or
    more faces; the closure is transitive).  The label is the smallest face index of the component, -1 for a face that does not
    contribute.  trimesh's ``split`` cuts at a non-manifold edge; this joins across it."""
    f, V, F, mask, restore = _checked(faces, n_verts, face_mask, "face_components")
    t, _ = _edge_table(f, V, F, mask)
    label, C = _face_components(t, F, f.device)
    return restore(label), C


def face_adjacency(faces, n_verts):
    """[P, 2] int32: the face pairs (f0 < f1) of the edges with exactly two faces, in edge order -- trimesh's ``face_adjacency``"""
    f, V, F, _, restore = _checked(faces, n_verts, None, "face_adjacency")
    t = _slice(*_edge_table(f, V, F, None))
    s = t["edge_start"][:-1][t["edge_count"] == 2].long()
    he = t["edge_halfedges"]
    pairs = torch.stack([torch.div(he[s], 3, rounding_mode="floor"), torch.div(he[s + 1], 3, rounding_mode="floor")], 1)
    return restore(pairs.to(torch.int32))


def boundary_edges(faces, n_verts):
    """[B, 2] int32: the (lo, hi) of the edges with one face, in edge order"""
    f, V, F, _, restore = _checked(faces, n_verts, None, "boundary_edges")
    t = _slice(*_edge_table(f, V, F, None))
    return restore(t["edges"][t["edge_count"] == 1])


def _report(F, totals, C):
    r = {"n_faces": F}
    r.update(totals)
    r["n_components"] = C
    r["euler"] = totals["n_used_verts"] - totals["n_edges"] + totals["n_contributing"]
    r["is_watertight"] = totals["n_contributing"] > 0 and totals["n_boundary"] == 0 and totals["n_nonmanifold"] == 0
    r["is_oriented"] = r["is_watertight"] and totals["n_inconsistent"] == 0
    return {k: r[k] for k in REPORT_KEYS}


@torch.no_grad()
def topology(mesh, weld=False, device="cuda"):
    """The topology report of ``mesh`` (a dict with ``verts`` and ``faces``, numpy or torch), a dict of ints and bools:
      n_faces, n_contributing, n_used_verts, n_edges, n_boundary, n_nonmanifold, n_inconsistent, n_boundary_loops (the holes),
      n_components (joined across edges), euler = used vertices - edges + contributing faces,
      is_watertight  (some face contributes, no boundary and no non-manifold edge),
      is_oriented    (watertight and no interior edge that its two faces traverse the same way).
    ``weld=True`` names every vertex by its fp32 coordinates as ``TriIndex.adjacency(weld=True)`` does
    (``mesh_eval.welded_faces``), so a mesh whose seams repeat vertices is connected across them, and masks out the faces that have
    a non-finite vertex; the mesh itself is not rewritten."""
    from .mesh_eval import welded_faces
    if "verts" not in mesh or "faces" not in mesh:
        raise ValueError("topology: mesh needs 'verts' and 'faces'")
    if len(mesh["verts"].shape) != 2 or mesh["verts"].shape[1] != 3:
        raise ValueError("topology: verts must be [V, 3]")
    if torch.is_tensor(mesh["verts"]) and mesh["verts"].is_cuda:
        device = mesh["verts"].device
    f, V, F, _, _ = _checked(mesh["faces"], mesh["verts"].shape[0], None, "topology", device)
    v, _, _ = _to_cuda(mesh["verts"], "topology", f.device)
    mask = None
    if weld and F:
        v = v.detach().float()
        ok = ((f >= 0) & (f < V)).all(1)
        safe = torch.where(ok[:, None], f, torch.zeros_like(f)).long()
        mask = (ok & torch.isfinite(v)[safe].all(2).all(1)).to(torch.uint8) if V else ok.to(torch.uint8)
        f = welded_faces(v, f) if V else f
    t, totals = _edge_table(f, V, F, mask)
    _, C = _face_components(t, F, f.device)
    return _report(F, totals, C)


def split_faces(faces, face_label, n_verts):
    """(faces' [F, 3] int32, origin [V'] int64): ``faces`` over the vertices duplicated once per edge-joined component that uses
    them.  Vertex v gets max(1, components that use it) consecutive slots, the vertices in their order and a vertex's components in
    ascending label order, so a mesh without a vertex shared between components keeps every index; ``origin`` names the vertex
    each slot copies; a face with label -1 becomes (-1, -1, -1).  On this mesh the vertex-joined components of
    ``mesh_clean.components`` are the edge-joined ones of the original."""
    V, dev = int(n_verts), faces.device
    ok = face_label >= 0
    key = faces[ok].long() * (1 << 31) + face_label[ok].long()[:, None]
    uniq, inverse = torch.unique(key.reshape(-1), return_inverse=True)
    per_vertex = torch.bincount(uniq >> 31, minlength=V)
    slots = per_vertex.clamp_min(1)
    base = torch.cumsum(slots, 0) - slots                        # first slot of vertex v
    first = torch.cumsum(per_vertex, 0) - per_vertex             # first (vertex, component) pair of vertex v
    v_of = uniq >> 31
    slot = base[v_of] + (torch.arange(uniq.numel(), device=dev) - first[v_of])
    out = torch.full_like(faces, -1)
    out[ok] = slot[inverse].reshape(-1, 3).to(faces.dtype)
    origin = torch.repeat_interleave(torch.arange(V, device=dev), slots)
    return out, origin


def format_report(r):
    lines = [f"faces {r['n_faces']} ({r['n_contributing']} contributing), vertices used {r['n_used_verts']}, edges {r['n_edges']}",
             f"boundary edges {r['n_boundary']} in {r['n_boundary_loops']} loops, non-manifold edges {r['n_nonmanifold']}, "
             f"inconsistent edges {r['n_inconsistent']}",
             f"components (joined across edges) {r['n_components']}, Euler characteristic {r['euler']}",
             f"watertight: {'yes' if r['is_watertight'] else 'no'}   consistently oriented: {'yes' if r['is_oriented'] else 'no'}"]
    return lines


def main(argv=None):
    from .inference import read_ply
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_topology", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--weld", action="store_true", help="name vertices by their coordinates: connect across repeated seam vertices")
    ap.add_argument("--json", action="store_true", help="print the report as one JSON object")
    a = ap.parse_args(argv)
    _need_gpu("mesh_topology")
    try:
        r = topology(read_ply(a.mesh), weld=a.weld)
    except (ValueError, OSError) as e:
        print(f"mesh_topology: {e}", file=sys.stderr)
        raise SystemExit(2)
    print(json.dumps(r) if a.json else "\n".join(format_report(r)))
    return r


if __name__ == "__main__":
    main()
