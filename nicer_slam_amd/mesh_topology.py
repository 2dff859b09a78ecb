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
* ``orientation(mesh)`` / ``orient(mesh, outward=...)``: the faces to reverse for a consistent winding, whether that exists, and the
  re-wound mesh with its normals outward by signed volume or towards the cameras (C ABI Section 20, csrc/mesh_orient.hip).
* ``python -m nicer_slam_amd.mesh_topology MESH.ply [--weld] [--json]`` prints the report; ``--orient OUT.ply [--outward
  volume|views|none] [--poses P --intrinsics fx fy cx cy --size H W]`` writes the re-wound mesh and prints its report instead;
  ``--split`` cuts the mesh into a 2-manifold first (``mesh_repair.split_nonmanifold``), so that the winding can be
  carried across what were edges with more than two faces.

Everything is integer work and exact.  numpy in, numpy out; torch in, torch out.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import json
import sys

import numpy as np
import torch

from . import mesh_raycast as R
from ._native import lib, check
from .mesh_args import MAX_FACES_EDGES, checked_mesh, cuda_faces, kind, need_gpu, restore_dict, restorer, stream, workspace
from .mesh_eval import TriIndex, welded_faces
from .mesh_intersect import self_intersections
from .ply import read_ply, write_mesh_ply

REPORT_KEYS = ("n_faces", "n_contributing", "n_used_verts", "n_edges", "n_boundary", "n_nonmanifold", "n_inconsistent",
               "n_boundary_loops", "n_components", "euler", "is_watertight", "is_oriented")
_TOTALS = ("n_edges", "n_contributing", "n_used_verts", "n_boundary", "n_nonmanifold", "n_inconsistent", "n_boundary_loops")
_checked = cuda_faces            # (faces, n_verts, face_mask, name) -> what _edge_table takes: the name the kernels' device tests use


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
    ws = workspace(lib.nsa_mesh_edges_workspace(V, F), dev)
    tot = torch.empty(8, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_edges(f.data_ptr(), F, V, mask.data_ptr() if mask is not None else None, ws.data_ptr(),
                             t["edges"].data_ptr(), t["edge_count"].data_ptr(), t["edge_forward"].data_ptr(),
                             t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(), t["face_edges"].data_ptr(),
                             tot.data_ptr(), stream(dev)))
    host = [int(x) for x in tot.cpu()]
    if host[7] != 0:
        raise RuntimeError(f"edge_table: the boundary union-find left its loop on a step cap (status {host[7]}); this is a bug")
    totals = dict(zip(_TOTALS, host[:7]))
    t["_totals"] = tot                                   # (the device copy: nsa_mesh_orient reads E there)
    return t, totals


@torch.no_grad()
def _face_components(t, F, dev):
    label = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return label, 0
    ws = workspace(lib.nsa_mesh_face_components_workspace(F), dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_face_components(t["face_edges"].data_ptr(), t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(), F,
                                       ws.data_ptr(), label.data_ptr(), tot.data_ptr(), stream(dev)))
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
    f, V, F, mask, restore = cuda_faces(faces, n_verts, face_mask, "edge_table")
    return {k: restore(x) if torch.is_tensor(x) else x for k, x in _slice(*_edge_table(f, V, F, mask)).items()}


def face_components(faces, n_verts, face_mask=None):
    """(face_label [F] int32, n_components): the components of the contributing faces joined across shared edges (any edge with two or
    more faces; the closure is transitive).  The label is the smallest face index of the component, -1 for a face that does not
    contribute.  trimesh's ``split`` cuts at a non-manifold edge; this joins across it."""
    f, V, F, mask, restore = cuda_faces(faces, n_verts, face_mask, "face_components")
    t, _ = _edge_table(f, V, F, mask)
    label, C = _face_components(t, F, f.device)
    return restore(label), C


def face_adjacency(faces, n_verts):
    """[P, 2] int32: the face pairs (f0 < f1) of the edges with exactly two faces, in edge order -- trimesh's ``face_adjacency``"""
    f, V, F, _, restore = cuda_faces(faces, n_verts, None, "face_adjacency")
    t = _slice(*_edge_table(f, V, F, None))
    s = t["edge_start"][:-1][t["edge_count"] == 2].long()
    he = t["edge_halfedges"]
    pairs = torch.stack([torch.div(he[s], 3, rounding_mode="floor"), torch.div(he[s + 1], 3, rounding_mode="floor")], 1)
    return restore(pairs.to(torch.int32))


def boundary_edges(faces, n_verts):
    """[B, 2] int32: the (lo, hi) of the edges with one face, in edge order"""
    f, V, F, _, restore = cuda_faces(faces, n_verts, None, "boundary_edges")
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


def _mesh_arrays(mesh, weld, device, name):
    """(faces of the topology int32 CUDA [F, 3], V, F, mask or None, verts CUDA, the mesh's own faces int32 CUDA) of a mesh dict:
    with ``weld`` the first are ``mesh_eval.welded_faces`` and the mask leaves out the faces that have a non-finite vertex"""
    v, f, V, F, _, _ = checked_mesh(mesh, name, device, max_faces=MAX_FACES_EDGES)
    mask, f0 = None, f
    if weld and F:
        v = v.detach().float()
        ok = ((f >= 0) & (f < V)).all(1)
        safe = torch.where(ok[:, None], f, torch.zeros_like(f)).long()
        mask = (ok & torch.isfinite(v)[safe].all(2).all(1)).to(torch.uint8) if V else ok.to(torch.uint8)
        f = welded_faces(v, f) if V else f
    return f, V, F, mask, v, f0


@torch.no_grad()
def topology(mesh, weld=False, device="cuda", intersections=False):
    """The topology report of ``mesh`` (a dict with ``verts`` and ``faces``, numpy or torch), a dict of ints and bools:
      n_faces, n_contributing, n_used_verts, n_edges, n_boundary, n_nonmanifold, n_inconsistent, n_boundary_loops (the holes),
      n_components (joined across edges), euler = used vertices - edges + contributing faces,
      is_watertight  (some face contributes, no boundary and no non-manifold edge),
      is_oriented    (watertight and no interior edge that its two faces traverse the same way).
    ``weld=True`` names every vertex by its fp32 coordinates as ``TriIndex.adjacency(weld=True)`` does
    (``mesh_eval.welded_faces``), so a mesh whose seams repeat vertices is connected across them, and masks out the faces that have
    a non-finite vertex; the mesh itself is not rewritten.  ``intersections=True`` adds n_proper_pairs, the pairs of faces that
    meet properly (``mesh_intersect``, header Section 25, on the positions as they are: it welds by position itself), and embedded
    = there is none."""
    f, V, F, mask, _, _ = _mesh_arrays(mesh, weld, device, "topology")
    t, totals = _edge_table(f, V, F, mask)
    _, C = _face_components(t, F, f.device)
    r = _report(F, totals, C)
    if intersections:
        r["n_proper_pairs"] = int(self_intersections(mesh, kinds=("proper",), device=device)[0].shape[0])
        r["embedded"] = r["n_proper_pairs"] == 0
    return r


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


OUTWARD = ("volume", "views", None)
_ORIENT_TOTALS = ("n_components", "n_nonorientable", "n_flipped")


@torch.no_grad()
def _orientation(f, t, F):
    """(orient_label int32, orientable uint8, flip uint8) [F] on the device and the totals of nsa_mesh_orient as a dict of ints, from
    the topology faces ``f`` and their full-size edge table ``t`` (one read back: a synchronisation)"""
    dev = f.device
    label = torch.empty(F, dtype=torch.int32, device=dev)
    orientable = torch.empty(F, dtype=torch.uint8, device=dev)
    flip = torch.empty(F, dtype=torch.uint8, device=dev)
    if F == 0:
        return label, orientable, flip, dict.fromkeys(_ORIENT_TOTALS, 0)
    ws = workspace(lib.nsa_mesh_orient_workspace(F), dev)
    tot = torch.empty(4, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_orient(f.data_ptr(), F, t["face_edges"].data_ptr(), t["edge_start"].data_ptr(), t["edge_halfedges"].data_ptr(),
                              t["_totals"].data_ptr(), ws.data_ptr(), label.data_ptr(), orientable.data_ptr(), flip.data_ptr(),
                              tot.data_ptr(), stream(dev)))
    host = [int(x) for x in tot.cpu()]
    if host[3] != 0:
        raise RuntimeError(f"orientation: the union-find left its loop on a step cap (status {host[3]}); this is a bug")
    return label, orientable, flip, dict(zip(_ORIENT_TOTALS, host[:3]))


def _bbox_centre(v, f, label):
    """fp32 [3] on the device: the centre of the bounding box of the vertices the contributing faces use, formed in float64 and
    rounded once; zeros when no face contributes"""
    idx = f[label >= 0].reshape(-1).long()
    if idx.numel() == 0:
        return torch.zeros(3, dtype=torch.float32, device=v.device)
    used = v[idx]
    return ((used.amin(0).double() + used.amax(0).double()) / 2).float().contiguous()


@torch.no_grad()
def _orient_volume(v, f, V, F, t, label, orientable, flip):
    """nsa_mesh_orient_volume: (flip after the toggles uint8 [F], dict of the per-label arrays S, P, n, flags, origin, totals).
    ``f`` are the faces that index ``v``; the table ``t`` and the labels may come from a welded naming of the same faces."""
    dev = f.device
    v = v.detach().float().contiguous()
    origin = _bbox_centre(v, f, label) if V else torch.zeros(3, dtype=torch.float32, device=dev)
    S = torch.zeros(F, dtype=torch.float64, device=dev)
    P = torch.zeros(F, dtype=torch.float64, device=dev)
    n = torch.zeros(F, dtype=torch.int32, device=dev)
    flags = torch.zeros(F, dtype=torch.uint8, device=dev)
    out = torch.empty(F, dtype=torch.uint8, device=dev)
    totals = dict(n_closed=0, n_decided=0, n_toggled=0, n_flipped=0)
    if F:
        ws = workspace(lib.nsa_mesh_orient_volume_workspace(F), dev)
        tot = torch.empty(5, dtype=torch.int64, device=dev)
        check(lib.nsa_mesh_orient_volume(v.data_ptr() if V else None, V, f.data_ptr(), F, t["face_edges"].data_ptr(),
                                         t["edge_start"].data_ptr(), label.data_ptr(), orientable.data_ptr(), flip.data_ptr(),
                                         origin.data_ptr(), ws.data_ptr(), S.data_ptr(), P.data_ptr(), n.data_ptr(), flags.data_ptr(),
                                         out.data_ptr(), tot.data_ptr(), stream(dev)))
        host = [int(x) for x in tot.cpu()]
        if host[4] != 0:
            raise RuntimeError(f"orient: the sort by label left its range (status {host[4]}); this is a bug")
        totals = dict(zip(("n_closed", "n_decided", "n_toggled", "n_flipped"), host[:4]))
    return out, dict(S=S, P=P, n=n, flags=flags, origin=origin, **totals)


def _components(label, t, F):
    """(labels [C] int64 ascending, component index of every contributing face, the contributing faces, face count [C], closed [C]):
    the per-component part of the report, integer work in torch on the device"""
    ok = label >= 0
    comp = torch.nonzero(label == torch.arange(F, dtype=torch.int32, device=label.device)).reshape(-1)
    idx = torch.searchsorted(comp, label[ok].long())
    count = torch.bincount(idx, minlength=comp.numel())
    fe = t["face_edges"][ok].long().clamp_min(0)
    start = t["edge_start"].long()
    open_face = ((start[fe + 1] - start[fe]) != 2).any(1)
    closed = torch.bincount(idx[open_face], minlength=comp.numel()) == 0
    return comp, idx, ok, count, closed


def view_votes(verts, faces, flip, hit_face, dirs):
    """int64 [F]: for every face the votes of the rays that hit it -- +1 where the face, wound as ``flip`` says (second and third
    index swapped), faces the ray's origin (n . d < 0 with n = (b - a) x (c - a), float64 of the fp32 inputs, every operation a
    torch operation of its own), -1 where n . d > 0, nothing at 0.  ``hit_face`` [m] (-1: no hit), ``dirs`` [m, 3]."""
    F = faces.shape[0]
    hit = hit_face >= 0
    hf = hit_face[hit].long()
    fc = faces[hf].long()
    sw = flip[hf] != 0
    a = verts[fc[:, 0]].double()
    b, c = verts[torch.where(sw, fc[:, 2], fc[:, 1])].double(), verts[torch.where(sw, fc[:, 1], fc[:, 2])].double()
    u, w, d = b - a, c - a, dirs[hit].double()
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    dot = (nx * d[:, 0] + ny * d[:, 1]) + nz * d[:, 2]
    vote = (dot < 0).long() - (dot > 0).long()
    return torch.zeros(F, dtype=torch.int64, device=faces.device).index_add_(0, hf, vote)


@torch.no_grad()
def _view_hits(v, f0, c2w, intrinsics, size):
    """(hit face int64 [m], dirs fp32 [m, 3]) of the pixel rays of every camera, cast with ``TriIndex.raycast`` at the default near"""
    P = R._as_numpy(c2w, np.float64)
    P = P[None] if P.ndim == 2 else P
    if P.ndim != 3 or P.shape[1:] != (4, 4) or P.shape[0] == 0:
        raise ValueError("orient: c2w must be [4, 4] or [n, 4, 4] camera-to-world matrices")
    Ks = R._intrinsics4(intrinsics, P.shape[0])
    R._camera(P[0], Ks[0], size)
    ix = TriIndex(v, f0)
    faces, dirs = [], []
    for i in range(P.shape[0]):
        o, d = R.camera_rays(P[i], Ks[i if Ks.shape[0] > 1 else 0], size, device=ix.device)
        faces.append(ix.raycast(o, d, tmin=R.DEFAULT_NEAR)[1])
        dirs.append(d)
    return torch.cat(faces), torch.cat(dirs)


@torch.no_grad()
def _orient_arrays(mesh, outward, c2w, intrinsics, size, weld, device, name):
    if outward not in OUTWARD:
        raise ValueError(f"{name}: outward must be one of {OUTWARD}, got {outward!r}")
    if outward == "views" and (c2w is None or intrinsics is None or size is None):
        raise ValueError(f"{name}: outward='views' needs c2w, intrinsics and size")
    f, V, F, mask, v, f0 = _mesh_arrays(mesh, weld, device, name)
    t, _ = _edge_table(f, V, F, mask)
    label, orientable, flip, totals = _orientation(f, t, F)
    comp, idx, ok, count, closed = _components(label, t, F)
    C = comp.numel()
    rep = dict(totals)
    rep["is_orientable"] = totals["n_nonorientable"] == 0
    rep["component_label"], rep["component_faces"], rep["component_closed"] = comp, count, closed
    rep["outward"] = outward
    out = flip
    decided = torch.zeros(C, dtype=torch.bool, device=f.device)
    toggled = torch.zeros(C, dtype=torch.bool, device=f.device)
    if outward == "volume":
        out, vol = _orient_volume(v, f0, V, F, t, label, orientable, flip)     # (the mesh's own faces: welded names are no indices)
        fl = vol["flags"][comp]
        decided, toggled = (fl & 2) != 0, (fl & 4) != 0
        rep["component_volume"], rep["component_volume_bound"] = vol["S"][comp], vol["P"][comp]
        rep["origin"] = vol["origin"]
        rep["n_flipped"] = vol["n_flipped"]
    elif outward == "views" and F and V:
        hit_face, dirs = _view_hits(v.detach().float().contiguous(), f0, c2w, intrinsics, size)
        face_votes = view_votes(v.detach().float(), f0, flip, hit_face, dirs)
        votes = torch.zeros(C, dtype=torch.int64, device=f.device).index_add_(0, idx, face_votes[ok])
        can = orientable[comp] != 0
        decided, toggled = can & (votes != 0), can & (votes < 0)
        rep["component_votes"] = votes
        tog_face = torch.zeros(F, dtype=torch.bool, device=f.device)
        tog_face[ok] = toggled[idx]
        out = ((flip != 0) ^ tog_face).to(torch.uint8)
        rep["n_flipped"] = int(out.sum())
    rep["component_decided"], rep["component_toggled"] = decided, toggled
    rep["n_closed"] = int(closed.sum())
    rep["n_open"] = C - rep["n_closed"]
    rep["n_undecided"] = C - int(decided.sum()) if outward is not None else C
    rep["n_toggled"] = int(toggled.sum())
    return f0, V, F, label, orientable, flip, out, rep


def orientation(mesh, weld=False, device="cuda"):
    """(orient_label [F] int32, orientable [F] bool, flip [F] bool, report) of ``mesh`` (a dict with ``verts`` and ``faces``, numpy or
    torch; header Section 20).  Faces are joined across the edges that carry exactly two half-edges (trimesh's ``face_adjacency``);
    ``orient_label`` is the smallest face index of the face's component (-1 for a face that does not contribute), ``orientable``
    whether that component can be wound consistently (a Moebius strip cannot), ``flip`` the faces to reverse so that every orientable
    component is wound like its smallest face.  The report: ``n_components``, ``n_nonorientable``, ``n_flipped``, ``is_orientable``
    and per component, in ascending label, ``component_label``, ``component_faces`` and ``component_closed`` (every half-edge on
    an edge of count 2).  ``weld`` as in ``topology``."""
    _, _, _, label, orientable, flip, _, rep = _orient_arrays(mesh, None, None, None, None, weld, device, "orientation")
    was_numpy, orig = kind(mesh["faces"])
    back = restorer(was_numpy, orig)
    keep = _ORIENT_TOTALS + ("is_orientable", "component_label", "component_faces", "component_closed")
    return back(label), back(orientable != 0), back(flip != 0), restore_dict({k: rep[k] for k in keep}, was_numpy, orig)


def orient(mesh, outward="volume", c2w=None, intrinsics=None, size=None, weld=False, return_report=False, device="cuda"):
    """``mesh`` with a consistent winding: a new dict of the same kind (numpy or torch) in which every flipped face has its second
    and third index swapped, so a face that was reversed with that swap is restored bit for bit.  Faces that do not contribute and
    the faces of a non-orientable component are untouched; vertices, colours and the order of everything are unchanged; vertex
    ``normals``, when present, are negated at a vertex exactly when every contributing face at it ended up flipped (a vertex with both
    kinds keeps its normal and counts in ``n_mixed_normals``).
    ``outward`` picks between the two consistent windings of an orientable component:
      "volume"  a closed component (every half-edge on an edge of count 2) whose signed volume is decided against its float64 error
                bound is wound so that the volume is positive; open and undecided components keep the winding of their smallest face;
      "views"   needs ``c2w`` ([4, 4] or [n, 4, 4]), ``intrinsics`` and ``size`` as ``mesh_raycast.render_depth`` takes them: every
                pixel ray that hits a component votes +1 when the face hit looks at the camera and -1 when it looks away; a negative
                total toggles the component, a zero total leaves it undecided -- "outward" is "towards where the cameras were";
      None      the winding of each component's smallest face.
    ``return_report=True`` appends ``orientation``'s report with ``n_closed``, ``n_open``, ``n_undecided``, ``n_toggled``,
    ``n_mixed_normals``, the per-component ``component_decided`` / ``component_toggled`` and, by rule, ``component_volume`` and
    ``component_volume_bound`` (S_c, P_c) or ``component_votes``; ``n_flipped`` counts the faces reversed in the result."""
    f0, V, F, label, _, _, out, rep = _orient_arrays(mesh, outward, c2w, intrinsics, size, weld, device, "orient")
    was_numpy, orig = kind(mesh["faces"])
    faces = mesh["faces"] if torch.is_tensor(mesh["faces"]) else torch.from_numpy(np.ascontiguousarray(mesh["faces"]))
    sw = (out != 0).to(faces.device)
    new_faces = torch.where(sw[:, None], faces[:, [0, 2, 1]], faces) if F else faces.clone()
    result = dict(mesh)
    result["faces"] = new_faces.numpy() if was_numpy else new_faces
    rep["n_mixed_normals"] = 0
    if mesh.get("normals") is not None and F and V:
        ok = label >= 0
        at = torch.zeros(V, dtype=torch.int64, device=f0.device)
        fl = torch.zeros(V, dtype=torch.int64, device=f0.device)
        idx = f0[ok].reshape(-1).long()
        at.index_add_(0, idx, torch.ones_like(idx))
        fl.index_add_(0, idx, (out[ok] != 0).long()[:, None].expand(-1, 3).reshape(-1))
        neg = (at > 0) & (fl == at)
        rep["n_mixed_normals"] = int(((fl > 0) & (fl < at)).sum())
        nrm = mesh["normals"]
        if torch.is_tensor(nrm):
            result["normals"] = torch.where(neg.to(nrm.device)[:, None], -nrm, nrm)
        else:
            nrm = np.asarray(nrm)
            result["normals"] = np.where(neg.cpu().numpy()[:, None], -nrm, nrm).astype(nrm.dtype)
    return (result, restore_dict(rep, was_numpy, orig)) if return_report else result


def format_report(r):
    lines = [f"faces {r['n_faces']} ({r['n_contributing']} contributing), vertices used {r['n_used_verts']}, edges {r['n_edges']}",
             f"boundary edges {r['n_boundary']} in {r['n_boundary_loops']} loops, non-manifold edges {r['n_nonmanifold']}, "
             f"inconsistent edges {r['n_inconsistent']}",
             f"components (joined across edges) {r['n_components']}, Euler characteristic {r['euler']}",
             f"watertight: {'yes' if r['is_watertight'] else 'no'}   consistently oriented: {'yes' if r['is_oriented'] else 'no'}"]
    if "embedded" in r:
        lines.append(f"pairs of faces meeting properly {r['n_proper_pairs']}: {'embedded' if r['embedded'] else 'NOT embedded'}")
    return lines


def format_orient_report(r):
    return [f"components (joined across two-face edges) {r['n_components']}: {r['n_closed']} closed, {r['n_open']} open, "
            f"{r['n_nonorientable']} not orientable",
            f"outward rule {r['outward']}: {r['n_toggled']} components turned, {r['n_undecided']} undecided",
            f"faces reversed {r['n_flipped']}, vertex normals left at mixed vertices {r['n_mixed_normals']}"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_topology", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--weld", action="store_true", help="name vertices by their coordinates: connect across repeated seam vertices")
    ap.add_argument("--json", action="store_true", help="print the report as one JSON object")
    ap.add_argument("--intersections", action="store_true", help="add n_proper_pairs and embedded (mesh_intersect, DESIGN 4x)")
    ap.add_argument("--split", action="store_true",
                    help="cut the mesh into a 2-manifold first: one vertex per fan of faces (mesh_repair, DESIGN 4y)")
    ap.add_argument("--orient", metavar="OUT.ply", help="write the mesh with a consistent winding (DESIGN 4s) and print that report")
    ap.add_argument("--outward", choices=("volume", "views", "none"), default="volume",
                    help="with --orient: which of the two consistent windings a component gets")
    ap.add_argument("--poses", metavar="P", help="with --outward views: camera-to-world matrices, .npy [n, 4, 4] or text rows of 16")
    ap.add_argument("--intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"))
    a = ap.parse_args(argv)
    if a.orient is not None and a.outward == "views" and (a.poses is None or a.intrinsics is None or a.size is None):
        ap.error("--outward views needs --poses, --intrinsics and --size")
    if a.split and a.weld:
        ap.error("--split and --weld undo each other: the welded names join the vertices that the split made")
    need_gpu("mesh_topology")
    try:
        mesh = read_ply(a.mesh)
        if a.split:
            from .mesh_repair import split_nonmanifold            # (a cycle: mesh_repair is built on this module's edge table)
            mesh = split_nonmanifold(mesh)
        if a.orient is None:
            r = topology(mesh, weld=a.weld, intersections=a.intersections)
        else:
            poses = None
            if a.outward == "views":
                poses = np.load(a.poses) if a.poses.endswith(".npy") else np.loadtxt(a.poses).reshape(-1, 4, 4)
            out, full = orient(mesh, None if a.outward == "none" else a.outward, poses, a.intrinsics, a.size, weld=a.weld,
                               return_report=True)
            write_mesh_ply(a.orient, out)
            r = {k: (x if isinstance(x, (bool, str)) or x is None else int(x)) for k, x in full.items() if np.ndim(x) == 0}
    except (ValueError, OSError) as e:
        print(f"mesh_topology: {e}", file=sys.stderr)
        raise SystemExit(2)
    if a.orient is None:
        print(json.dumps(r) if a.json else "\n".join(format_report(r)))
    else:
        print(json.dumps(r) if a.json else "\n".join(format_orient_report(r) + [f"-> {a.orient}"]))
    return r


if __name__ == "__main__":
    main()
