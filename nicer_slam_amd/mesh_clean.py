"""Mesh clean-up on the device: the steps code/evaluation/eval_rec.py:259-272 leaves to a person with Meshlab and to a file from
the trajectory evaluation.

* ``components`` / ``component_stats``: connected components of a triangle mesh by shared vertex index and their face count,
  vertex count, area and bounding box (C ABI Section 11, csrc/mesh_clean.hip).
* ``keep_components``: keep the largest component (code/utils/viz.py:136-141), or the components that touch / do not touch a box
  (Meshlab's "select connected components in a region", delete: eval_rec.py:269).
* ``select_faces``: the compaction behind it; order-preserving, so a cleaned mesh is a function of its input.
* ``transform_mesh``: a 4x4 similarity applied to vertices and normals (alignment_transformation_sim3.npy, eval_rec.py:259-264).
* ``python -m nicer_slam_amd.mesh_clean IN.ply --out OUT.ply [--keep ...] [--transform T.npy] [--list]``.

Departure from trimesh's ``split``: faces that share a vertex are joined, not only faces that share an edge;
``keep_components(..., connectivity="edge")`` takes the edge rule from mesh_topology.
Labelling and statistics have no CPU path: a missing GPU is an error.  ``select_faces`` and ``transform_mesh`` are torch
plumbing and run wherever their input lives.
"""
import argparse
import sys

import numpy as np
import torch

from . import mesh_topology
from ._native import lib, check
from .mesh_args import PER_VERTEX, checked_faces, mesh_dict_tensors, need_gpu, ptr, restore_dict, stream, workspace
from .mesh_eval import _transform
from .ply import read_ply, write_mesh_ply

KEEP_MODES = ("largest", "touching", "not_touching")
CONNECTIVITY = ("vertex", "edge")


@torch.no_grad()
def components(faces, n_verts):
    """(vertex_label [V] int32, face_label [F] int32, n_components, n_referenced) of the mesh ``faces`` [F, 3] (CUDA, int32 or
    int64) over ``n_verts`` vertices.  Faces that share a vertex index are connected; the label of a component is its smallest
    vertex index; a vertex no valid face uses and a face with an index outside [0, n_verts) get -1.  Reads the three totals
    back once (a synchronisation)."""
    f = checked_faces(faces, "components", require_cuda=True, n_verts=n_verts).to(torch.int32).contiguous()
    V, F, dev = int(n_verts), f.shape[0], f.device
    vl = torch.empty(V, dtype=torch.int32, device=dev)
    fl = torch.empty(F, dtype=torch.int32, device=dev)
    if V == 0 and F == 0:
        return vl, fl, 0, 0
    ws = workspace(max(1, lib.nsa_mesh_components_workspace(V)), dev)
    totals = torch.empty(3, dtype=torch.int64, device=dev)
    check(lib.nsa_mesh_components(ptr(f), F, V, ws.data_ptr(), ptr(vl), ptr(fl), totals.data_ptr(), stream(dev)))
    C, R, status = (int(x) for x in totals.cpu())
    if status != 0:
        raise RuntimeError(f"components: the labelling kernel left its loop on a step cap (status {status}); this is a bug")
    return vl, fl, C, R


@torch.no_grad()
def component_stats(verts, faces):
    """Per-component table of the mesh (CUDA ``verts`` [V, 3], ``faces`` [F, 3]) in ascending label order, as device tensors:
    ``label`` [C] int32, ``n_faces`` [C] int32, ``n_verts`` [C] int32, ``area`` [C] float64, ``lo`` / ``hi`` [C, 3] float32, and
    the per-element ranks ``vertex_comp`` [V], ``face_comp`` [F] int32 (-1: no component); ``n_components`` = C as an int."""
    if not (torch.is_tensor(verts) and verts.is_cuda and verts.dim() == 2 and verts.shape[1] == 3):
        raise ValueError("component_stats: verts must be a CUDA tensor [V, 3]")
    v = verts.detach().float().contiguous()
    f = checked_faces(faces, "component_stats", require_cuda=True).to(torch.int32).contiguous()
    V, F, dev = v.shape[0], f.shape[0], v.device
    if f.device != dev:
        raise ValueError("component_stats: verts and faces on different devices")
    vl, fl, C, _ = components(f, V)
    out = dict(label=torch.empty(C, dtype=torch.int32, device=dev), n_faces=torch.empty(C, dtype=torch.int32, device=dev),
               n_verts=torch.empty(C, dtype=torch.int32, device=dev), area=torch.empty(C, dtype=torch.float64, device=dev),
               lo=torch.empty(C, 3, device=dev), hi=torch.empty(C, 3, device=dev),
               vertex_comp=torch.full((V,), -1, dtype=torch.int32, device=dev),
               face_comp=torch.full((F,), -1, dtype=torch.int32, device=dev), n_components=C)
    if V == 0:
        return out
    ws = workspace(max(1, lib.nsa_mesh_component_stats_workspace(V, F, C)), dev)
    check(lib.nsa_mesh_component_stats(v.data_ptr(), V, ptr(f), F, vl.data_ptr(), ptr(fl), C, ws.data_ptr(), ptr(out["label"]),
                                       ptr(out["n_faces"]), ptr(out["n_verts"]), ptr(out["area"]), ptr(out["lo"]), ptr(out["hi"]),
                                       out["vertex_comp"].data_ptr(), ptr(out["face_comp"]), stream(dev)))
    return out


@torch.no_grad()
def select_faces(mesh, face_mask):
    """The mesh of the faces where ``face_mask`` [F] is set: the kept faces in their original order, the vertices some kept
    face uses in their original order, faces re-indexed, every per-vertex entry (``verts``, ``normals``, ``colors``) carried.
    numpy in, numpy out; torch in, torch out on the same device."""
    m, was_numpy, dev = mesh_dict_tensors(mesh)
    f = m["faces"]
    mask = torch.as_tensor(face_mask, device=f.device).bool().reshape(-1)
    V = m["verts"].shape[0]
    if mask.shape[0] != f.shape[0]:
        raise ValueError(f"select_faces: mask of {mask.shape[0]} for {f.shape[0]} faces")
    kept = f[mask].long()
    if kept.numel() and (int(kept.min()) < 0 or int(kept.max()) >= V):
        raise ValueError("select_faces: a kept face has an index outside [0, V)")
    used = torch.zeros(V, dtype=torch.bool, device=f.device)
    used[kept.reshape(-1)] = True
    remap = torch.cumsum(used.long(), 0) - 1
    out = dict(m)
    out["faces"] = remap[kept].to(f.dtype)
    for k in PER_VERTEX:
        if k in m:
            out[k] = m[k][used]
    return restore_dict(out, was_numpy, dev)


def _region(region):
    if region is None:
        raise ValueError("keep_components: this selection needs region=(lo, hi)")
    lo, hi = (np.asarray(x, dtype=np.float64).reshape(-1) for x in region)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (lo > hi).any():
        raise ValueError("keep_components: region must be two finite corners (lo, hi) with lo <= hi")
    return lo, hi


@torch.no_grad()
def keep_components(mesh, keep="largest", region=None, device="cuda", connectivity="vertex"):
    """(mesh, stats): the components of ``mesh`` (a dict as marching_cubes / extract_mesh / TSDFVolume.extract_mesh / read_ply
    give, numpy or torch) selected by ``keep``, compacted with ``select_faces``:
      "largest"       the component of greatest area, ties to the smallest label
      "touching"      with region=(lo, hi): the components with at least one vertex inside the closed box
      "not_touching"  the others
    ``stats`` is the ``component_stats`` table of the input plus ``kept`` [C] bool and ``kept_area_fraction``.
    ``connectivity="edge"``: a component is a set of faces joined across shared EDGES (mesh_topology.face_components; trimesh's
    ``split``), not at shared vertices.  The table is then that of the mesh in which every vertex has been duplicated once per
    edge-joined component that uses it (mesh_topology.split_faces), on which the two rules coincide: ``label`` and ``vertex_comp``
    refer to that mesh's vertices (the original indices when no vertex is shared between components), ``n_verts`` counts a pinch
    vertex once per component, and a face with a repeated index belongs to no component and is dropped.  The returned mesh is the
    selection applied to the ORIGINAL mesh: a pinch vertex two kept components share stays one vertex.
    An empty mesh or a selection that keeps nothing raises ValueError."""
    if keep not in KEEP_MODES:
        raise ValueError(f"keep_components: keep must be one of {KEEP_MODES}, got {keep!r}")
    if connectivity not in CONNECTIVITY:
        raise ValueError(f"keep_components: connectivity must be one of {CONNECTIVITY}, got {connectivity!r}")
    if keep != "largest":
        lo, hi = _region(region)
    need_gpu("keep_components")
    m, was_numpy, orig = mesh_dict_tensors(mesh, device)
    if m["verts"].shape[0] == 0 or m["faces"].shape[0] == 0:
        raise ValueError("keep_components: empty mesh")
    sv, sf = m["verts"], m["faces"]                            # the mesh the table is of
    if connectivity == "edge":
        f32 = checked_faces(sf, "keep_components", require_cuda=True).to(torch.int32).contiguous()
        label, _ = mesh_topology.face_components(f32, sv.shape[0])
        sf, origin = mesh_topology.split_faces(f32, label, sv.shape[0])
        sv = sv[origin]
    st = component_stats(sv, sf)
    C = st["n_components"]
    if C == 0:
        raise ValueError("keep_components: no valid face")
    dev = m["verts"].device
    if keep == "largest":
        area = st["area"]
        best = int((area == area.max()).nonzero()[0])            # ranks ascend with the label: the first is the smallest label
        kept = torch.zeros(C, dtype=torch.bool, device=dev)
        kept[best] = True
    else:
        v = sv.double()
        inside = ((v >= torch.tensor(lo, device=dev)) & (v <= torch.tensor(hi, device=dev))).all(1)
        vc = st["vertex_comp"].long()
        hit = torch.zeros(C, dtype=torch.bool, device=dev)
        hit[vc[inside & (vc >= 0)]] = True
        kept = hit if keep == "touching" else ~hit
    if not bool(kept.any()):
        raise ValueError(f"keep_components: the selection {keep!r} keeps nothing")
    fc = st["face_comp"].long()
    mask = (fc >= 0) & kept[fc.clamp_min(0)]
    out = select_faces(m, mask)
    st["kept"] = kept
    total = float(st["area"].sum())
    st["kept_area_fraction"] = float(st["area"][kept].sum()) / total if total > 0 else float("nan")
    return restore_dict(out, was_numpy, orig), st


def check_similarity(T, tol=1e-6):
    """(s, T float64 [4, 4]) for a 4x4 whose linear part is s * R, s > 0, R a rotation, within ``tol``; ValueError otherwise."""
    T = np.asarray(T.cpu() if torch.is_tensor(T) else T, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("transform: needs a finite 4x4 matrix")
    if np.abs(T[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > tol:
        raise ValueError("transform: the last row must be (0, 0, 0, 1)")
    A = T[:3, :3]
    det = np.linalg.det(A)
    if not det > 0:
        raise ValueError("transform: the linear part is singular or a reflection")
    s = det ** (1.0 / 3.0)
    if np.abs(A @ A.T / (s * s) - np.eye(3)).max() > tol:
        raise ValueError("transform: the linear part is not a positive multiple of a rotation")
    return s, T


@torch.no_grad()
def transform_mesh(mesh, T):
    """``mesh`` moved by the similarity ``T`` (4x4, T[:3, :3] = s R): vertices through mesh_eval._transform in float64, rounded
    once to fp32; normals multiplied by T[:3, :3] and normalised again (zero stays zero); everything else carried.  A ``T``
    whose linear part is not a positive multiple of a rotation within 1e-6 raises ValueError."""
    _, T = check_similarity(T)
    m, was_numpy, dev = mesh_dict_tensors(mesh)
    out = dict(m)
    Tt = torch.from_numpy(T).to(m["verts"].device)
    out["verts"] = _transform(m["verts"].double(), Tt).float()
    if "normals" in m:
        Z = torch.zeros(4, 4, dtype=torch.float64, device=Tt.device)
        Z[:3, :3] = Tt[:3, :3]
        n = _transform(m["normals"].double(), Z)
        length = n.norm(dim=-1, keepdim=True)
        out["normals"] = torch.where(length > 0, n / length.clamp_min(1e-300), torch.zeros_like(n)).float()
    return restore_dict(out, was_numpy, dev)


def format_table(stats):
    """the component table, largest area first (ties: smallest label), as text lines"""
    area = stats["area"].cpu().numpy()
    order = sorted(range(len(area)), key=lambda c: (-area[c], c))
    lab, nf, nv = (stats[k].cpu().numpy() for k in ("label", "n_faces", "n_verts"))
    lo, hi = stats["lo"].cpu().numpy(), stats["hi"].cpu().numpy()
    lines = [f"{len(area)} components", f"{'label':>10} {'faces':>10} {'vertices':>10} {'area':>14}  box"]
    for c in order:
        box = " ".join(f"{x:.4f}" for x in lo[c]) + " .. " + " ".join(f"{x:.4f}" for x in hi[c])
        lines.append(f"{lab[c]:>10} {nf[c]:>10} {nv[c]:>10} {area[c]:>14.6f}  {box}")
    return lines


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_clean", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--out")
    ap.add_argument("--keep", choices=KEEP_MODES)
    ap.add_argument("--region", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--connectivity", choices=CONNECTIVITY, default="vertex",
                    help="with --keep: faces joined at a shared vertex (the default) or only across a shared edge")
    ap.add_argument("--transform", metavar="T.npy", help="4x4 similarity applied before the selection")
    ap.add_argument("--list", action="store_true", help="print the component table and write nothing")
    a = ap.parse_args(argv)
    if a.keep in ("touching", "not_touching") and a.region is None:
        ap.error(f"--keep {a.keep} needs --region")
    if a.region is not None and a.keep not in ("touching", "not_touching"):
        ap.error("--region goes with --keep touching or not_touching")
    if not a.list and not a.out:
        ap.error("--out is required unless --list is given")
    if not a.list and a.keep is None and a.transform is None:
        ap.error("nothing to do: give --keep, --transform or --list")
    return a


def main(argv=None):
    a = parse_args(argv)
    try:
        mesh = read_ply(a.mesh)
        if a.transform:
            mesh = transform_mesh(mesh, np.load(a.transform))
        if a.list:
            st = component_stats(torch.from_numpy(mesh["verts"]).cuda(), torch.from_numpy(mesh["faces"]).cuda())
            print("\n".join(format_table(st)))
            return st
        if a.keep:
            region = (a.region[:3], a.region[3:]) if a.region else None
            mesh, st = keep_components(mesh, a.keep, region, connectivity=a.connectivity)
            print(f"{st['n_components']} components, kept {int(st['kept'].sum())} "
                  f"({st['kept_area_fraction'] * 100:.2f} % of the area): {mesh['verts'].shape[0]} vertices, "
                  f"{mesh['faces'].shape[0]} faces")
    except (ValueError, OSError) as e:
        print(f"mesh_clean: {e}", file=sys.stderr)
        raise SystemExit(2)
    write_mesh_ply(a.out, mesh)
    return mesh


if __name__ == "__main__":
    main()
