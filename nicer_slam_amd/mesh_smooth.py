"""Mesh smoothing on the device: vertex rings, Laplacian / Taubin steps and vertex normals from the faces (C ABI Section 21,
csrc/mesh_smooth.hip).

* ``vertex_ring(faces, n_verts)``: for every vertex its neighbours in ascending index and the edge id of each, in CSR form.
* ``smooth(mesh, method="taubin", iterations=10, lam=0.5, mu=-0.53, boundary="curve", ...)``: the mesh with its vertices smoothed.
  Taubin's lambda / mu pairs take the noise out and keep the volume; plain Laplacian steps shrink.  Float64 between the steps, every
  sum in row order: the result is bit-reproducible and equals the numpy statement in tests/smooth_ref.py bit for bit.
* ``vertex_normals(mesh, weighting="angle")``: unit vertex normals that follow the face winding, angle- or area-weighted -- for a
  smoothed mesh, whose stored normals are stale, or a PLY without normals.
* ``python -m nicer_slam_amd.mesh_smooth IN.ply --out OUT.ply [--method taubin|laplacian] [--iterations N] [--lam L] [--mu M]
  [--boundary free|fixed|curve] [--max-move D] [--normals angle|area|keep|none] [--json]``

Smoothing is BY INDEX: two vertices are neighbours when a face lists both.  A mesh whose seams repeat vertices (one copy per face or
per patch) tears along the seams; welding is out of scope here (``mesh_eval.welded_faces`` names coincident vertices, it does not merge
them).  The marching-cubes meshes of this package are indexed.

numpy in, numpy out; torch in, torch out on the caller's device.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import ctypes
import json
import math
import sys

import torch

from . import _native
from ._native import lib, check
from .mesh_args import MAX_FACES_RINGS, checked_mesh, cuda_faces, need_gpu, ptr, stream, workspace
from .mesh_topology import _edge_table
from .ply import read_ply, write_mesh_ply

METHODS = ("taubin", "laplacian")
BOUNDARY = {"free": _native.SMOOTH_FREE, "fixed": _native.SMOOTH_FIXED, "curve": _native.SMOOTH_CURVE}
WEIGHTING = {"area": _native.NORMALS_AREA, "angle": _native.NORMALS_ANGLE}
NORMALS = ("angle", "area", "keep", None)
STATE_LIVE, STATE_ON_BOUNDARY, STATE_MOVES, STATE_STEPS = 1, 2, 4, 8


@torch.no_grad()
def _ring(t, V, F, dev):
    """the full-size device arrays of nsa_mesh_ring from the full-size edge table ``t`` of ``mesh_topology._edge_table``"""
    ring_start = torch.zeros(V + 1, dtype=torch.int32, device=dev)
    ring = torch.empty(6 * F, dtype=torch.int32, device=dev)
    ring_edge = torch.empty(6 * F, dtype=torch.int32, device=dev)
    if F:
        ws = workspace(lib.nsa_mesh_ring_workspace(V, F), dev)
        check(lib.nsa_mesh_ring(t["edges"].data_ptr(), t["_totals"].data_ptr(), V, F, ws.data_ptr(), ring_start.data_ptr(),
                                ring.data_ptr(), ring_edge.data_ptr(), stream(dev)))
    return ring_start, ring, ring_edge


def vertex_ring(faces, n_verts):
    """The vertex rings of ``faces`` [F, 3] (int32 or int64) over ``n_verts`` vertices (header Section 21), a dict of tensors (arrays
    for numpy faces): ``ring_start`` [V + 1], ``ring`` [2 E] the neighbours of vertex v at ``ring_start[v]:ring_start[v + 1]`` in
    ascending index, ``ring_edge`` [2 E] the edge id of each entry in ``mesh_topology.edge_table``'s numbering, all int32 -- plus that
    table's totals as ints (``n_edges``, ``n_boundary``, ...).  Reads the totals back once (a synchronisation)."""
    f, V, F, _, restore = cuda_faces(faces, n_verts, None, "vertex_ring", max_faces=MAX_FACES_RINGS)
    t, totals = _edge_table(f, V, F, None)
    ring_start, ring, ring_edge = _ring(t, V, F, f.device)
    n = 2 * totals["n_edges"]
    out = dict(ring_start=restore(ring_start), ring=restore(ring[:n]), ring_edge=restore(ring_edge[:n]))
    out.update(totals)
    return out


@torch.no_grad()
def _smooth(v, V, F, t, rings, factors, boundary, fixed, max_move):
    """nsa_mesh_smooth on device arrays: (out fp32 [V, 3], state uint8 [V])"""
    dev = v.device
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    state = torch.zeros(V, dtype=torch.uint8, device=dev)
    if V == 0:
        return out, state
    n = len(factors)
    fac = (ctypes.c_double * max(n, 1))(*factors)
    ws = workspace(lib.nsa_mesh_smooth_workspace(V, F), dev)
    ring_start, ring, ring_edge = rings
    no_faces = lambda x: x.data_ptr() if F else None        # (NULL without faces, though ring_start is never empty)
    check(lib.nsa_mesh_smooth(v.data_ptr(), V, F, no_faces(ring_start), ptr(ring), ptr(ring_edge), ptr(t["edge_count"]),
                              ptr(fixed), fac, n, BOUNDARY[boundary],
                              math.inf if max_move is None else float(max_move), ws.data_ptr(), out.data_ptr(), state.data_ptr(),
                              stream(dev)))
    return out, state


@torch.no_grad()
def _vertex_normals(v, f, V, F, weighting):
    out = torch.empty(V, 3, dtype=torch.float32, device=v.device)
    if V == 0:
        return out
    ws = workspace(lib.nsa_mesh_vertex_normals_workspace(V, F), v.device) if F else None
    check(lib.nsa_mesh_vertex_normals(v.data_ptr(), V, ptr(f), F, WEIGHTING[weighting], ws.data_ptr() if F else None, out.data_ptr(),
                                      stream(v.device)))
    return out


def factors_of(method="taubin", iterations=10, lam=0.5, mu=-0.53):
    """the list of step factors: ``lam`` repeated (laplacian) or ``lam, mu`` pairs (taubin), after checking them"""
    if method not in METHODS:
        raise ValueError(f"smooth: method must be one of {METHODS}, got {method!r}")
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0 or iterations >= 1 << 30:
        raise ValueError(f"smooth: iterations must be a count, got {iterations!r}")
    lam = float(lam)
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"smooth: 0 < lam <= 1, got {lam!r}")
    if method == "laplacian":
        return [lam] * int(iterations)
    mu = float(mu)
    if not -1.0 <= mu < -lam:
        raise ValueError(f"smooth: -1 <= mu < -lam for taubin (mu = {mu!r}, lam = {lam!r}): the pair must inflate more than it shrank")
    return [lam, mu] * int(iterations)


def smooth(mesh, method="taubin", iterations=10, lam=0.5, mu=-0.53, boundary="curve", fixed=None, max_move=None, normals="angle",
           return_report=False, device="cuda"):
    """``mesh`` (a dict with ``verts`` [V, 3] and ``faces`` [F, 3], numpy or torch) with its vertices smoothed: a new dict of the same
    kind with the same faces.  Header Section 21 states every operation.
      method      "taubin": ``iterations`` pairs of a ``lam`` step and a ``mu`` step (0 < lam <= 1, -1 <= mu < -lam), which keeps the
                  volume (Taubin, "A signal processing approach to fair surface design", 1995); "laplacian": ``iterations`` steps of
                  ``lam``, which shrinks.  A step moves a vertex by the factor times (mean of its neighbours - itself).
      boundary    "curve": a vertex on a boundary edge is smoothed along the boundary edges only; "fixed": it stays; "free": it moves
                  like any other (and the rim creeps inward).
      fixed       [V] mask (anything non-zero holds the vertex) or None.
      max_move    None, or the largest move per component from the INPUT position: the result is clamped to that box at every step.
      normals     "angle" / "area": ``vertex_normals`` of the smoothed mesh; "keep": the input's, when it has any; None: dropped.
    ``colors`` and every other key pass through untouched.  A vertex that is not finite, lies on no face, is held, or has no finite
    neighbour is returned bit for bit.  ``return_report=True`` appends a dict: ``n_steps``, ``n_live`` (finite, on a face),
    ``n_moving``, ``n_boundary``, ``n_held`` (live and not moving) and ``max_move`` (the largest change of a component).
    Smoothing is by index: see the module docstring about seams."""
    factors = factors_of(method, iterations, lam, mu)
    if boundary not in BOUNDARY:
        raise ValueError(f"smooth: boundary must be one of {tuple(BOUNDARY)}, got {boundary!r}")
    if normals not in NORMALS:
        raise ValueError(f"smooth: normals must be one of {NORMALS}, got {normals!r}")
    if max_move is not None and not float(max_move) > 0.0:
        raise ValueError(f"smooth: max_move must be positive, got {max_move!r}")
    if not isinstance(mesh, dict) or "verts" not in mesh:
        raise ValueError("smooth: mesh needs 'verts' and 'faces'")
    mask = None
    if fixed is not None:
        mask = torch.as_tensor(fixed).reshape(-1)
        if mask.shape[0] != mesh["verts"].shape[0]:
            raise ValueError(f"smooth: fixed mask of {mask.shape[0]} for {mesh['verts'].shape[0]} vertices")
    v, f, V, F, _, give = checked_mesh(mesh, "smooth", device, float_verts=True, max_faces=MAX_FACES_RINGS)
    if mask is not None:
        mask = (mask.to(v.device) != 0).to(torch.uint8).contiguous()
    t, _ = _edge_table(f, V, F, None)
    out, state = _smooth(v, V, F, t, _ring(t, V, F, v.device), factors, boundary, mask, max_move)
    result = dict(mesh)
    result["verts"] = give(out)
    if normals in WEIGHTING:
        result["normals"] = give(_vertex_normals(out, f, V, F, normals))
    elif normals is None:
        result.pop("normals", None)
    if not return_report:
        return result
    bit = lambda b: int(((state & b) != 0).sum())
    steps = (state & STATE_STEPS) != 0
    moved = (out - v).abs()[steps]
    report = dict(n_verts=V, n_steps=len(factors), n_live=bit(STATE_LIVE), n_moving=bit(STATE_STEPS), n_boundary=bit(STATE_ON_BOUNDARY),
                  n_held=bit(STATE_LIVE) - bit(STATE_STEPS), max_move=float(moved.max()) if moved.numel() else 0.0)
    return result, report


def vertex_normals(mesh, weighting="angle", device="cuda"):
    """[V, 3] float32 unit vertex normals of ``mesh`` from its faces (header Section 21): at every corner the cross product of the
    edges to the next and to the previous vertex of the face -- so the normals follow the winding, ``mesh_eval``'s face-normal
    convention, and on this package's marching-cubes meshes point towards increasing value like the stored ones -- added per vertex
    in ascending corner order, weighted by the corner's angle ("angle") or by the face's area ("area"), and normalised.  The zero
    vector for a vertex on no face with finite vertices.  Same kind (numpy or torch, device) as the mesh's verts."""
    if weighting not in WEIGHTING:
        raise ValueError(f"vertex_normals: weighting must be one of {tuple(WEIGHTING)}, got {weighting!r}")
    v, f, V, F, _, give = checked_mesh(mesh, "vertex_normals", device, float_verts=True, max_faces=MAX_FACES_RINGS)
    return give(_vertex_normals(v, f, V, F, weighting))


def format_report(r):
    return [f"vertices {r['n_verts']}: {r['n_live']} live, {r['n_moving']} moving, {r['n_held']} held, {r['n_boundary']} on the boundary",
            f"steps {r['n_steps']}, largest move of a component {r['max_move']:.6g}"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_smooth", description=__doc__.splitlines()[0])
    ap.add_argument("mesh", metavar="IN.ply")
    ap.add_argument("--out", required=True, metavar="OUT.ply")
    ap.add_argument("--method", choices=METHODS, default="taubin")
    ap.add_argument("--iterations", type=int, default=10, help="lambda steps (laplacian) or lambda / mu pairs (taubin)")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--boundary", choices=tuple(BOUNDARY), default="curve")
    ap.add_argument("--max-move", type=float, default=None, help="largest move per component from the input position")
    ap.add_argument("--normals", choices=("angle", "area", "keep", "none"), default="angle")
    ap.add_argument("--json", action="store_true", help="print the report as one JSON object")
    a = ap.parse_args(argv)
    need_gpu("mesh_smooth")
    try:
        mesh = read_ply(a.mesh)
        out, r = smooth(mesh, a.method, a.iterations, a.lam, a.mu, a.boundary, None, a.max_move,
                        None if a.normals == "none" else a.normals, return_report=True)
        write_mesh_ply(a.out, out)
    except (ValueError, OSError) as e:
        print(f"mesh_smooth: {e}", file=sys.stderr)
        raise SystemExit(2)
    print(json.dumps(r) if a.json else "\n".join(format_report(r) + [f"-> {a.out}"]))
    return r


if __name__ == "__main__":
    main()
