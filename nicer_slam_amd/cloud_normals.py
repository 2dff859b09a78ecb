"""Normals of a raw point cloud on the device: exact k nearest neighbours and the smallest principal axis of each neighbourhood (DESIGN
4za; C ABI Section 28, csrc/mesh_eval.hip k_nn_query_k and csrc/cloud_normals.hip).

* ``estimate_normals(points, k=30, max_dist=inf, viewpoint=None, queries=None, index=None, info=False)``: open3d's ``estimate_normals``
  with KDTreeSearchParamKNN(k) (``max_dist``: ...ParamHybrid(max_dist, k)) and, with ``viewpoint``, ``orient_normals_towards_camera_location``.
* ``python -m nicer_slam_amd.cloud_normals IN.ply --out OUT.ply [--k K] [--radius R] [--viewpoint x y z] [--json]``

Per row: the k nearest points under the total order (d2, index); their float64 mean and scatter in two passes, summed in that order; the
eigen-decomposition of the 3x3 by cyclic Jacobi with + - * / sqrt alone; the eigenvector of the smallest eigenvalue, oriented and rounded
once to fp32.  The result is the same bits on every run and equals the numpy statement in tests/normals_ref.py bit for bit.

Not built: consistent orientation without a viewpoint (tangent-plane propagation over a spanning tree), radius-only neighbourhoods with
more than 64 members, outlier filters, FPFH.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import json
import math
import sys

import numpy as np
import torch

from ._native import check, lib
from .mesh_args import checked_points, need_gpu, ptr, stream
from .mesh_eval import NNIndex
from .ply import read_ply, write_mesh_ply


def _cloud(x, name, device=None):
    """``checked_points`` for a cloud that may be an array or live on the host: moved to ``device`` first"""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x, np.float32)).reshape(-1, 3)
    if not x.is_cuda:
        x = x.to(device if device is not None else "cuda")
    return checked_points(x, name)


@torch.no_grad()
def normals_from_neighbours(points, idx, count, origin, viewpoint=None, eigenvalues=True):
    """nsa_cloud_normals on CUDA tensors: ``points`` [n, 3] fp32, ``idx`` [m, k] int32 and ``count`` [m] int32 as ``NNIndex._knn`` gives
    them, ``origin`` [m, 3] fp32 the point each row belongs to, ``viewpoint`` None, [3] or [m, 3].  Returns (normals [m, 3] fp32,
    eigenvalues [m, 3] float64 ascending or None, valid [m] bool)."""
    m, k = idx.shape
    dev = points.device
    if idx.dtype != torch.int32 or count.dtype != torch.int32 or count.shape != (m,) or origin.shape != (m, 3):
        raise ValueError("normals_from_neighbours: idx [m, k] and count [m] must be int32, origin [m, 3]")
    rows = 0
    if viewpoint is not None:
        viewpoint = torch.as_tensor(viewpoint).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(viewpoint.shape) == (3,):
            rows = 1
        elif tuple(viewpoint.shape) == (m, 3):
            rows = m
        else:
            raise ValueError(f"estimate_normals: viewpoint must be [3] or [{m}, 3], got {tuple(viewpoint.shape)}")
    normals = torch.empty(m, 3, dtype=torch.float32, device=dev)
    eig = torch.empty(m, 3, dtype=torch.float64, device=dev) if eigenvalues else None
    valid = torch.empty(m, dtype=torch.uint8, device=dev)
    if m:
        check(lib.nsa_cloud_normals(points.data_ptr(), points.shape[0], idx.data_ptr(), count.data_ptr(), m, k, origin.data_ptr(),
                                    viewpoint.data_ptr() if rows else None, rows, normals.data_ptr(), ptr(eig), valid.data_ptr(),
                                    stream(dev)))
    return normals, eig, valid.bool()


@torch.no_grad()
def estimate_normals(points, k=30, max_dist=math.inf, viewpoint=None, queries=None, index=None, info=False):
    """Unit normals [m, 3] fp32 of the cloud ``points`` [n, 3] (array or CUDA tensor, taken as fp32) at its own points, or at ``queries``
    [m, 3]: for each the ``k`` (1 .. 64) nearest points of the cloud (``NNIndex.knn``; with ``max_dist`` only those with d2 <
    fp32(max_dist^2)), and the eigenvector of the smallest eigenvalue of their scatter matrix.  At its own points each point is its own
    first neighbour, as in open3d.  ``index``: a prebuilt ``NNIndex`` of ``points``.
    Orientation: with ``viewpoint`` [3] (or [m, 3], one camera centre per row) the normal is turned towards it, n . (w - p) >= 0; without,
    its component of largest magnitude is made positive (ties: the lowest axis), which is repeatable but not consistent over a surface.
    A row is VALID when it has at least 3 neighbours, its eigenvalues are finite and the middle one is > 0 (the neighbours are not all on
    one line); a row that is not gets the normal (0, 0, 0), which ``icp_point_to_plane`` leaves out.
    ``info=True`` returns (normals, dict(valid [m] bool, eigenvalues [m, 3] float64 ascending, variation [m] = w0 / ((w0 + w1) + w2) -- the
    surface variation, 0 on a plane and 1/3 on an isotropic blob --, count [m] int64, idx [m, k] int64))."""
    need_gpu("estimate_normals")
    dev = index.device if index is not None else None
    pts = _cloud(points, "estimate_normals", dev)
    if pts.shape[0] == 0:
        raise ValueError("estimate_normals: empty cloud")
    if index is None:
        index = NNIndex(pts)
    if not isinstance(index, NNIndex) or index.n != pts.shape[0] or index.device != pts.device:
        raise ValueError("estimate_normals: index must be an NNIndex of the same points on the same device")
    q = pts if queries is None else _cloud(queries, "estimate_normals", pts.device)
    _, idx, count = index._knn(q, k, max_dist, "estimate_normals")
    normals, eig, valid = normals_from_neighbours(pts, idx, count, q, viewpoint, eigenvalues=info)
    if not info:
        return normals
    return normals, dict(valid=valid, eigenvalues=eig, variation=eig[:, 0] / ((eig[:, 0] + eig[:, 1]) + eig[:, 2]), count=count.long(),
                         idx=idx.long())


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.cloud_normals", description=__doc__.splitlines()[0])
    ap.add_argument("input", metavar="IN.ply", help="a cloud (no face element) or a mesh, whose faces are kept")
    ap.add_argument("--out", metavar="OUT.ply", required=True, help="the vertices with nx ny nz and the faces read")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--radius", type=float, default=math.inf, help="only neighbours closer than R")
    ap.add_argument("--viewpoint", type=float, nargs=3, metavar=("x", "y", "z"), help="turn the normals towards this point")
    ap.add_argument("--json", action="store_true", help="print the summary as one JSON object")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("cloud_normals: needs a GPU", file=sys.stderr)
        raise SystemExit(2)
    try:
        ply = read_ply(a.input)
        normals, extra = estimate_normals(ply["verts"], a.k, a.radius, a.viewpoint, info=True)
        write_mesh_ply(a.out, dict(ply, normals=normals))
    except (ValueError, OSError) as e:
        print(f"cloud_normals: {e}", file=sys.stderr)
        raise SystemExit(2)
    valid = extra["valid"]
    r = dict(points=int(valid.numel()), valid=int(valid.sum()), k=a.k,
             mean_variation=float(extra["variation"][valid].mean()) if bool(valid.any()) else None)
    if a.json:
        print(json.dumps(r))
    else:
        print(f"points: {r['points']}  valid normals: {r['valid']}  k: {r['k']}  mean surface variation: {r['mean_variation']}")
    return r


if __name__ == "__main__":
    main()
