"""Point-to-plane registration on the device: ICP against a cloud with normals or against a mesh's surface itself (C ABI
Section 27, csrc/mesh_register.hip).

* ``icp_point_to_plane(source, target, normals=None, max_corr=0.1, ...)``: open3d's registration_icp with
  TransformationEstimationPointToPlane (Chen & Medioni 1992) and an optional RobustKernel.  ``target`` with ``normals`` is a cloud
  (correspondences from ``mesh_eval.NNIndex``); a mesh dict, a ``(verts, faces)`` pair or a ``mesh_eval.TriIndex`` is a SURFACE: every
  source point is matched with its exact closest point on the mesh and that face's normal (``TriIndex.query(max_dist=max_corr)``), which
  takes the sample spacing of the target out of the result.
* ``plane_system(cur, ...)``: one iteration's 6x6 normal equations from given correspondences -- the thirty float64 sums and two counts
  of header Section 27.
* ``python -m nicer_slam_amd.mesh_register SRC.ply TGT.ply [--metric plane|surface] [--max-corr D] [--kernel l2|huber:K|tukey:K]
  [--estimate-normals [K]] [--init T.npy] [--out-transform T.npy] [--out MOVED.ply] [--json]``

Every sum runs in float64 in an order that depends on the number of rows alone, every operation rounded on its own; the 6x6 solve
is plain float64 arithmetic on the host in a stated order.  The result is the same bits on every run and equals the numpy statement in
tests/register_ref.py bit for bit.  Per iteration: one launch that moves the source, one query, the system's two launches (one more
above 2^20 rows) and one readback of 32 words.

Not built: a scale together with point-to-plane (``mesh_eval.icp_point_to_point(with_scaling=True)`` estimates one), symmetric and
coloured ICP.  A raw cloud's normals come from ``cloud_normals.estimate_normals`` (``normals="estimate"``, ``--estimate-normals``), a
mesh's from ``mesh_smooth.vertex_normals``.  There is no CPU path: a missing GPU is an error.
"""
import argparse
import ctypes
import json
import math
import sys

import numpy as np
import torch

from . import _native
from ._native import check, lib
from .cloud_normals import estimate_normals
from .mesh_args import as_tensor, checked_points, cuda_verts_faces, max_d2, need_gpu, ptr, stream, workspace
from .mesh_eval import NNIndex, TriIndex, _transform
from .mesh_smooth import vertex_normals
from .ply import read_ply, write_mesh_ply

_KERNEL_CODE = {name: code for code, name in enumerate(_native.ICP_KERNELS)}


def _kernel(kernel):
    """(code, k) of "l2" | ("huber", k) | ("tukey", k)"""
    if kernel == "l2":
        return _KERNEL_CODE["l2"], 0.0
    if isinstance(kernel, (tuple, list)) and len(kernel) == 2 and kernel[0] in ("huber", "tukey"):
        k = float(kernel[1])
        if k > 0 and math.isfinite(k):
            return _KERNEL_CODE[kernel[0]], k
    raise ValueError(f"kernel must be 'l2', ('huber', k) or ('tukey', k) with k > 0, got {kernel!r}")


def _cuda(x, dtype, device="cuda"):
    # (not mesh_args.checked_points: any dtype and shape, cast and moved; the callers check the shapes against each other)
    x = as_tensor(x)
    return x.detach().to(device=device if not x.is_cuda else x.device, dtype=dtype).contiguous()


# ---- the host step ----------------------------------------------------------------------------------------------------------------

def ldlt_solve(A, b):
    """x of the 6x6 system A x = b by LDL^T without pivoting in plain float64, or None when a pivot is not > 2^-40 A_jj: the system is
    DEGENERATE (the correspondences leave a motion free -- one plane, two planes, a sphere -- or there are none).  Column by column:
    v_k = L_jk D_k, D_j = A_jj - sum_k L_jk v_k and L_ij = (A_ij - sum_k L_ik v_k) / D_j, each sum subtracted term by term for k
    ascending; then L y = b forwards, z = y / D, L^T x = z backwards, k ascending in every row."""
    A = [[float(A[i][j]) for j in range(6)] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        v = [L[j][k] * D[k] for k in range(j)]
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * v[k]
        if not d > 2.0 ** -40 * A[j][j]:
            return None
        D[j] = d
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * v[k]
            L[i][j] = s / d
    y = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    z = [y[i] / D[i] for i in range(6)]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = z[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x


def update_matrix(x):
    """open3d's TransformVector6dToMatrix4d: R = Rz(x_2) Ry(x_1) Rx(x_0), t = x_3..5"""
    ca, sa, cb, sb, cc, sc = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    return np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, x[3]],
                     [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def _matmul4(U, T):
    """U T with out_ij = ((U_i0 T_0j + U_i1 T_1j) + U_i2 T_2j) + U_i3 T_3j"""
    return ((U[:, 0:1] * T[0] + U[:, 1:2] * T[1]) + U[:, 2:3] * T[2]) + U[:, 3:4] * T[3]


# ---- the device calls -------------------------------------------------------------------------------------------------------------

def _move(cur, upd, cur32):
    """nsa_icp_transform: cur [n, 3] float64 moved in place by the 4x4 ``upd``, its fp32 rounding into cur32"""
    m = (ctypes.c_double * 16)(*np.asarray(upd, np.float64).reshape(16).tolist())
    check(lib.nsa_icp_transform(cur.data_ptr(), cur.shape[0], m, cur32.data_ptr(), stream(cur.device)))


class _System:
    """the buffers of nsa_icp_plane_system for n rows, made once per registration"""

    def __init__(self, n, device):
        self.n = n
        self.ws = workspace(lib.nsa_icp_plane_system_workspace(n), device)
        self.out = torch.zeros(32, dtype=torch.int64, device=device)        # 30 float64 sums, then 2 counts

    def run(self, cur, mode, corr, cloud, surface, code, k):
        dist, targets, normals = cloud if cloud else (None, None, None)
        d2, closest, verts, faces = surface if surface else (None, None, None, None)
        check(lib.nsa_icp_plane_system(cur.data_ptr(), self.n, mode, corr.data_ptr(), ptr(dist), ptr(targets), ptr(normals),
                                       targets.shape[0] if cloud else 0, ptr(d2), ptr(closest), ptr(verts),
                                       verts.shape[0] if surface else 0, ptr(faces), faces.shape[0] if surface else 0, code, k,
                                       self.ws.data_ptr(), self.out.data_ptr(), self.out.data_ptr() + 240, stream(cur.device)))

    def read(self):
        """the one readback: dict(sums [30], k_corr, k_used, A [6, 6], b [6])"""
        h = self.out.cpu().numpy()
        S = h[:30].view(np.float64).copy()
        A = np.zeros((6, 6))
        s = 0
        for i in range(6):
            for j in range(i, 6):
                A[i, j] = A[j, i] = S[s]
                s += 1
        return dict(sums=S, k_corr=int(h[30]), k_used=int(h[31]), A=A, b=-S[21:27])


@torch.no_grad()
def plane_system(cur, kernel="l2", idx=None, dist=None, targets=None, normals=None, face_idx=None, d2=None, closest=None, verts=None,
                 faces=None, device="cuda"):
    """The normal equations of one point-to-plane iteration from given correspondences (header Section 27), arrays or tensors.
    ``cur`` [n, 3] float64, the moved source.  Cloud mode: ``idx`` [n] (< 0: none) and ``dist`` [n] fp32 as ``NNIndex.query`` gives them,
    ``targets`` and ``normals`` [m, 3] fp32.  Surface mode: ``face_idx`` [n] (< 0: none), ``d2`` [n] float64 and ``closest`` [n, 3] fp32 as
    ``TriIndex.query(squared=True)`` gives them, ``verts`` and ``faces`` of the mesh.  Returns dict(A [6, 6], b [6], sums [30], k_corr,
    k_used), numpy float64 and ints: A x = b is the update's system, sums the thirty sums in the header's slots."""
    code, k = _kernel(kernel)
    if (idx is None) == (face_idx is None):
        raise ValueError("plane_system: give idx (cloud mode) or face_idx (surface mode)")
    cur = _cuda(cur, torch.float64, device)
    if cur.dim() != 2 or cur.shape[1] != 3 or cur.shape[0] >= 1 << 31:
        raise ValueError(f"plane_system: cur must be [n, 3] with n < 2^31, got {tuple(cur.shape)}")
    n, dev = cur.shape[0], cur.device
    if n == 0:
        raise ValueError("plane_system: no rows")
    cloud = surface = None
    if idx is not None:
        corr = _cuda(idx, torch.int32, dev)
        cloud = (_cuda(dist, torch.float32, dev), _cuda(targets, torch.float32, dev).reshape(-1, 3), _cuda(normals, torch.float32, dev).reshape(-1, 3))
        if cloud[0].shape != (n,) or cloud[1].shape != cloud[2].shape:
            raise ValueError("plane_system: dist must be [n], targets and normals [m, 3]")
    else:
        corr = _cuda(face_idx, torch.int32, dev)
        surface = (_cuda(d2, torch.float64, dev), _cuda(closest, torch.float32, dev), _cuda(verts, torch.float32, dev).reshape(-1, 3),
                   _cuda(faces, torch.int32, dev).reshape(-1, 3))
        if surface[0].shape != (n,) or surface[1].shape != (n, 3):
            raise ValueError("plane_system: d2 must be [n], closest [n, 3]")
    if corr.shape != (n,):
        raise ValueError("plane_system: one correspondence per row")
    sys_ = _System(n, dev)
    sys_.run(cur, _native.ICP_CLOUD if cloud else _native.ICP_SURFACE, corr, cloud, surface, code, k)
    return sys_.read()


def _is_mesh_pair(t):
    return isinstance(t, (tuple, list)) and len(t) == 2 and len(getattr(t[1], "shape", ())) == 2 and t[1].shape[1] == 3 and (
        t[1].dtype in (torch.int32, torch.int64) if torch.is_tensor(t[1]) else np.asarray(t[1]).dtype.kind in "iu")


@torch.no_grad()
def icp_point_to_plane(source, target, normals=None, max_corr=0.1, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, kernel="l2",
                       index=None):
    """open3d's registration_icp(source, target, max_corr, init, TransformationEstimationPointToPlane(kernel)) with
    ICPConvergenceCriteria(rel_fitness, rel_rmse, max_iter).  ``source`` [n, 3] (array or CUDA tensor; taken as fp32 and moved in float64).
    ``target``: points [m, 3] with ``normals`` [m, 3] -- CLOUD mode, correspondences from an ``NNIndex`` by ``icp_point_to_point``'s rule
    (the nearest target with d2 < fp32(max_corr^2)) -- or a mesh dict, a ``(verts, faces)`` pair or a ``TriIndex`` -- SURFACE mode: each
    source point's closest point ON the mesh and that face's normal, accepted by ``TriIndex.query(points, max_dist=max_corr)``'s rule
    (d2 <= max_corr^2).  ``index``: a prebuilt NNIndex (cloud) or TriIndex (surface) of the target.
    ``normals="estimate"`` or ``normals=dict(k=..., max_dist=..., viewpoint=...)``: a raw cloud target; its normals are estimated once, on
    the NNIndex the loop queries, by ``cloud_normals.estimate_normals``.  Targets without a valid normal are matched but not used.
    Each iteration minimises sum w(r) r^2 over the linearised motion, r = n . (p - q): the 6x6 system of header Section 27, solved by
    ``ldlt_solve``; the update ``update_matrix(x)`` is left-multiplied onto the transformation and moves the float64 source.  Residual
    and Jacobian change sign together with the normal, so neither the winding of the mesh nor the side the cloud's normals point to
    matters.  ``kernel``: "l2", ("huber", k) or ("tukey", k), the weights of open3d's RobustKernel on r.
    Loop, criteria and result keys are ``icp_point_to_point``'s: dict(transformation [4, 4] float64 numpy, fitness = correspondences /
    source points, inlier_rmse = sqrt(mean squared correspondence distance), iterations), and ``residual_rmse`` = sqrt(mean r^2 over the
    used rows), ``used`` (rows with a correspondence and a usable normal) and ``degenerate``: the last system left a motion free
    (``ldlt_solve`` gave None), the update was the identity and the loop ended there."""
    code, k = _kernel(kernel)
    need_gpu("icp_point_to_plane")
    if not torch.is_tensor(source):
        source = torch.as_tensor(np.asarray(source, np.float32)).reshape(-1, 3).cuda()
    src32 = checked_points(source, "icp_point_to_plane")
    n, dev = src32.shape[0], src32.device
    if n == 0:
        raise ValueError("icp_point_to_plane: empty source")
    surface_mode = isinstance(target, (TriIndex, dict)) or _is_mesh_pair(target)
    if surface_mode:
        if normals is not None:
            raise ValueError("icp_point_to_plane: normals go with a cloud target; a mesh target takes its faces' normals")
        if index is None:
            index = target if isinstance(target, TriIndex) else TriIndex(*cuda_verts_faces(
                target if isinstance(target, dict) else {"verts": target[0], "faces": target[1]}, dev))
        if not isinstance(index, TriIndex):
            raise ValueError("icp_point_to_plane: a mesh target takes a TriIndex")
        bound = max_d2(max_corr, "icp_point_to_plane")
    else:
        if normals is None:
            raise ValueError("icp_point_to_plane: a cloud target needs normals [m, 3]")
        if not torch.is_tensor(target):
            target = torch.as_tensor(np.asarray(target, np.float32)).reshape(-1, 3).to(dev)
        tgt = checked_points(target, "icp_point_to_plane")
        if isinstance(normals, str) and normals != "estimate":
            raise ValueError(f"icp_point_to_plane: normals must be [m, 3], 'estimate' or dict(k=, max_dist=, viewpoint=), got {normals!r}")
        estimate = normals if isinstance(normals, dict) else ({} if isinstance(normals, str) else None)
        if estimate is None:
            nrm = _cuda(normals, torch.float32, dev)
            if nrm.shape != tgt.shape:
                raise ValueError(f"icp_point_to_plane: {tuple(nrm.shape)} normals for {tuple(tgt.shape)} targets")
        elif not set(estimate) <= {"k", "max_dist", "viewpoint"}:
            raise ValueError(f"icp_point_to_plane: normals=dict(...) takes k, max_dist and viewpoint, got {sorted(estimate)}")
        index = index if index is not None else NNIndex(tgt)
        if not isinstance(index, NNIndex) or index.n != tgt.shape[0]:
            raise ValueError("icp_point_to_plane: a cloud target takes an NNIndex of the same targets")
        if estimate is not None:                       # once, on the index the loop queries anyway
            nrm = estimate_normals(tgt, index=index, **estimate)
        if not float(max_corr) > 0:
            raise ValueError("icp_point_to_plane: max_corr must be > 0")
    if index.device != dev:
        raise ValueError("icp_point_to_plane: source on another device than the target")

    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4).copy()
    cur = src32.double()
    cur32 = torch.empty(n, 3, dtype=torch.float32, device=dev)
    corr = torch.empty(n, dtype=torch.int32, device=dev)
    system = _System(n, dev)
    if surface_mode:
        d2 = torch.empty(n, dtype=torch.float64, device=dev)
        closest = torch.empty(n, 3, dtype=torch.float32, device=dev)
    else:
        dist = torch.empty(n, dtype=torch.float32, device=dev)

    def evaluate():
        s = stream(dev)
        if surface_mode:
            check(lib.nsa_tri_query_bounded(index.buf.data_ptr(), index.verts.data_ptr(), index.V, index.faces.data_ptr(), index.F,
                                            cur32.data_ptr(), n, bound, corr.data_ptr(), d2.data_ptr(), closest.data_ptr(), None, None, s))
            system.run(cur, _native.ICP_SURFACE, corr, None, (d2, closest, index.verts, index.faces), code, k)
        else:
            check(lib.nsa_nn_query(index.buf.data_ptr(), index.n, cur32.data_ptr(), n, float(max_corr), corr.data_ptr(), dist.data_ptr(), s))
            system.run(cur, _native.ICP_CLOUD, corr, (dist, tgt, nrm), None, code, k)
        r = system.read()
        kc = r["k_corr"]
        return r, (kc / n if kc else 0.0), (math.sqrt(float(r["sums"][29]) / kc) if kc else 0.0)

    _move(cur, T, cur32)
    r, fit, rmse = evaluate()
    iterations, degenerate = 0, False
    for it in range(max_iter):
        x = ldlt_solve(r["A"], r["b"])
        if x is None:
            degenerate = True
            break
        upd = update_matrix(x)
        T = _matmul4(upd, T)
        _move(cur, upd, cur32)
        prev = (fit, rmse)
        r, fit, rmse = evaluate()
        iterations = it + 1
        if abs(prev[0] - fit) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
            break
    used = r["k_used"]
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, iterations=iterations, used=used, degenerate=degenerate,
                residual_rmse=math.sqrt(float(r["sums"][27]) / used) if used else 0.0)


def _parse_kernel(text):
    if text == "l2":
        return "l2"
    name, _, k = text.partition(":")
    try:
        spec = (name, float(k))
        _kernel(spec)
        return spec
    except ValueError:
        raise argparse.ArgumentTypeError(f"--kernel takes l2, huber:K or tukey:K with K > 0, got {text!r}")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_register", description=__doc__.splitlines()[0])
    ap.add_argument("source", metavar="SRC.ply")
    ap.add_argument("target", metavar="TGT.ply")
    ap.add_argument("--metric", choices=("plane", "surface"), default="surface",
                    help="plane: SRC's vertices against TGT's vertices and their angle-weighted normals; surface: against TGT's faces")
    ap.add_argument("--max-corr", type=float, default=0.1)
    ap.add_argument("--kernel", type=_parse_kernel, default="l2", metavar="l2|huber:K|tukey:K")
    ap.add_argument("--estimate-normals", type=int, nargs="?", const=30, default=None, metavar="K",
                    help="TGT is a cloud without nx ny nz: point-to-plane against its vertices with normals estimated from K neighbours")
    ap.add_argument("--init", metavar="T.npy", help="4x4 applied to SRC first")
    ap.add_argument("--out-transform", metavar="T.npy")
    ap.add_argument("--out", metavar="MOVED.ply", help="SRC moved by the result")
    ap.add_argument("--json", action="store_true", help="print the result as one JSON object")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("mesh_register: needs a GPU", file=sys.stderr)
        raise SystemExit(2)
    try:
        src, tgt = read_ply(a.source), read_ply(a.target)
        init = np.load(a.init) if a.init else None
        sv = torch.as_tensor(np.asarray(src["verts"]), dtype=torch.float32).cuda()
        if a.estimate_normals is not None:
            r = icp_point_to_plane(sv, torch.as_tensor(np.asarray(tgt["verts"]), dtype=torch.float32).cuda(),
                                   dict(k=a.estimate_normals), a.max_corr, init, kernel=a.kernel)
        elif a.metric == "plane":
            r = icp_point_to_plane(sv, torch.as_tensor(np.asarray(tgt["verts"]), dtype=torch.float32).cuda(),
                                   torch.as_tensor(np.asarray(vertex_normals(tgt, "angle"))), a.max_corr, init, kernel=a.kernel)
        else:
            r = icp_point_to_plane(sv, tgt, None, a.max_corr, init, kernel=a.kernel)
        if a.out_transform:
            np.save(a.out_transform, r["transformation"])
        if a.out:
            T = torch.from_numpy(r["transformation"]).cuda()
            moved = dict(src, verts=_transform(sv.double(), T).float())
            if "normals" in src:
                R = T.clone()
                R[:3, 3] = 0
                moved["normals"] = _transform(torch.as_tensor(np.ascontiguousarray(src["normals"])).double().cuda(), R).float()
            write_mesh_ply(a.out, moved)
    except (ValueError, OSError) as e:
        print(f"mesh_register: {e}", file=sys.stderr)
        raise SystemExit(2)
    if a.json:
        print(json.dumps({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items()}))
    else:
        print(f"metric: {a.metric}  iterations: {r['iterations']}  degenerate: {r['degenerate']}")
        print(f"fitness: {r['fitness']}  inlier rmse: {r['inlier_rmse']}  residual rmse: {r['residual_rmse']}  used: {r['used']}")
        print("transformation:\n" + np.array2string(r["transformation"], precision=10))
    return r


if __name__ == "__main__":
    main()
