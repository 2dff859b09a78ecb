"""Argument handling shared by the mesh and cloud front ends: one implementation of every check, of the move to the GPU and of the way
back.  A leaf module: it imports no other module of the package.

The contract every front end keeps, and that the ``*_cpu.py`` tests rely on: a malformed argument is a ``ValueError`` raised wherever
the argument lives, BEFORE the GPU is needed; a missing GPU is a ``RuntimeError`` (``need_gpu``).  So the checks (``checked_faces``,
the first half of ``checked_mesh``) never move anything, and the move (``to_cuda``) is a step of its own.  Every message starts with
``name``, the public function the caller is.
"""
import math

import numpy as np
import torch

# How many faces an entry point may take.  Indices are int32 on the device; what is indexed differs:
MAX_FACES = 2 ** 31 - 1                    # F < 2^31: a face index itself (components, the indexes of mesh_eval, the rasteriser)
MAX_FACES_EDGES = (2 ** 31 - 1) // 3       # 3 F < 2^31: the half-edge index 3 f + k of the edge table (nsa_mesh_edges) and its readers
MAX_FACES_RINGS = (2 ** 31 - 1) // 6       # 6 F < 2^31: the ring arrays of nsa_mesh_ring, two entries per half-edge (smooth, decimate, fill)
INDEX_DTYPES = (torch.int32, torch.int64)


def need_gpu(name):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{name}: needs a GPU")


def stream(dev=None):
    """the raw handle of torch's current stream on ``dev``, as the C entry points take it"""
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(t):
    """the device pointer of ``t``, or NULL for None and for an empty tensor"""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def workspace(nbytes, dev):
    """an uninitialised byte buffer for an ``nsa_*_workspace`` size"""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def as_tensor(x):
    """a tensor as it is, an array as a tensor over the same memory where it is contiguous"""
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def kind(x):
    """(was_numpy, original device or None) of an argument: what a result has to be given back as"""
    return (False, x.device) if torch.is_tensor(x) else (True, None)


def to_cuda(x, name, device="cuda"):
    """(CUDA tensor, was_numpy, original device) of an array or tensor; a CUDA tensor stays where it is"""
    if torch.is_tensor(x) and x.is_cuda:
        return x, False, x.device
    need_gpu(name)
    return (as_tensor(x).to(device),) + kind(x)


def restorer(was_numpy, orig):
    """the function that gives a result tensor back as the caller's kind: numpy, or torch on the device ``orig``"""
    return lambda t: t.cpu().numpy() if was_numpy else t.to(orig)


def restore_dict(d, was_numpy, orig):
    """``d`` with every tensor given back as the caller's kind; everything else carried"""
    give = restorer(was_numpy, orig)
    return {k: give(x) if torch.is_tensor(x) else x for k, x in d.items()}


def _count_error(name, max_faces):
    return ValueError(f"{name}: count out of range (0 <= n_verts < 2^31, n_faces <= {max_faces})")


def checked_faces(faces, name, *, max_faces=MAX_FACES, dtypes=INDEX_DTYPES, require_cuda=False, n_verts=None):
    """``faces`` as a tensor, still where it was, after the checks: shape [F, 3], a dtype of ``dtypes`` (None: any), F <= ``max_faces``
    (and 0 <= ``n_verts`` < 2^31 when given), every index inside int32.  The last reads the extrema back from wherever the faces live
    -- a synchronisation for CUDA faces -- and is skipped for int32, which cannot fail it.  The cast to int32 and the move to the GPU
    are the caller's next step (``to_cuda``), so that all of this runs without one."""
    if require_cuda and not (torch.is_tensor(faces) and faces.is_cuda):
        raise ValueError(f"{name}: faces must be a CUDA tensor [F, 3]")
    f = as_tensor(faces)
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"{name}: faces must be [F, 3]")
    if dtypes is not None and f.dtype not in dtypes:
        raise ValueError(f"{name}: faces must be int32 or int64")
    if f.shape[0] > max_faces or (n_verts is not None and not 0 <= int(n_verts) < 1 << 31):
        raise _count_error(name, max_faces)
    if f.dtype != torch.int32 and f.numel() and (int(f.min()) < -2 ** 31 or int(f.max()) >= 2 ** 31):
        raise ValueError(f"{name}: face index outside int32")
    return f


def cuda_faces(faces, n_verts, face_mask, name, device="cuda", *, max_faces=MAX_FACES_EDGES):
    """(faces int32 CUDA [F, 3], V, F, mask uint8 CUDA or None, restore) of a face list over ``n_verts`` vertices and an optional
    per-face mask (anything non-zero selects): ``checked_faces`` first, then the move, and the function that gives a result tensor
    the kind of ``faces`` back"""
    f = checked_faces(faces, name, max_faces=max_faces, n_verts=n_verts)
    V, F = int(n_verts), f.shape[0]
    mask = None
    if face_mask is not None:
        mask = torch.as_tensor(face_mask).reshape(-1)
        if mask.shape[0] != F:
            raise ValueError(f"{name}: mask of {mask.shape[0]} for {F} faces")
    f = to_cuda(f, name, device)[0].to(torch.int32).contiguous()
    if mask is not None:
        mask = (mask.to(f.device) != 0).to(torch.uint8).contiguous()
    return f, V, F, mask, restorer(*kind(faces))


def checked_rows(mesh, V, name, keys=("normals", "colors")):
    """every per-vertex entry of ``mesh`` among ``keys`` that is present has one row per vertex -- the check for entries that are
    carried along by index, whatever their width"""
    for k in keys:
        a = mesh.get(k)
        if a is not None and (len(a.shape) < 1 or a.shape[0] != V):
            raise ValueError(f"{name}: '{k}' has {a.shape[0] if len(a.shape) else 0} rows for {V} vertices")


def checked_mesh(mesh, name, device="cuda", *, float_verts=False, attributes=(), float_attributes=False, max_faces=MAX_FACES_EDGES):
    """(verts CUDA [V, 3], faces int32 CUDA [F, 3], V, F, {attribute: fp32 CUDA [V, 3]}, restore) of a mesh dict.  Checked first,
    wherever the arrays live: the dict has ``verts`` [V, 3] and ``faces`` (``checked_faces`` with ``max_faces``); with ``float_verts``
    the vertices are floating point; each of ``attributes`` that is present and not None is [V, 3] -- a kernel reads three floats per
    vertex there -- and floating point with ``float_attributes``.  Then the move: to the device of CUDA ``verts``, else to ``device``.
    ``float_verts`` also makes the vertices fp32 and contiguous; without it they keep their dtype.  ``restore`` gives a result tensor
    the kind of the mesh's ``verts`` back."""
    if not isinstance(mesh, dict) or "verts" not in mesh or "faces" not in mesh:
        raise ValueError(f"{name}: mesh needs 'verts' and 'faces'")
    v = as_tensor(mesh["verts"])
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"{name}: verts must be [V, 3]")
    if float_verts and not v.dtype.is_floating_point:
        raise ValueError(f"{name}: verts must be floating point")
    V = v.shape[0]
    f = checked_faces(mesh["faces"], name, max_faces=max_faces, n_verts=V)
    extra = {}
    for k in attributes:
        if mesh.get(k) is not None:
            a = as_tensor(mesh[k])
            if tuple(a.shape) != (V, 3) or (float_attributes and not a.dtype.is_floating_point):
                raise ValueError(f"{name}: {k} must be {'floating point ' if float_attributes else ''}[V, 3]")
            extra[k] = a
    if v.is_cuda:
        device = v.device
    f = to_cuda(f, name, device)[0].to(torch.int32).contiguous()
    v = to_cuda(v, name, f.device)[0]
    if float_verts:
        v = v.detach().float().contiguous()
    extra = {k: a.detach().to(f.device).float().contiguous() for k, a in extra.items()}
    return v, f, V, f.shape[0], extra, restorer(*kind(mesh["verts"]))


PER_VERTEX = ("verts", "normals", "colors")


def mesh_dict_tensors(mesh, device=None, name="mesh"):
    """(dict of tensors, was_numpy, original device) of a mesh dict, for the functions that hand a whole mesh on: ``verts``,
    ``faces``, ``normals`` and ``colors`` become tensors -- dtypes kept, moved to ``device`` when one is given -- and every other
    key is carried.  Checks ``verts`` [V, 3], ``faces`` [F, 3] and one row per vertex for the per-vertex entries; nothing else."""
    if "verts" not in mesh or "faces" not in mesh:
        raise ValueError(f"{name}: needs 'verts' and 'faces'")
    out = {}
    for k, x in mesh.items():
        if k in PER_VERTEX or k == "faces":
            out[k] = as_tensor(x) if device is None else as_tensor(x).to(device)
        else:
            out[k] = x
    if out["verts"].dim() != 2 or out["verts"].shape[1] != 3 or out["faces"].dim() != 2 or out["faces"].shape[1] != 3:
        raise ValueError(f"{name}: verts must be [V, 3] and faces [F, 3]")
    checked_rows(out, out["verts"].shape[0], name, PER_VERTEX)
    return (out,) + kind(mesh["verts"])


def cuda_verts_faces(mesh, device=None, cast=False):
    """(verts, faces) of a mesh dict on the GPU, for ``mesh_eval.TriIndex`` and the metrics: fp32 vertices [V, 3] and int64 faces
    [F, 3] on ``device`` (None: "cuda").  Without ``cast`` a mesh whose two arrays are CUDA tensors already is returned as it is,
    whatever its dtypes -- the index casts for itself.  Nothing is checked here: the index does that."""
    v, f = mesh["verts"], mesh["faces"]
    if not cast and torch.is_tensor(v) and v.is_cuda and torch.is_tensor(f) and f.is_cuda:
        return v, f
    device = "cuda" if device is None else device
    return (as_tensor(v).detach().to(device=device, dtype=torch.float32).reshape(-1, 3),
            as_tensor(f).detach().to(device=device, dtype=torch.int64).reshape(-1, 3))


def max_d2(max_dist, name):
    """the float64 squared bound the range-limited queries take for ``max_dist`` (None: +inf)"""
    if max_dist is None:
        return math.inf
    d = float(max_dist)
    if not d >= 0:
        raise ValueError(f"{name}: max_dist must be >= 0 or None, got {max_dist!r}")
    return d * d


def checked_points(x, name):
    """fp32 contiguous [n, 3] of a CUDA tensor of points, n < 2^31; anything else is a ValueError"""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise ValueError(f"{name}: needs a CUDA tensor [n, 3]")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name}: needs shape [n, 3], got {tuple(x.shape)}")
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"{name}: more than 2^31 - 1 points")
    return x.detach().float().contiguous()
