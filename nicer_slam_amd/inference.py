"""Batch inference consumers of the render core: full-image rendering in pixel chunks and SDF
evaluation on dense grids for mesh extraction.  Same kernels as the training path, no gradients, large batches.

Reference: utils.general.split_input / merge_output (code/utils/general.py:169-204), the vis loop of
VolSDFTrainRunner.vis (code/training/volsdf_train.py:255-290), get_grid_uniform / get_surface_trace's grid evaluation
(code/utils/plots.py:102-166), and the mesh that get_surface_trace extracts from that grid: marching cubes on the device
(csrc/mesh_extract.hip), vertex colours from the fused colour kernels, a binary PLY writer (plots.py:87-155).
PNG writing stays with the caller.
"""
import ctypes

import numpy as np
import torch

from ._native import lib, check, PointsDesc
from .fused.sampler import grid_desc, packed_sdf, precision_of, sdf_grid_desc, supported as fused_supported


def split_input(model_input, total_pixels, n_pixels=10000):
    """List of per-chunk copies of ``model_input`` (uv and the optional per-pixel entries sliced along dim 1)."""
    out = []
    dev = model_input["uv"].device
    for idx in torch.split(torch.arange(total_pixels, device=dev), n_pixels, dim=0):
        data = dict(model_input)
        for key in ("uv", "object_mask", "depth", "gt_depth"):
            if key in data:
                data[key] = torch.index_select(model_input[key], 1, idx.to(model_input[key].device))
        out.append(data)
    return out


def merge_output(res, total_pixels, batch_size):
    """Concatenate per-chunk output dicts back to [batch*total_pixels(, C)] like the reference."""
    merged = {}
    for key, first in res[0].items():
        if first is None:
            continue
        if first.dim() == 1:
            merged[key] = torch.cat([r[key].reshape(batch_size, -1, 1) for r in res], 1).reshape(batch_size * total_pixels)
        else:
            merged[key] = torch.cat([r[key].reshape(batch_size, -1, r[key].shape[-1]) for r in res], 1).reshape(
                batch_size * total_pixels, -1)
    return merged


@torch.no_grad()
def render_image(model, model_input, indices=None, ground_truth=None, mode="tracking_vis", n_pixels=65536,
                 stage="fine", color_stage="highfreq"):
    """Render every pixel of ``model_input['uv']`` ([b, H*W, 2]) in chunks of ``n_pixels`` rays; returns the merged
    ``rgb_values``, ``normal_map``, ``depth_values``.  Call on a model in eval mode (deterministic sampler)."""
    total = model_input["uv"].shape[1]
    bs = model_input["uv"].shape[0]
    if indices is None:
        indices = torch.arange(bs, device=model_input["uv"].device)
    res = []
    for chunk in split_input(model_input, total, n_pixels):
        out = model(chunk, indices, ground_truth or {}, mode=mode, stage=stage, color_stage=color_stage)
        res.append({k: out[k].detach() for k in ("rgb_values", "normal_map", "depth_values")})
    return merge_output(res, total, bs)


def get_grid_uniform(resolution, grid_boundary=(-2.0, 2.0), device="cpu"):
    """Axis values and the [res^3, 3] point list in the reference's order (np.meshgrid 'xy' indexing: the flat index
    runs over (y, x, z))."""
    x = torch.linspace(grid_boundary[0], grid_boundary[1], resolution, dtype=torch.float64, device=device)
    yy, xx, zz = torch.meshgrid(x, x, x, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1).float()
    return {"grid_points": pts, "shortest_axis_length": 2.0, "xyz": [x, x, x], "shortest_axis_index": 0}


@torch.no_grad()
def sdf_values(model, points, stage="fine", chunk=1 << 22):
    """SDF (coarse + fine) at ``points`` [N,3] on the GPU, no gradients: ImplicitNetworkGrid_COMBINE.get_sdf_vals[:, 0]."""
    if not (points.is_cuda and fused_supported(model)):
        raise RuntimeError("sdf_values: needs CUDA points and a model configuration covered by the fused kernels")
    imp = model.implicit_network
    gc, keep_c = sdf_grid_desc(model, "coarse", "sampler")
    gf, keep_f = sdf_grid_desc(model, "fine", "sampler")
    pc, pf = packed_sdf(model, "coarse", use="sampler"), packed_sdf(model, "fine", use="sampler")
    points = points.contiguous().float()
    out = torch.empty(points.shape[0], device=points.device)
    st = torch.cuda.current_stream().cuda_stream
    fine = stage != "coarse"
    for lo in range(0, points.shape[0], chunk):
        n = min(chunk, points.shape[0] - lo)
        check(lib.nsa_sdf_points(points[lo:lo + n].data_ptr(), n, ctypes.byref(gc), ctypes.byref(gf) if fine else None,
                                 pc.data_ptr(), pf.data_ptr() if fine else None, out[lo:lo + n].data_ptr(), st))
    return out


@torch.no_grad()
def sdf_grid(model, resolution, grid_boundary=(-2.0, 2.0), stage="fine", chunk=1 << 22):
    """SDF volume [res, res, res] indexed (x, y, z) -- what get_surface_trace hands to marching cubes (plots.py:
    121-127: reshape(ny, nx, nz).transpose(1, 0, 2)) -- evaluated chunk by chunk without materialising the point list."""
    dev = model.voxels.device
    ax = torch.linspace(grid_boundary[0], grid_boundary[1], resolution, dtype=torch.float64, device=dev).float()
    n = resolution ** 3
    out = torch.empty(n, device=dev)
    for lo in range(0, n, chunk):
        flat = torch.arange(lo, min(lo + chunk, n), device=dev)
        iy = flat // (resolution * resolution)
        ix = (flat // resolution) % resolution
        iz = flat % resolution
        pts = torch.stack([ax[ix], ax[iy], ax[iz]], -1)
        out[lo:lo + flat.numel()] = sdf_values(model, pts, stage, chunk)
    return out.view(resolution, resolution, resolution).permute(1, 0, 2).contiguous()


@torch.no_grad()
def marching_cubes(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Surface ``volume == level`` of a CUDA fp32 volume [nx, ny, nz] indexed (x, y, z) (what ``sdf_grid`` returns), on the device:
    dict(verts [V,3] f32, normals [V,3] f32, faces [F,3] int32).  Inside is ``value < level``; a vertex sits at
    ``origin + spacing * (sample index + t * axis)``; normals point towards increasing value; faces are oriented inside -> outside;
    the order is canonical.  Replaces skimage.measure.marching_cubes + the origin shift (plots.py:128-136).
    Offline inference: the call reads the two totals back to the host once (a synchronisation) to size the outputs."""
    if not (volume.is_cuda and volume.dtype == torch.float32 and volume.dim() == 3):
        raise ValueError("marching_cubes: needs a CUDA float32 volume [nx, ny, nz]")
    vol = volume.contiguous()
    nx, ny, nz = vol.shape
    dev = vol.device
    ws = torch.empty(max(1, lib.nsa_marching_cubes_workspace(nx, ny, nz)), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    check(lib.nsa_marching_cubes_count(vol.data_ptr(), nx, ny, nz, float(level), ws.data_ptr(), totals.data_ptr(), st))
    V, F = (int(v) for v in totals.cpu())
    verts = torch.empty(V, 3, device=dev)
    normals = torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    spc = (ctypes.c_float * 3)(*[float(v) for v in spacing])
    check(lib.nsa_marching_cubes_emit(vol.data_ptr(), nx, ny, nz, float(level), org, spc, ws.data_ptr(), V, F,
                                      verts.data_ptr() if V else None, normals.data_ptr() if V else None,
                                      faces.data_ptr() if F else None, st))
    return dict(verts=verts, normals=normals, faces=faces)


@torch.no_grad()
def vertex_colours(model, verts, normals, chunk=1 << 20):
    """rgb [V,3] of the colour network at ``verts`` seen along ``-normals``: the COMBINE's "fine" outputs (sdf gradient and
    feature) followed by the colour network with color_stage "highfreq" -- plots.py:137-147 -- through the fused kernels.
    The vertices travel as one-sample rays (o = vertex, d = -normal, z = 0), for which the kernels' point o + 0 * d is o."""
    from .fused.render import grid_desc, hl_size, packed_colour, supported as render_supported
    from .fused.sampler import forward_pair_ok
    if not (verts.is_cuda and render_supported(model)):
        raise RuntimeError("vertex_colours: needs CUDA vertices and a model configuration covered by the fused kernels")
    dev = verts.device
    V = verts.shape[0]
    out = torch.empty(V, 3, device=dev)
    if V == 0:
        return out
    gc, keep_c = sdf_grid_desc(model, "coarse")
    gf, keep_f = sdf_grid_desc(model, "fine")
    gr, keep_r = grid_desc(model.rendering_network.encoding, model.rendering_network.divide_factor, 2, precision_of(model, "colour"))
    pc, pf, pr = packed_sdf(model, "coarse"), packed_sdf(model, "fine"), packed_colour(model)
    pair = forward_pair_ok(model)
    if pair:
        gcp, keep_cp = sdf_grid_desc(model, "coarse", "coarse_pair")
        pcp = packed_sdf(model, "coarse", use="coarse_pair")
    verts = verts.contiguous().float()
    dirs = (-normals).contiguous().float()
    st = torch.cuda.current_stream(dev).cuda_stream
    n_max = min(chunk, V)
    z = torch.zeros(n_max, device=dev)
    sdf = torch.empty(n_max, device=dev)
    grad = torch.empty(n_max, 3, device=dev)
    feat = torch.empty(hl_size(n_max), device=dev)
    for lo in range(0, V, chunk):
        n = min(chunk, V - lo)
        pts = PointsDesc(verts[lo:].data_ptr(), dirs[lo:].data_ptr(), z.data_ptr(), None, n, 1, None)
        if pair:
            check(lib.nsa_sdfnet_forward_pair(ctypes.byref(pts), ctypes.byref(gcp), ctypes.byref(gf), pcp.data_ptr(), pf.data_ptr(),
                                              sdf.data_ptr(), grad.data_ptr(), feat.data_ptr(), st))
        else:
            check(lib.nsa_sdfnet_forward(ctypes.byref(pts), ctypes.byref(gc), pc.data_ptr(), 0, sdf.data_ptr(), grad.data_ptr(),
                                         feat.data_ptr(), st))
            check(lib.nsa_sdfnet_forward(ctypes.byref(pts), ctypes.byref(gf), pf.data_ptr(), 1, sdf.data_ptr(), grad.data_ptr(),
                                         feat.data_ptr(), st))
        check(lib.nsa_colour_forward(ctypes.byref(pts), ctypes.byref(gr), pr.data_ptr(), grad.data_ptr(), feat.data_ptr(),
                                     out[lo:].data_ptr(), None, st))
    return out


@torch.no_grad()
def extract_mesh(model, resolution, grid_boundary=(-2.0, 2.0), level=0.0, stage="fine", color=True, chunk=1 << 22, simplify=None,
                 smooth=None, decimate=None, fill_holes=None, split=None):
    """get_surface_trace on the device (plots.py:87-155): ``sdf_grid`` -> ``marching_cubes`` with the grid's spacing and origin
    -> (``color``) ``vertex_colours``.  Returns the marching_cubes dict, plus ``colors`` [V,3] in [0,1] when ``color`` is set.
    A level outside the volume's range gives empty tensors (the reference prints "NO MESH" and writes nothing).
    ``simplify``: a dict of ``mesh_simplify.simplify`` keywords (``cell=`` or ``target_faces=``, ...), applied after the colouring;
    None leaves the mesh as marching cubes made it.
    ``smooth``: a dict of ``mesh_smooth.smooth`` keywords (``method=``, ``iterations=``, ...), applied after the colouring -- the
    colours are queried on the true level set -- and before ``simplify``; None leaves the vertices where marching cubes put them.
    ``decimate``: a dict of ``mesh_decimate.decimate`` keywords (``target_faces=`` or ``max_error=``, ...), applied last, after
    ``simplify``; None collapses nothing.
    ``fill_holes``: a dict of ``mesh_fill.fill_holes`` keywords (``max_edges=``, ``max_size=``, ...), applied after the colouring
    and before ``smooth``, ``simplify`` and ``decimate`` -- a mesh cut by the grid's box is closed there; None fills nothing.
    ``split``: True or a dict of ``mesh_repair.split_nonmanifold`` keywords, applied after ``simplify`` and before ``decimate`` -- the
    edges with more than two faces that clustering makes are cut there, so that ``decimate`` need not lock them; None cuts nothing."""
    if split is not None and not isinstance(split, (bool, dict)):
        raise ValueError("extract_mesh: split must be None, a bool or a dict of mesh_repair.split_nonmanifold keywords")
    if fill_holes is not None and not isinstance(fill_holes, dict):
        raise ValueError("extract_mesh: fill_holes must be None or a dict of mesh_fill.fill_holes keywords")
    if decimate is not None and not isinstance(decimate, dict):
        raise ValueError("extract_mesh: decimate must be None or a dict of mesh_decimate.decimate keywords")
    if simplify is not None and not isinstance(simplify, dict):
        raise ValueError("extract_mesh: simplify must be None or a dict of mesh_simplify.simplify keywords")
    if smooth is not None and not isinstance(smooth, dict):
        raise ValueError("extract_mesh: smooth must be None or a dict of mesh_smooth.smooth keywords")
    vol = sdf_grid(model, resolution, grid_boundary, stage, chunk)
    ax = torch.linspace(grid_boundary[0], grid_boundary[1], resolution, dtype=torch.float64)     # get_grid_uniform's axis
    step = float(ax[1] - ax[0]) if resolution > 1 else 1.0
    mesh = marching_cubes(vol, level, (step,) * 3, (float(ax[0]),) * 3)
    if color:
        mesh["colors"] = vertex_colours(model, mesh["verts"], mesh["normals"], min(chunk, 1 << 20))
    if fill_holes is not None:
        from .mesh_fill import fill_holes as fill_mesh
        mesh = fill_mesh(mesh, **fill_holes)
    if smooth is not None:
        from .mesh_smooth import smooth as smooth_mesh
        mesh = smooth_mesh(mesh, **smooth)
    if simplify is not None:
        from .mesh_simplify import simplify as simplify_mesh
        mesh = simplify_mesh(mesh, **simplify)
    if split:
        from .mesh_repair import split_nonmanifold
        mesh = split_nonmanifold(mesh, **(split if isinstance(split, dict) else {}))
    if decimate is not None:
        from .mesh_decimate import decimate as decimate_mesh
        mesh = decimate_mesh(mesh, **decimate)
    return mesh


def write_ply(path, mesh):
    """Binary little-endian PLY of a ``marching_cubes`` / ``extract_mesh`` dict: per vertex float x y z nx ny nz (+ uchar
    red green blue when ``colors`` is present, round(255 * clamp(c, 0, 1))), faces as a uchar-counted int32 list."""
    v = mesh["verts"].detach().cpu().numpy().astype("<f4")
    n = mesh["normals"].detach().cpu().numpy().astype("<f4")
    f = mesh["faces"].detach().cpu().numpy().astype("<i4")
    col = mesh.get("colors")
    vfields = [(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")]
    if col is not None:
        vfields += [(k, "u1") for k in ("red", "green", "blue")]
    vrec = np.empty(v.shape[0], dtype=vfields)
    for i, k in enumerate(("x", "y", "z")):
        vrec[k] = v[:, i]
        vrec["n" + k] = n[:, i]
    if col is not None:
        c = np.rint(np.clip(col.detach().float().cpu().numpy(), 0, 1) * 255).astype(np.uint8)
        for i, k in enumerate(("red", "green", "blue")):
            vrec[k] = c[:, i]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    head += [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")]
    if col is not None:
        head += [f"property uchar {k}" for k in ("red", "green", "blue")]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path):
    """Read a PLY mesh (binary little-endian or ASCII, any scalar property types): dict of numpy ``verts`` [V,3] float32,
    ``faces`` [F,3] int32 (polygons fan-triangulated: (v0, v_k, v_k+1)), plus ``normals`` [V,3] float32 when nx ny nz are present
    and ``colors`` [V,3] float32 in [0, 1] (uchar / 255, other types as stored) when red green blue are.  The file comes from
    outside the program: a malformed header, a truncated body or a face index outside [0, V) raises ValueError.  A ``write_ply``
    -> ``read_ply`` round trip is exact (colours as the written uchar / 255)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic or no end_header)")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: header not terminated")
    try:
        header = data[:end].decode("ascii").splitlines()
    except UnicodeDecodeError as e:
        raise ValueError(f"{path}: header is not ASCII") from e
    body = data[nl + 1:]
    fmt, elements = None, []
    for line in header[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if len(tok) != 3 or tok[1] not in ("ascii", "binary_little_endian"):
                raise ValueError(f"{path}: unsupported format {line!r}")
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit():
                raise ValueError(f"{path}: bad element line {line!r}")
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if len(tok) == 5 and tok[1] == "list" and tok[2] in _PLY_TYPES and tok[3] in _PLY_TYPES:
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            elif len(tok) == 3 and tok[1] in _PLY_TYPES:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
            else:
                raise ValueError(f"{path}: bad property line {line!r}")
        else:
            raise ValueError(f"{path}: unknown header line {line!r}")
    if fmt is None:
        raise ValueError(f"{path}: no format line")
    out = {}
    if fmt == "ascii":
        words = body.split()
        pos = 0

        def take(k):
            nonlocal pos
            if pos + k > len(words):
                raise ValueError(f"{path}: truncated body")
            w = words[pos:pos + k]
            pos += k
            return w
    else:
        pos = 0
    for name, count, props in elements:
        has_list = any(p[2] is not None for p in props)
        fixed = None
        if fmt == "binary_little_endian" and len(props) == 1 and has_list and count > 0:
            _, t, it = props[0]                      # one list property: try a fixed length (triangle meshes)
            if pos + np.dtype(t).itemsize <= len(body):
                k = int(np.frombuffer(body, "<" + t, 1, pos)[0])
                fixed = np.dtype([("n", "<" + t), ("v", "<" + it, (k,))]) if k >= 0 else None
        if fixed is not None and pos + fixed.itemsize * count <= len(body) and \
                (np.frombuffer(body, fixed, count, pos)["n"] == fixed["v"].shape[0]).all():
            rec = np.frombuffer(body, fixed, count, pos)
            pos += fixed.itemsize * count
            cols = {props[0][0]: rec["v"].astype(np.int64)}
        elif fmt == "binary_little_endian" and not has_list:
            dt = np.dtype([(p[0], "<" + p[1]) for p in props])
            nbytes = dt.itemsize * count
            if pos + nbytes > len(body):
                raise ValueError(f"{path}: truncated body in element {name!r}")
            rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)
            pos += nbytes
            cols = {p[0]: rec[p[0]] for p in props}
        else:
            cols = {p[0]: [] for p in props}
            for _ in range(count):
                for pname, t, it in props:
                    if fmt == "ascii":
                        if it is None:
                            cols[pname].append(np.array(take(1), dtype=np.float64 if t[0] == "f" else np.int64)[0])
                        else:
                            n = int(take(1)[0])
                            if n < 0:
                                raise ValueError(f"{path}: negative list length")
                            cols[pname].append(np.array(take(n), dtype=np.int64))
                    else:
                        if it is None:
                            sz = np.dtype(t).itemsize
                            if pos + sz > len(body):
                                raise ValueError(f"{path}: truncated body in element {name!r}")
                            cols[pname].append(np.frombuffer(body, "<" + t, 1, pos)[0])
                            pos += sz
                        else:
                            sz = np.dtype(t).itemsize
                            if pos + sz > len(body):
                                raise ValueError(f"{path}: truncated body in element {name!r}")
                            n = int(np.frombuffer(body, "<" + t, 1, pos)[0])
                            pos += sz
                            isz = np.dtype(it).itemsize
                            if n < 0 or pos + n * isz > len(body):
                                raise ValueError(f"{path}: truncated body in element {name!r}")
                            cols[pname].append(np.frombuffer(body, "<" + it, n, pos).astype(np.int64))
                            pos += n * isz
            for pname, t, it in props:
                if it is None:
                    cols[pname] = np.asarray(cols[pname], dtype=t)
        out[name] = (count, cols)
    if "vertex" not in out:
        raise ValueError(f"{path}: no vertex element")
    V, vc = out["vertex"]
    if not all(k in vc for k in ("x", "y", "z")):
        raise ValueError(f"{path}: vertex element without x y z")
    mesh = {"verts": np.stack([np.asarray(vc[k]).astype(np.float32) for k in ("x", "y", "z")], -1).reshape(V, 3)}
    if all(k in vc for k in ("nx", "ny", "nz")):
        mesh["normals"] = np.stack([np.asarray(vc[k]).astype(np.float32) for k in ("nx", "ny", "nz")], -1).reshape(V, 3)
    if all(k in vc for k in ("red", "green", "blue")):
        c = np.stack([np.asarray(vc[k]) for k in ("red", "green", "blue")], -1).reshape(V, 3)
        mesh["colors"] = c.astype(np.float32) / 255.0 if c.dtype == np.uint8 else c.astype(np.float32)
    tris = []
    if "face" in out:
        F, fc = out["face"]
        lists = fc.get("vertex_indices", fc.get("vertex_index"))
        if lists is None:
            raise ValueError(f"{path}: face element without vertex_indices")
        if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.shape[1] >= 3:
            if lists.size and (lists.min() < 0 or lists.max() >= V):
                raise ValueError(f"{path}: face index outside [0, {V})")
            k = lists.shape[1]
            fan = [np.stack([lists[:, 0], lists[:, j], lists[:, j + 1]], -1) for j in range(1, k - 1)]
            mesh["faces"] = np.stack(fan, 1).reshape(-1, 3).astype(np.int32)
            return mesh
        for poly in lists:
            poly = np.asarray(poly, dtype=np.int64)
            if poly.size < 3:
                raise ValueError(f"{path}: face with fewer than 3 vertices")
            if poly.min() < 0 or poly.max() >= V:
                raise ValueError(f"{path}: face index outside [0, {V})")
            for k in range(1, poly.size - 1):
                tris.append((poly[0], poly[k], poly[k + 1]))
    mesh["faces"] = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    return mesh
