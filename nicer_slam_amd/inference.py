"""Batch inference consumers of the render core: full-image rendering in pixel chunks and SDF
evaluation on dense grids for mesh extraction.  Same kernels as the training path, no gradients, large batches.

Reference: utils.general.split_input / merge_output (code/utils/general.py:169-204), the vis loop of
VolSDFTrainRunner.vis (code/training/volsdf_train.py:255-290), get_grid_uniform / get_surface_trace's grid evaluation
(code/utils/plots.py:102-166), and the mesh that get_surface_trace extracts from that grid: marching cubes on the device
(csrc/mesh_extract.hip), vertex colours from the fused colour kernels, a binary PLY writer (plots.py:87-155; nicer_slam_amd/ply.py).
PNG writing stays with the caller.
"""
import ctypes

import torch

from ._native import lib, check, PointsDesc
from .fused.sampler import grid_desc, packed_sdf, precision_of, sdf_grid_desc, supported as fused_supported
from .ply import read_ply, write_ply  # noqa: F401  (their home is ply.py; the names stay importable from here)


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
