"""The signed distance field of a triangle mesh on the device (C ABI Section 15, csrc/mesh_sdf.hip), on the closest-point
index of mesh_eval.TriIndex.

* ``signed_distance(mesh, points)``: the exact distance of each point to the mesh with the sign of the angle-weighted pseudo-normal
  of the closest feature (Baerentzen & Aanaes 2005): positive on the side the faces' normals point to.
* ``contains(mesh, points)``: whether each point lies inside a CLOSED mesh.
* ``winding_number(mesh, points)``: the generalised winding number (C ABI Section 16, csrc/mesh_winding.hip; Jacobson et
  al. 2013, Barill et al. 2018): 1 inside and 0 outside a closed mesh, and on an OPEN mesh a smooth field that is 1/2 across a hole's
  virtual closure.  ``sign="winding"`` (``method="winding"`` for ``contains``) takes the sign of every function here from
  ``w > 0.5`` instead: an inside / outside test for meshes with holes.  The default ``"normal"`` is the pseudo-normal rule, unchanged.
  ``sign="auto"`` picks between the two: "normal" when the mesh is closed and consistently oriented, which
  ``mesh_topology.topology`` decides exactly, "winding" otherwise; ``resolve_sign`` returns the rule used.
  ``orient=True`` (``--orient``) on the functions that take a ``sign=`` winds the mesh consistently and its closed components outward
  first (``mesh_topology.orient``); "auto" is then resolved on the result.  The default changes nothing.
* ``mesh_sdf_grid(mesh, resolution, ...)``: a narrow-band SDF volume of the mesh, NaN outside the band, in the point order of
  inference.get_grid_uniform; inference.marching_cubes meshes it as it is.
* ``sdf_field_metrics(sdf, mesh, ...)``: the learned SDF field (a model, through inference.sdf_values, or any callable) against the
  mesh's signed distance at points scattered about its surface -- the field itself, not its marching-cubes level set.
* ``python -m nicer_slam_amd.mesh_sdf MESH.ply --resolution R --bounds LO HI --band B --out SDF.npy [--flip] [--orient]
  [--sign winding|auto [--beta B | --exact]] [--points P.npy --out-dist D.npy [--out-winding W.npy]]``.

For an open mesh the "normal" sign is that of the nearest surface element, not an inside / outside test; the "winding" sign is one.
There is no CPU path: a missing GPU
is an error.
"""
import argparse
import math

import numpy as np
import torch

from .mesh_args import cuda_verts_faces, need_gpu
from .mesh_eval import TriIndex, sample_surface
from .mesh_topology import orient as orient_mesh
from .ply import read_ply


def _index(mesh, points=None):
    if isinstance(mesh, TriIndex):
        return mesh
    return TriIndex(*cuda_verts_faces(mesh, points.device if torch.is_tensor(points) and points.is_cuda else None))


def _on_device(points, index):
    if not torch.is_tensor(points):
        points = torch.as_tensor(np.asarray(points), dtype=torch.float32).reshape(-1, 3)
    return points.to(index.device)


SIGNS = ("normal", "winding", "auto")


def _oriented(mesh, orient, weld=True, points=None):
    """the TriIndex the functions below work on: that of ``mesh`` itself, or with ``orient`` that of
    ``mesh_topology.orient(mesh, outward="volume", weld=weld)`` -- wound consistently, closed components outward"""
    index = _index(mesh, points)
    if not orient:
        return index
    return TriIndex(index.verts, orient_mesh({"verts": index.verts, "faces": index.faces}, outward="volume", weld=weld)["faces"])


def resolve_sign(mesh, sign, weld=True):
    """the sign rule a call with ``sign`` uses on ``mesh`` (a dict or a TriIndex): "normal" and "winding" are themselves; "auto"
    is "normal" when the mesh is closed and consistently oriented -- ``topology(mesh, weld=weld)["is_oriented"]``,
    cached on a TriIndex -- and "winding" otherwise."""
    if sign not in SIGNS:
        raise ValueError(f"resolve_sign: sign must be one of {SIGNS}, got {sign!r}")
    if sign != "auto":
        return sign
    return "normal" if _index(mesh).topology(weld=weld)["is_oriented"] else "winding"


def _sign_rule(sign, beta, name):
    """the checked (sign, beta) of a call: ``sign`` one of SIGNS, ``beta`` >= 1 (math.inf: the exact sum)"""
    if sign not in SIGNS:
        raise ValueError(f"{name}: sign must be one of {SIGNS}, got {sign!r}")
    beta = float(beta)
    if not beta >= 1.0:
        raise ValueError(f"{name}: beta must be >= 1, got {beta!r}")
    return sign, beta


@torch.no_grad()
def winding_number(mesh, points, beta=2.0, flip=False):
    """[m] float64: the generalised winding number of ``mesh`` (dict with ``verts`` and ``faces``, or a TriIndex) at ``points``:
    ``TriIndex.winding``.  1 inside and 0 outside a closed mesh with outward normals (``flip``: inward ones); on an open mesh a
    smooth field, 1/2 across a hole's virtual closure.  ``beta``: 2 the hierarchical approximation of Barill et al., math.inf the
    exact sum."""
    index = _index(mesh, points)
    return index.winding(_on_device(points, index), beta=beta, flip=flip)


def _winding_signed(index, pts, max_dist, flip, beta):
    """the distance of ``TriIndex.query`` -- the d2 of the signed query, bit for bit -- with the sign of the winding number: -1 where
    w > 0.5.  w is evaluated only at the points that have a closest point within ``max_dist``: compact, query, scatter back."""
    dist = index.query(pts, max_dist=max_dist)[0]
    have = torch.nonzero(torch.isfinite(dist)).reshape(-1)
    sign = torch.ones_like(dist)
    if have.numel():
        inside = index.winding(pts[have], beta=beta, flip=flip) > 0.5
        sign[have[inside]] = -1.0
    return sign * dist


@torch.no_grad()
def signed_distance(mesh, points, max_dist=None, flip=False, weld=True, sign="normal", beta=2.0, orient=False):
    """[m] float64: the signed distance of ``points`` (CUDA tensor or array [m, 3]) to ``mesh`` (dict with ``verts`` and ``faces``, or
    a TriIndex): ``TriIndex.signed_query(...)[0]``.  +inf (-inf with ``flip``) where nothing lies within ``max_dist``.
    ``sign="winding"``: the same magnitude, negative where the winding number (of the mesh with its normals turned by ``flip``)
    exceeds 0.5 -- inside / outside also for a mesh with holes, where the hole counts as closed by a surface on which w = 1/2;
    ``beta`` as in ``winding_number``; +inf where nothing lies within ``max_dist``, whatever ``flip``.
    ``orient=True``: the mesh goes through ``mesh_topology.orient(outward="volume")`` first, and ``sign="auto"`` is resolved on the
    result -- for a mesh whose faces are not wound consistently, or all inwards."""
    sign, beta = _sign_rule(sign, beta, "signed_distance")
    index = _oriented(mesh, orient, weld, points)
    sign = resolve_sign(index, sign, weld)
    if sign == "winding":
        return _winding_signed(index, _on_device(points, index), max_dist, flip, beta)
    return index.signed_query(_on_device(points, index), max_dist=max_dist, flip=flip, weld=weld)[0]


@torch.no_grad()
def contains(mesh, points, flip=False, weld=True, method="normal", beta=2.0, orient=False):
    """[m] bool: whether each point lies strictly inside ``mesh`` -- a CLOSED manifold mesh with outward normals (``flip`` for inward
    ones).  A point on the surface, and a non-finite point, is not inside.  On an open mesh the answer is the side of the nearest
    surface element and says nothing about an inside.  ``method="winding"``: whether the winding number exceeds 0.5 (a NaN is not
    inside) -- an answer for open meshes too, with every hole closed by the surface on which w = 1/2.  ``orient`` as in
    ``signed_distance``."""
    method, beta = _sign_rule(method, beta, "contains")
    if orient:
        mesh = _oriented(mesh, True, weld, points)
    if method == "auto":
        mesh = _index(mesh, points)
        method = resolve_sign(mesh, method, weld)
    if method == "winding":
        return winding_number(mesh, points, beta=beta, flip=flip) > 0.5
    return signed_distance(mesh, points, flip=flip, weld=weld) < 0


def grid_axis(resolution, grid_boundary, device):
    """the fp32 axis values of inference.get_grid_uniform / sdf_grid"""
    return torch.linspace(grid_boundary[0], grid_boundary[1], resolution, dtype=torch.float64, device=device).float()


def grid_points(ax, lo, hi):
    """points lo .. hi - 1 of inference.get_grid_uniform's list over the axis values ``ax``: the flat index runs over (y, x, z)"""
    R = ax.shape[0]
    flat = torch.arange(lo, hi, device=ax.device)
    iy = flat // (R * R)
    ix = (flat // R) % R
    iz = flat % R
    return torch.stack([ax[ix], ax[iy], ax[iz]], -1)


@torch.no_grad()
def mesh_sdf_grid(mesh, resolution, grid_boundary=(-1, 1), band=None, flip=False, chunk=1 << 22, weld=True, sign="normal", beta=2.0,
                  orient=False):
    """fp32 [R, R, R]: the signed distance to ``mesh`` at the points of ``inference.get_grid_uniform(R, grid_boundary)``, in that
    list's order (the flat index runs over (y, x, z); ``.permute(1, 0, 2)`` is the (x, y, z) volume inference.marching_cubes takes,
    as in inference.sdf_grid).  ``band`` (a distance; None: none): points farther than it from the mesh are NaN, and their queries
    stop after the few rings the band reaches -- without it a grid over the whole cube is the slow case of DESIGN 4m.
    inference.marching_cubes emits no face for a cell with a non-finite corner, so the volume can be meshed as it is.
    ``sign="winding"``: the sign of ``signed_distance(..., sign="winding", beta=beta)``; the winding number is evaluated only at the
    points within the band, so a banded grid still costs what the band sets.  ``orient`` as in ``signed_distance``."""
    sign, beta = _sign_rule(sign, beta, "mesh_sdf_grid")
    resolution = int(resolution)
    if resolution < 2 or resolution ** 3 >= 1 << 40:
        raise ValueError(f"mesh_sdf_grid: resolution {resolution} out of range")
    if not float(grid_boundary[1]) > float(grid_boundary[0]):
        raise ValueError("mesh_sdf_grid: grid_boundary must be (lo, hi) with hi > lo")
    if band is not None and not float(band) >= 0:
        raise ValueError("mesh_sdf_grid: band must be >= 0 or None")
    if chunk < 1:
        raise ValueError("mesh_sdf_grid: chunk must be >= 1")
    index = _oriented(mesh, orient, weld)
    sign = resolve_sign(index, sign, weld)
    ax = grid_axis(resolution, grid_boundary, index.device)
    n = resolution ** 3
    out = torch.empty(n, dtype=torch.float32, device=index.device)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        if sign == "winding":
            d = _winding_signed(index, grid_points(ax, lo, hi), band, flip, beta)
        else:
            d = index.signed_query(grid_points(ax, lo, hi), max_dist=band, flip=flip, weld=weld)[0]
        out[lo:hi] = torch.where(torch.isfinite(d), d, torch.full_like(d, math.nan)).float()
    return out.view(resolution, resolution, resolution)


def field_metrics(f, d, band):
    """The arithmetic of sdf_field_metrics on tensors of any device: ``f`` the field's values and ``d`` the mesh's signed distances at
    the same points.  Only points with |d| <= band count (a non-finite d does not)."""
    f, d = f.double().reshape(-1), d.double().reshape(-1)
    use = torch.isfinite(d) & (d.abs() <= band)
    k = int(use.sum())
    if k == 0:
        return {"mean abs error": math.nan, "rms error": math.nan, "sign agreement": math.nan, "points": 0}
    err = (f[use] - d[use]).abs()
    same = (f[use] < 0) == (d[use] < 0)
    return {"mean abs error": float(err.mean()), "rms error": math.sqrt(float((err * err).mean())),
            "sign agreement": float(same.double().mean()), "points": k}


@torch.no_grad()
def sdf_field_metrics(sdf, mesh, n_points=200000, sigma=0.01, band=0.05, seed=0, flip=False, weld=True, sign="normal", beta=2.0,
                      orient=False):
    """The SDF field ``sdf`` against the signed distance to ``mesh`` (the ground truth, or any surface the field should be the SDF
    of).  ``sdf``: a model (evaluated through inference.sdf_values) or a callable taking CUDA points [n, 3] fp32 and returning [n]
    values.  The points are ``mesh_eval.sample_surface(mesh, n_points, seed)`` each moved by a draw of N(0, sigma^2) per coordinate
    from a torch generator seeded with ``seed``, so they lie on both sides of the surface and on it.  Of the points within ``band``
    of the mesh: "mean abs error" and "rms error" of |f - d|, "sign agreement" (the share with (f < 0) == (d < 0)) and "points" (how
    many counted).  ``flip``: the mesh's normals point inwards.  ``sign="winding"``: d takes its sign from the winding number
    (``signed_distance``), the rule to use when the mesh is open.  ``orient`` as in ``signed_distance``."""
    sign, beta = _sign_rule(sign, beta, "sdf_field_metrics")
    if not (n_points > 0 and sigma >= 0 and band >= 0):
        raise ValueError("sdf_field_metrics: needs n_points > 0, sigma >= 0 and band >= 0")
    index = _oriented(mesh, orient, weld)
    sign = resolve_sign(index, sign, weld)
    pts, _ = sample_surface(index.verts, index.faces, int(n_points), seed)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    noise = torch.randn(pts.shape, generator=gen, dtype=torch.float64) * float(sigma)
    pts = (pts.double() + noise.to(pts.device)).float()
    if sign == "winding":
        d = _winding_signed(index, pts, band, flip, beta)
    else:
        d = index.signed_query(pts, max_dist=band, flip=flip, weld=weld)[0]
    if callable(sdf) and not isinstance(sdf, torch.nn.Module):
        f = sdf(pts)
    else:
        from . import inference            # (no cycle: it keeps the render stack out of a mesh tool's import)
        f = inference.sdf_values(sdf, pts)
    if not (torch.is_tensor(f) and f.numel() == pts.shape[0]):
        raise ValueError("sdf_field_metrics: the field must return one value per point")
    return field_metrics(f.to(d.device), d, float(band))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_sdf", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--resolution", type=int, help="write the [R, R, R] narrow-band SDF grid to --out")
    ap.add_argument("--bounds", type=float, nargs=2, default=(-1.0, 1.0), metavar=("LO", "HI"))
    ap.add_argument("--band", type=float, help="distance beyond which the grid (and --out-dist) is NaN")
    ap.add_argument("--out", metavar="SDF.npy")
    ap.add_argument("--flip", action="store_true", help="the mesh's normals point inwards")
    ap.add_argument("--points", metavar="P.npy", help="[m, 3] points to measure as well")
    ap.add_argument("--out-dist", metavar="D.npy", help="their signed distances, float64")
    ap.add_argument("--sign", choices=SIGNS, default="normal", help="the sign rule: pseudo-normal, winding number > 0.5, or auto: pseudo-normal when the mesh is closed and "
                    "consistently oriented (mesh_topology), winding otherwise")
    ap.add_argument("--beta", type=float, default=2.0, help="accuracy of the hierarchical winding number (>= 1)")
    ap.add_argument("--exact", action="store_true", help="the exact winding number: beta = +inf")
    ap.add_argument("--out-winding", metavar="W.npy", help="the winding numbers of --points, float64")
    ap.add_argument("--orient", action="store_true",
                    help="wind the mesh consistently, closed components outward, first (mesh_topology.orient)")
    a = ap.parse_args(argv)
    if (a.resolution is None) != (a.out is None):
        ap.error("--resolution and --out go together")
    if (a.points is None) != (a.out_dist is None):
        ap.error("--points and --out-dist go together")
    if a.resolution is None and a.points is None:
        ap.error("nothing to do: give --resolution and --out, or --points and --out-dist")
    if a.out_winding is not None and a.points is None:
        ap.error("--out-winding goes with --points")
    if not a.beta >= 1.0:
        ap.error("--beta must be >= 1")
    beta = math.inf if a.exact else a.beta
    need_gpu("mesh_sdf")
    index = _oriented(read_ply(a.mesh), a.orient)
    rule = resolve_sign(index, a.sign)
    result = {}
    if a.sign == "auto":                                       # (the other two say themselves; their output stays as it was)
        print(f"sign rule: {rule} (auto)")
        result["sign"] = rule
    if a.resolution is not None:
        grid = mesh_sdf_grid(index, a.resolution, tuple(a.bounds), a.band, a.flip, sign=rule, beta=beta)
        np.save(a.out, grid.cpu().numpy())
        inside = int(torch.isfinite(grid).sum())
        print(f"grid: {a.resolution}^3 over [{a.bounds[0]}, {a.bounds[1]}], {inside} points within the band -> {a.out}")
        result["grid"] = grid
    if a.points is not None:
        pts = np.load(a.points).reshape(-1, 3)
        d = signed_distance(index, pts, a.band, a.flip, sign=rule, beta=beta)
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.nan))
        np.save(a.out_dist, d.cpu().numpy())
        print(f"points: {pts.shape[0]}, {int(torch.isfinite(d).sum())} within the band -> {a.out_dist}")
        result["dist"] = d
        if a.out_winding is not None:
            w = winding_number(index, pts, beta=beta, flip=a.flip)
            np.save(a.out_winding, w.cpu().numpy())
            print(f"winding numbers: {pts.shape[0]}, {int((w > 0.5).sum())} inside -> {a.out_winding}")
            result["winding"] = w
    return result


if __name__ == "__main__":
    main()
