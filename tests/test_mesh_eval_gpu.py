"""Mesh evaluation on the device (csrc/mesh_eval.hip, nicer_slam_amd/mesh_eval.py) against the numpy oracle tests/eval_ref.py and
chunked fp32 brute force: exact nearest neighbours, surface sampling, ICP and the eval_rec.py metrics."""
import math

import numpy as np
import pytest
import torch

import eval_ref as E

pytestmark = pytest.mark.gpu


def _brute_torch(q, t, max_dist=math.inf, chunk=256):
    """fp32 brute force on the device with the kernel's operation order (separate torch ops: each one rounded, no contraction);
    the lowest index among the exact minima."""
    valid = torch.isfinite(t).all(1)
    strict = max_dist < math.inf
    r2 = float(np.float32(max_dist * max_dist)) if strict else math.inf
    ar = torch.arange(t.shape[0], device=t.device)
    dist = torch.empty(q.shape[0], device=q.device)
    idx = torch.empty(q.shape[0], dtype=torch.long, device=q.device)
    big = torch.tensor(t.shape[0], device=t.device)
    for lo in range(0, q.shape[0], chunk):
        qq = q[lo:lo + chunk]
        dx = t[None, :, 0] - qq[:, None, 0]
        dy = t[None, :, 1] - qq[:, None, 1]
        dz = t[None, :, 2] - qq[:, None, 2]
        d2 = torch.add(torch.add(dx * dx, dy * dy), dz * dz)
        ok = (d2 < r2) if strict else (valid[None, :] & ~torch.isnan(d2))
        ok &= valid[None, :]
        best = torch.where(ok, d2, torch.full_like(d2, math.inf)).min(1).values
        first = torch.where(ok & (d2 == best[:, None]), ar[None, :], big).min(1).values
        found = first < t.shape[0]
        idx[lo:lo + chunk] = torch.where(found, first, torch.full_like(first, -1))
        root = torch.from_numpy(np.sqrt(best.cpu().numpy())).to(best.device)     # IEEE sqrt (torch's on ROCm is not rounded)
        dist[lo:lo + chunk] = torch.where(found, root, torch.full_like(best, math.inf))
    bad = ~torch.isfinite(q).all(1)
    idx[bad] = -1
    dist[bad] = math.nan
    return dist, idx


def _check_nn(q, t, max_dist=math.inf):
    from nicer_slam_amd.mesh_eval import nearest
    d, i = nearest(q, t, max_dist)
    bd, bi = _brute_torch(q, t, max_dist)
    assert torch.equal(i, bi), (i != bi).nonzero()[:5]
    assert torch.equal(torch.isnan(d), torch.isnan(bd))
    ok = ~torch.isnan(d)
    assert torch.equal(d[ok], bd[ok])
    return d, i


def _g(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


@pytest.mark.parametrize("n", [1, 7, 1000, 20000, 200000])
def test_nearest_uniform_clouds_bit_exact(n):
    g = _g(n)
    t = torch.rand(n, 3, device="cuda", generator=g)
    q = torch.rand(min(n, 50000) if n > 1 else 100, 3, device="cuda", generator=g) * 1.2 - 0.1
    if n == 200000:
        q = torch.rand(200000, 3, device="cuda", generator=g)
    _check_nn(q, t)


def test_nearest_sphere_samples_bit_exact():
    g = _g(1)
    t = torch.randn(100000, 3, device="cuda", generator=g)
    t = t / t.norm(dim=1, keepdim=True) * 0.7 + 0.1
    q = torch.randn(50000, 3, device="cuda", generator=g)
    q = q / q.norm(dim=1, keepdim=True) * (0.7 + 0.01 * torch.randn(50000, 1, device="cuda", generator=g)) + 0.1
    _check_nn(q, t)


def test_nearest_heavy_duplicates_tie_to_lowest_index():
    g = _g(2)
    base = (torch.rand(50, 3, device="cuda", generator=g) * 8).round() / 8          # exact grid values: many equal distances
    t = base[torch.randint(0, 50, (20000,), device="cuda", generator=g)]
    q = (torch.rand(5000, 3, device="cuda", generator=g) * 8).round() / 8
    d, i = _check_nn(q, t)
    # the chosen index is the first occurrence of the nearest distinct point
    first = {}
    for k, row in enumerate(t.cpu().numpy().tolist()):
        first.setdefault(tuple(row), k)
    assert all(first[tuple(t[j].tolist())] == j for j in i[:200].tolist())
    _check_nn(q, t[:1].expand(3000, 3).contiguous())                                    # all targets identical


def test_nearest_cluster_with_far_outlier_and_far_queries():
    g = _g(3)
    t = torch.rand(100000, 3, device="cuda", generator=g) * 0.01
    t[12345] = torch.tensor([1e4, -3e3, 5e2], device="cuda")                          # a stray component far away
    q = torch.cat([torch.rand(20000, 3, device="cuda", generator=g) * 0.012,
                   torch.tensor([[1e4, -3e3, 5e2 + 1.0], [9e3, 0.0, 0.0], [-50.0, 20.0, 1e3]], device="cuda"),
                   torch.randn(2000, 3, device="cuda", generator=g) * 100.0])         # queries far outside the bulk
    d, i = _check_nn(q, t)
    assert int(i[20000]) == 12345


def test_nearest_nonfinite_entries_and_single_target():
    g = _g(4)
    t = torch.rand(5000, 3, device="cuda", generator=g)
    t[::97, 1] = math.nan
    t[5::101, 2] = math.inf
    q = torch.rand(3000, 3, device="cuda", generator=g)
    q[::50, 0] = math.nan
    q[7::70, 1] = -math.inf
    d, i = _check_nn(q, t)
    assert (i[::50] == -1).all() and torch.isnan(d[::50]).all()
    assert not (~torch.isfinite(t[i[i >= 0]])).any()
    _check_nn(q, t[:1].clone())
    _check_nn(torch.tensor([[0.0, 0.0, 0.0], [1e30, 1e30, 1e30]], device="cuda"), torch.tensor([[1.0, 2.0, 3.0]], device="cuda"))
    none = torch.full((10, 3), math.nan, device="cuda")                               # no finite target at all
    from nicer_slam_amd.mesh_eval import nearest
    d, i = nearest(q[:100], none)
    assert (i == -1).all() and torch.isinf(d[torch.isfinite(q[:100]).all(1)]).all()


@pytest.mark.parametrize("r", [0.001, 0.02, 0.1, 1.0])
def test_nearest_radius_form(r):
    g = _g(5)
    t = torch.rand(30000, 3, device="cuda", generator=g)
    q = torch.rand(20000, 3, device="cuda", generator=g) * 1.4 - 0.2
    d, i = _check_nn(q, t, r)
    assert (i == -1).any() or r >= 0.1
    assert torch.isinf(d[i == -1]).all()
    # a query exactly at the radius is outside (strict)
    t1 = torch.tensor([[0.0, 0.0, 0.0]], device="cuda")
    from nicer_slam_amd.mesh_eval import nearest
    _, i1 = nearest(torch.tensor([[0.5, 0.0, 0.0], [0.25, 0.0, 0.0]], device="cuda"), t1, 0.5)
    assert i1.tolist() == [-1, 0]


def test_nearest_index_reuse_and_repeats_are_identical():
    from nicer_slam_amd.mesh_eval import NNIndex
    g = _g(6)
    t = torch.rand(200000, 3, device="cuda", generator=g)
    q = torch.rand(200000, 3, device="cuda", generator=g)
    ix = NNIndex(t)
    a = ix.query(q)
    b = ix.query(q)
    c = NNIndex(t).query(q)
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


# ---- sampling -------------------------------------------------------------------------------------------------------------------

def _sphere_mesh(res=64, r=0.5, c=(0.0, 0.0, 0.0), bound=1.0):
    from nicer_slam_amd import inference
    ax = torch.linspace(-bound, bound, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r).float().cuda()
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol, 0.0, (step,) * 3, (-bound,) * 3)


def _blob_mesh(res=64):
    """three spheres of different radii: no rotational symmetry (ICP can recover a rotation)"""
    from nicer_slam_amd import inference
    ax = torch.linspace(-1, 1, res, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    s = lambda c, r: torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r
    vol = torch.minimum(torch.minimum(s((0.2, 0, 0), 0.4), s((-0.35, 0.25, 0.1), 0.25)), s((0, -0.3, 0.35), 0.2))
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol.float().cuda(), 0.0, (step,) * 3, (-1.0,) * 3)


def test_sample_surface_matches_oracle():
    from nicer_slam_amd.mesh_eval import sample_surface
    m = _blob_mesh(48)
    v, f = m["verts"], m["faces"]
    f = torch.cat([f, f[:5, [0, 0, 1]]])                                               # degenerate faces: never picked
    for seed in (0, 12345, 2 ** 40 + 7):
        p, fi = sample_surface(v, f, 200000, seed)
        rp, rfi = E.sample_surface(v.cpu().numpy(), f.cpu().numpy(), 200000, seed)
        assert np.array_equal(fi.cpu().numpy(), rfi), seed
        np.testing.assert_array_max_ulp(p.cpu().numpy(), rp, maxulp=4)
        assert (fi < m["faces"].shape[0]).all()
    p2, _ = sample_surface(v, f, 1000, 1)
    assert not torch.equal(p2, sample_surface(v, f, 1000, 2)[0])
    assert torch.equal(p2, sample_surface(v, f, 1000, 1)[0])


def test_sample_surface_on_faces_and_area_proportional():
    from nicer_slam_amd.mesh_eval import sample_surface
    g = torch.Generator().manual_seed(9)
    v = torch.randn(30, 3, generator=g)
    f = torch.randint(0, 30, (40, 3), generator=g, dtype=torch.int32)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    n = 400000
    p, fi = sample_surface(v.cuda(), f.cuda(), n, 3)
    p, fi = p.cpu().double(), fi.cpu()
    a, b, c = v.double()[f[fi, 0].long()], v.double()[f[fi, 1].long()], v.double()[f[fi, 2].long()]
    # barycentric residual: p - a in the span of (b - a, c - a), coefficients in the triangle
    M = torch.stack([b - a, c - a], -1)
    coef = torch.linalg.lstsq(M, (p - a)[..., None]).solution[..., 0]
    res = (M @ coef[..., None])[..., 0] - (p - a)
    scale = v.abs().max().item()
    assert res.abs().max().item() < 16 * 2 ** -24 * scale
    assert (coef > -1e-5).all() and (coef.sum(-1) < 1 + 1e-5).all()
    area = E.face_areas(v.numpy(), f.numpy())
    exp = area / area.sum() * n
    obs = np.bincount(fi.numpy(), minlength=len(f))
    chi2 = ((obs - exp) ** 2 / exp).sum()
    assert chi2 < len(f) + 6 * math.sqrt(2 * len(f)), chi2                              # fixed seed, ~6 sigma


def test_sample_surface_rejects_zero_area_and_empty():
    from nicer_slam_amd.mesh_eval import sample_surface
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]], device="cuda")
    with pytest.raises(ValueError):
        sample_surface(v, torch.tensor([[0, 1, 2]], device="cuda", dtype=torch.int32), 10, 0)
    with pytest.raises(ValueError):
        sample_surface(v, torch.zeros(0, 3, device="cuda", dtype=torch.int32), 10, 0)


# ---- ICP ------------------------------------------------------------------------------------------------------------------------

def test_icp_matches_oracle():
    from nicer_slam_amd.mesh_eval import icp_point_to_point
    g = np.random.default_rng(0)
    tgt = (g.random((4000, 3)) * np.array([1.0, 0.7, 0.4])).astype(np.float32)
    tgt = np.concatenate([tgt, tgt[:1000] * 0.3 + np.array([0.9, 0.1, 0.5], np.float32)])
    T = E.rigid([1.0, 0.3, -0.2], 3.0, [0.03, 0.01, -0.02])
    src = (E.transform(tgt.astype(np.float64), T) + g.normal(0, 0.002, tgt.shape)).astype(np.float32)
    got = icp_point_to_point(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), 0.05)
    ref = E.icp(src, tgt, 0.05)
    assert got["iterations"] == ref["iterations"]
    assert got["fitness"] == ref["fitness"]
    # (float64 sums on the device vs numpy differ in the last bits; a query that lands 1 ulp apart can pick a near-tied target)
    assert got["inlier_rmse"] == pytest.approx(ref["inlier_rmse"], rel=1e-6)
    np.testing.assert_allclose(got["transformation"], ref["transformation"], rtol=0, atol=1e-7)


def test_icp_recovers_a_small_motion_of_a_marching_cubes_mesh():
    from nicer_slam_amd.mesh_eval import icp_point_to_point
    v = _blob_mesh(64)["verts"]
    T = E.rigid([0.2, 1.0, -0.4], 5.0, [0.02, -0.01, 0.015])
    src = torch.from_numpy(E.transform(v.cpu().numpy().astype(np.float64), T).astype(np.float32)).cuda()
    out = icp_point_to_point(src, v, 0.1)
    assert np.abs(out["transformation"] - np.linalg.inv(T)).max() < 1e-4, out
    assert out["fitness"] == 1.0


# ---- metrics --------------------------------------------------------------------------------------------------------------------

def test_mesh_metrics_equal_oracle_on_the_same_samples():
    from nicer_slam_amd import mesh_eval as M
    rec, gt = _blob_mesh(48), _sphere_mesh(48, 0.45)
    out = M.mesh_metrics(rec, gt, n_points=20000, seed=3, align=False)
    rp, ri = M.sample_surface(rec["verts"], rec["faces"], 20000, 3)
    gp, gi = M.sample_surface(gt["verts"], gt["faces"], 20000, 4)
    rn = E.face_normals(rec["verts"].cpu().numpy(), rec["faces"].cpu().numpy())[ri.cpu().numpy()]
    gn = E.face_normals(gt["verts"].cpu().numpy(), gt["faces"].cpu().numpy())[gi.cpu().numpy()]
    da, ia = E.nn_brute(rp.cpu().numpy(), gp.cpu().numpy())
    dc, ic = E.nn_brute(gp.cpu().numpy(), rp.cpu().numpy())
    ref = E.metrics(da, ia, dc, ic, rn, gn)
    for k, v in ref.items():
        assert out[k] == pytest.approx(v, rel=1e-6, abs=1e-12), k


def test_mesh_metrics_concentric_spheres_and_self():
    from nicer_slam_amd import mesh_eval as M
    r, delta = 0.5, 0.02
    a, b = _sphere_mesh(128, r), _sphere_mesh(128, r + delta)
    out = M.mesh_metrics(a, b, align=False)
    assert abs(out["accuracy"] - delta) < 2e-3 and abs(out["completion"] - delta) < 2e-3, out
    assert out["completion ratio"] == 1.0 and out["f-score"] == 0.0 and out["normals"] > 0.99
    same = M.mesh_metrics(a, a)
    spacing = math.sqrt(4 * math.pi * r * r / 200000)
    assert same["completion ratio"] == 1.0 and 0 < same["accuracy"] < spacing and 0 < same["completion"] < spacing, same
    assert np.abs(same["transformation"] - np.eye(4)).max() < 1e-3 and same["icp fitness"] == 1.0
    with pytest.raises(ValueError):
        M.mesh_metrics({"verts": np.zeros((0, 3)), "faces": np.zeros((0, 3), np.int32)}, b)
    flat = {"verts": np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32), "faces": np.array([[0, 1, 2]], np.int32)}
    with pytest.raises(ValueError):
        M.mesh_metrics(flat, b, align=False)


def test_extract_write_read_metrics_end_to_end(tmp_path):
    from nicer_slam_amd import inference, mesh_eval as M
    from test_mesh_gpu import _model
    mesh = inference.extract_mesh(_model(), 64, (-1.0, 1.0))
    assert mesh["faces"].shape[0] > 0
    inference.write_ply(tmp_path / "rec.ply", mesh)
    back = inference.read_ply(tmp_path / "rec.ply")
    assert np.array_equal(back["verts"], mesh["verts"].cpu().numpy())
    assert np.array_equal(back["faces"], mesh["faces"].cpu().numpy())
    out = M.mesh_metrics(back, back, n_points=50000, seed=1)
    assert out["completion ratio"] == 1.0 and out["accuracy"] < 0.02 and out["normals"] > 0.9, out
    m = M.main([str(tmp_path / "rec.ply"), str(tmp_path / "rec.ply"), "--points", "20000", "--no-align"])
    assert m["completion ratio"] == 1.0
