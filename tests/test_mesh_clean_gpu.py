"""Mesh clean-up on the device (csrc/mesh_clean.hip, nicer_slam_amd/mesh_clean.py, the scaled ICP and the driver of
mesh_eval.py) against the numpy oracle tests/clean_ref.py: labels, statistics and cleaned meshes exactly, the
similarity transform, scale-adjusting ICP and the eval_rec.py chain end to end.  The small cases come first in the file."""
import math

import numpy as np
import pytest
import torch

import clean_ref as C
import eval_ref as E
import mc_ref

pytestmark = pytest.mark.gpu


def _mc(vol, res):
    from nicer_slam_amd import inference
    ax = torch.linspace(-1, 1, res, dtype=torch.float64)
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol.float().cuda(), 0.0, (step,) * 3, (-1.0,) * 3)


def _grid(res):
    ax = torch.linspace(-1, 1, res, dtype=torch.float64)
    return torch.meshgrid(ax, ax, ax, indexing="ij")


def _sphere(X, Y, Z, c, r):
    return torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r


def _blob_vol(res):
    """the volume of test_mesh_eval_gpu._blob_mesh"""
    X, Y, Z = _grid(res)
    s = lambda c, r: _sphere(X, Y, Z, c, r)
    return torch.minimum(torch.minimum(s((0.2, 0, 0), 0.4), s((-0.35, 0.25, 0.1), 0.25)), s((0, -0.3, 0.35), 0.2))


def _blob_with_stray(res):
    X, Y, Z = _grid(res)
    return _mc(torch.minimum(_blob_vol(res), _sphere(X, Y, Z, (-0.75, -0.75, -0.75), 0.12)), res)


def _four_spheres():
    X, Y, Z = _grid(64)
    vol = None
    for c, r in (((-0.5, -0.5, -0.5), 0.30), ((0.5, 0.5, -0.4), 0.22), ((0.5, -0.5, 0.5), 0.15), ((-0.5, 0.6, 0.6), 0.08)):
        s = _sphere(X, Y, Z, c, r)
        vol = s if vol is None else torch.minimum(vol, s)
    return _mc(vol, 64)


def _noisy_sphere():
    X, Y, Z = _grid(48)
    g = torch.Generator().manual_seed(11)
    noise = (torch.rand(48, 48, 48, generator=g, dtype=torch.float64) * 2 - 1) * 0.06
    return _mc(_sphere(X, Y, Z, (0, 0, 0), 0.6) + noise, 48)


def _check_labels(faces, V):
    """device labels == oracle, element for element; a second call is bit-identical"""
    from nicer_slam_amd.mesh_clean import components
    f = torch.as_tensor(faces).cuda()
    vl, fl, n, used = components(f, V)
    rvl, rfl, rn, rused = C.components(f.cpu().numpy(), V)
    assert (n, used) == (rn, rused)
    assert np.array_equal(vl.cpu().numpy(), rvl) and np.array_equal(fl.cpu().numpy(), rfl)
    vl2, fl2, n2, used2 = components(f, V)
    assert torch.equal(vl, vl2) and torch.equal(fl, fl2) and (n2, used2) == (n, used)
    return n


def _check_stats(verts, faces):
    """device table == oracle: integers and boxes exactly, areas within (n_faces + 16) 2^-53 of math.fsum; two runs identical"""
    from nicer_slam_amd.mesh_clean import component_stats
    v, f = torch.as_tensor(verts).cuda(), torch.as_tensor(faces).cuda()
    st = component_stats(v, f)
    ref = C.component_stats(v.cpu().numpy(), f.cpu().numpy())
    assert st["n_components"] == ref["n_components"]
    for k in ("label", "n_faces", "n_verts", "vertex_comp", "face_comp"):
        assert np.array_equal(st[k].cpu().numpy(), ref[k]), k
    for k in ("lo", "hi"):
        assert np.array_equal(st[k].cpu().numpy().view(np.uint32), ref[k].view(np.uint32)), k
    area = st["area"].cpu().numpy()
    rel = np.abs(area - ref["area"]) / np.maximum(ref["area"], 1e-300)
    bound = (ref["n_faces"] + 16) * 2.0 ** -53
    print("area: worst relative deviation from fsum", float(rel.max(initial=0.0)), "worst bound used", float((rel / bound).max(initial=0.0)))
    assert (rel <= bound).all(), (rel / bound).max()
    again = component_stats(v, f)
    for k, x in st.items():
        assert x == again[k] if isinstance(x, int) else torch.equal(x.view(torch.uint8), again[k].view(torch.uint8)), k
    return st, ref


# ---- labels ---------------------------------------------------------------------------------------------------------------------

def test_labels_small_lists():
    assert _check_labels(np.array([[0, 1, 2]], np.int32), 3) == 1
    assert _check_labels(np.zeros((0, 3), np.int32), 5) == 0
    f, V = C.adversarial_cases(1000)["invalid, degenerate, trailing"]
    assert _check_labels(f, V) == 2                                    # {0, 1, 2, 7, 8} and {5, 6}; 3, 4, 9, 10, 11 unreferenced
    assert _check_labels(np.array([[0, 1, 2], [2, 3, 4], [6, 7, 8], [8, 9, 4]], np.int64), 11) == 1
    from nicer_slam_amd.mesh_clean import components
    vl, fl, n, used = components(torch.zeros(0, 3, dtype=torch.int32, device="cuda"), 0)
    assert vl.numel() == 0 and fl.numel() == 0 and (n, used) == (0, 0)
    for name, (f, V) in C.adversarial_cases(2000).items():
        _check_labels(f, V)


def test_labels_four_disjoint_spheres():
    m = _four_spheres()
    assert _check_labels(m["faces"], m["verts"].shape[0]) == 4
    st, ref = _check_stats(m["verts"], m["faces"])
    # (face counts depend on where the centres sit in the grid; for these centres the two small spheres have 824 / 228 faces)
    assert sorted(ref["n_faces"].tolist(), reverse=True) == [3368, 1796, 824, 228]
    assert np.allclose(sorted(ref["area"].tolist(), reverse=True), [1.1270, 0.6042, 0.2788, 0.0764], atol=5e-5)


def test_labels_noisy_sphere_many_small_components():
    m = _noisy_sphere()
    assert mc_ref.is_closed(m["faces"].cpu().numpy())
    n = _check_labels(m["faces"], m["verts"].shape[0])
    assert n == 112                                                     # (the oracle's count for this seed)
    st, ref = _check_stats(m["verts"], m["faces"])
    assert ref["n_faces"].max() > 0.5 * ref["n_faces"].sum() and np.median(ref["n_faces"]) <= 32


def test_labels_blob_and_large_sphere_are_one_component():
    from test_mesh_eval_gpu import _blob_mesh, _sphere_mesh
    m = _blob_mesh(64)
    assert _check_labels(m["faces"], m["verts"].shape[0]) == 1
    s = _sphere_mesh(128, 0.8)                                          # about 100 k faces
    assert s["faces"].shape[0] > 80000
    assert _check_labels(s["faces"], s["verts"].shape[0]) == 1


@pytest.mark.parametrize("name", ["strip", "strip reversed", "strip permuted names", "star", "random sparse", "random dense", "soup",
                                  "two strips alternating", "invalid, degenerate, trailing", "no faces"])
def test_labels_adversarial_index_orders(name):
    f, V = C.adversarial_cases(100000)[name]
    n = _check_labels(f, V)
    expect = {"strip": 1, "strip reversed": 1, "strip permuted names": 1, "star": 1, "random dense": 1, "soup": 50000,
              "two strips alternating": 2, "no faces": 0}
    if name in expect:
        assert n == expect[name]
    if name == "random sparse":
        vl = C.components(f, V)[0]
        assert n > 1000 and (vl < 0).sum() > 100000


# ---- statistics -----------------------------------------------------------------------------------------------------------------

def test_stats_on_index_orders_and_nonfinite_vertices():
    g = np.random.default_rng(2)
    for name in ("random sparse", "soup", "two strips alternating", "invalid, degenerate, trailing", "no faces", "star"):
        f, V = C.adversarial_cases(20000)[name]
        v = g.normal(size=(V, 3)).astype(np.float32)
        v[::37, 1] = np.nan
        v[5::41, 0] = np.inf
        v[3::29, 2] = -0.0
        _check_stats(v, f)


@pytest.mark.parametrize("n,V", [(341, 1023), (341, 1024), (342, 1026), (349526, 1048578)])
def test_stats_soup_at_the_seams_of_the_rank_scan(n, V):
    """a soup of n disjoint triangles, triangle r on the vertices 3 r, 3 r + 1, 3 r + 2: V just below, at (one vertex unused) and just
    above the 1024 lanes of a block of the rank scan (csrc/block_scan.hpp), and V = 1 048 578 > 1024 * 1024, where a lane of the one
    workgroup that scans the block counts owns more than one block.  In closed form: n components, label[r] = 3 r, three vertices
    and one face each"""
    from nicer_slam_amd.mesh_clean import component_stats
    r = torch.arange(n, device="cuda")
    f = (3 * r[:, None] + torch.arange(3, device="cuda")).to(torch.int32)
    v = torch.zeros(V, 3, device="cuda")
    v[:3 * n, 0] = r.repeat_interleave(3).float()
    v[1:3 * n:3, 0] += 0.5
    v[2:3 * n:3, 1] = 0.5
    st = component_stats(v, f)
    assert st["n_components"] == n
    r32 = r.to(torch.int32)
    assert torch.equal(st["label"], 3 * r32) and torch.equal(st["face_comp"], r32)
    assert torch.equal(st["vertex_comp"][:3 * n], r32.repeat_interleave(3)) and bool((st["vertex_comp"][3 * n:] == -1).all())
    assert bool((st["n_verts"] == 3).all()) and bool((st["n_faces"] == 1).all())
    assert bool(((st["area"] - 0.125).abs() <= 0.125 * 2.0 ** -50).all())      # 1/8 each, exactly representable inputs
    lo = torch.stack([r.float(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")], 1)
    assert torch.equal(st["lo"], lo) and torch.equal(st["hi"], lo + torch.tensor([0.5, 0.5, 0.0], device="cuda"))


def test_stats_area_agrees_with_the_surface_sampler_total():
    from nicer_slam_amd._native import lib, check
    from test_mesh_eval_gpu import _blob_mesh
    for m in (_blob_mesh(64), _four_spheres(), _noisy_sphere()):
        st, ref = _check_stats(m["verts"], m["faces"])
        v, f = m["verts"].contiguous(), m["faces"].contiguous()
        V, F = v.shape[0], f.shape[0]
        ws = torch.empty(lib.nsa_surface_sample_workspace(F), dtype=torch.uint8, device="cuda")
        total = torch.empty(1, dtype=torch.float64, device="cuda")
        check(lib.nsa_surface_sample(v.data_ptr(), V, f.data_ptr(), F, 0, 0, ws.data_ptr(), None, None, total.data_ptr(), None))
        a, t = float(st["area"].sum()), float(total)
        # two fixed-order sums of the same F non-negative float64 terms: each within (F - 1) 2^-53 of the exact sum
        assert abs(a - t) <= 2 * (F + 16) * 2.0 ** -53 * t, (a, t)


# ---- cleaning -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", [48, 64])
def test_keep_largest_returns_the_blob_bit_for_bit(res, tmp_path):
    from nicer_slam_amd import inference, mesh_clean as M
    from test_mesh_eval_gpu import _blob_mesh
    blob, rec = _blob_mesh(res), _blob_with_stray(res)
    n_blob, n_stray = {48: (2482, 132), 64: (4536, 258)}[res]
    assert blob["verts"].shape[0] == n_blob and rec["verts"].shape[0] == n_blob + n_stray
    rec["colors"] = torch.rand(rec["verts"].shape[0], 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(res))
    out, st = M.keep_components(rec, "largest")
    assert st["n_components"] == 2 and st["kept"].sum() == 1 and 0.9 < st["kept_area_fraction"] < 1
    for k in ("verts", "normals", "faces"):
        assert out[k].dtype == blob[k].dtype and torch.equal(out[k].view(torch.uint8), blob[k].view(torch.uint8)), k
    assert mc_ref.is_closed(out["faces"].cpu().numpy())
    keep_v = st["vertex_comp"] == int(st["kept"].nonzero()[0])
    assert torch.equal(out["colors"], rec["colors"][keep_v])
    again, st2 = M.keep_components(out, "largest")
    assert st2["n_components"] == 1 and all(torch.equal(again[k], out[k]) for k in ("verts", "normals", "faces", "colors"))
    box = ([-1.0, -1.0, -1.0], [-0.5, -0.5, -0.5])
    stray, _ = M.keep_components(rec, "touching", box)
    assert stray["verts"].shape[0] == n_stray and float(stray["verts"].max()) < -0.5
    ref_stray = C.keep_components({k: x.cpu().numpy() for k, x in rec.items()}, "touching", box)[0]
    assert all(np.array_equal(stray[k].cpu().numpy(), ref_stray[k]) for k in ("verts", "normals", "faces", "colors"))
    other, _ = M.keep_components(rec, "not_touching", box)
    assert all(torch.equal(other[k], out[k]) for k in ("verts", "normals", "faces", "colors"))
    with pytest.raises(ValueError):
        M.keep_components(rec, "touching", ([0.9, 0.9, 0.9], [1.0, 1.0, 1.0]))                 # keeps nothing
    with pytest.raises(ValueError):
        M.keep_components({"verts": rec["verts"], "faces": rec["faces"][:0]}, "largest")      # empty
    # numpy in, numpy out; and the command line on files
    as_np, _ = M.keep_components({k: x.cpu().numpy() for k, x in rec.items()}, "largest")
    assert all(isinstance(as_np[k], np.ndarray) and np.array_equal(as_np[k], out[k].cpu().numpy()) for k in out)
    inference.write_ply(tmp_path / "rec.ply", rec)
    M.main([str(tmp_path / "rec.ply"), "--out", str(tmp_path / "clean.ply"), "--keep", "not_touching", "--region", "-1", "-1", "-1",
            "-0.5", "-0.5", "-0.5"])
    back = inference.read_ply(tmp_path / "clean.ply")
    assert np.array_equal(back["verts"], blob["verts"].cpu().numpy()) and np.array_equal(back["faces"], blob["faces"].cpu().numpy())
    assert np.array_equal(back["normals"], blob["normals"].cpu().numpy())
    assert np.array_equal(back["colors"], inference.read_ply(tmp_path / "rec.ply")["colors"][keep_v.cpu().numpy()])
    table = M.main([str(tmp_path / "rec.ply"), "--list"])
    assert table["n_components"] == 2
    with pytest.raises(SystemExit):
        M.main([str(tmp_path / "rec.ply"), "--out", str(tmp_path / "x.ply"), "--keep", "touching", "--region", "0.9", "0.9", "0.9", "1",
                "1", "1"])
    assert not (tmp_path / "x.ply").exists()


# ---- transform and ICP ----------------------------------------------------------------------------------------------------------

def test_transform_mesh_matches_float64_restatement():
    from nicer_slam_amd import mesh_clean as M
    from test_mesh_eval_gpu import _blob_mesh
    m = _blob_mesh(48)
    T = C.similarity([0.3, -1.0, 0.5], 37.0, [0.4, -0.2, 0.9], 1.7)
    got = M.transform_mesh(m, T)
    ref = C.transform_mesh({k: x.cpu().numpy() for k, x in m.items()}, T)
    assert got["verts"].is_cuda and np.array_equal(got["verts"].cpu().numpy(), ref["verts"])
    assert np.abs(got["normals"].cpu().numpy() - ref["normals"]).max() < 1e-6
    assert torch.equal(got["faces"], m["faces"])
    back = M.transform_mesh(got, np.linalg.inv(T))
    assert (back["verts"] - m["verts"]).abs().max() < 1e-6


def test_scaled_icp_matches_oracle():
    from nicer_slam_amd.mesh_eval import icp_point_to_point
    g = np.random.default_rng(0)                                        # the inputs of test_mesh_eval_gpu.test_icp_matches_oracle ...
    tgt = (g.random((4000, 3)) * np.array([1.0, 0.7, 0.4])).astype(np.float32)
    tgt = np.concatenate([tgt, tgt[:1000] * 0.3 + np.array([0.9, 0.1, 0.5], np.float32)])
    T = E.rigid([1.0, 0.3, -0.2], 3.0, [0.03, 0.01, -0.02])
    src = ((E.transform(tgt.astype(np.float64), T) + g.normal(0, 0.002, tgt.shape)) * 1.01).astype(np.float32)   # ... scaled by 1.01
    got = icp_point_to_point(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), 0.05, with_scaling=True)
    ref = C.icp(src, tgt, 0.05, with_scaling=True)
    s = np.linalg.det(got["transformation"][:3, :3]) ** (1 / 3)
    print("scaled icp: iterations", got["iterations"], ref["iterations"], "fitness", got["fitness"], ref["fitness"], "rmse",
          got["inlier_rmse"], ref["inlier_rmse"], "scale", s, "max |dT|", np.abs(got["transformation"] - ref["transformation"]).max())
    assert got["iterations"] == ref["iterations"]
    assert got["fitness"] == ref["fitness"]
    assert got["inlier_rmse"] == pytest.approx(ref["inlier_rmse"], rel=1e-6)
    np.testing.assert_allclose(got["transformation"], ref["transformation"], rtol=0, atol=1e-7)
    assert abs(s - 1 / 1.01) < 1e-3


def test_scaled_icp_recovers_a_similarity_and_rigid_icp_cannot():
    from nicer_slam_amd.mesh_eval import icp_point_to_point
    from test_mesh_eval_gpu import _blob_mesh
    v = _blob_mesh(64)["verts"]
    T = C.similarity([0.2, 1.0, -0.4], 3.0, [0.02, -0.01, 0.015], 1.04)
    src = torch.from_numpy(E.transform(v.cpu().numpy().astype(np.float64), T).astype(np.float32)).cuda()
    out = icp_point_to_point(src, v, 0.1, with_scaling=True)
    err = np.abs(out["transformation"] - np.linalg.inv(T)).max()
    rigid = icp_point_to_point(src, v, 0.1)
    err_rigid = np.abs(rigid["transformation"] - np.linalg.inv(T)).max()
    print("similarity recovery: with scaling", err, "iterations", out["iterations"], "rigid", err_rigid)
    assert err < 1e-4 and out["fitness"] == 1.0, out
    assert err_rigid > 1e-2, rigid


# ---- end to end -----------------------------------------------------------------------------------------------------------------

_METRICS = ("accuracy", "completion", "completion ratio", "normals", "chamfer-L1", "chamfer-L2", "f-score", "f-score-15", "f-score-20")


def test_mesh_metrics_with_clean_equals_the_clean_mesh():
    from nicer_slam_amd import mesh_eval as M
    from test_mesh_eval_gpu import _blob_mesh
    gt, rec = _blob_mesh(64), _blob_with_stray(64)
    same = M.mesh_metrics(gt, gt, align=False)
    cleaned = M.mesh_metrics(rec, gt, align=False, clean="largest")
    dirty = M.mesh_metrics(rec, gt, align=False)
    assert cleaned["components"] == 2 and 0.9 < cleaned["kept area fraction"] < 1 and "components" not in dirty
    for k in _METRICS:
        assert cleaned[k] == same[k], k
    other = M.mesh_metrics(rec, gt, align=False, clean="not_touching", region=([-1, -1, -1], [-0.5, -0.5, -0.5]))
    assert all(other[k] == same[k] for k in _METRICS)
    area = float(C.component_stats(gt["verts"].cpu().numpy(), gt["faces"].cpu().numpy())["area"].sum())
    spacing = math.sqrt(area / 200000)
    print("stray: accuracy", dirty["accuracy"], "cleaned", cleaned["accuracy"], "completion", dirty["completion"], cleaned["completion"],
          "spacing", spacing)
    assert dirty["accuracy"] >= 0.04
    assert 0 < dirty["completion"] < spacing and 0 < cleaned["completion"] < spacing


def test_mesh_metrics_similarity_chain_and_command_line(tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_clean, mesh_eval as M
    from test_mesh_eval_gpu import _blob_mesh
    gt = _blob_mesh(64)
    S = C.similarity([0.3, -1.0, 0.5], 37.0, [0.4, -0.2, 0.9], 1.7)
    D = C.similarity([0.2, 1.0, -0.4], 2.0, [0.01, -0.005, 0.0], 1.02)
    rec = mesh_clean.transform_mesh(gt, np.linalg.inv(S) @ np.linalg.inv(D))
    area = float(C.component_stats(gt["verts"].cpu().numpy(), gt["faces"].cpu().numpy())["area"].sum())
    spacing = math.sqrt(area / 200000)
    scaled = M.mesh_metrics(rec, gt, pre_transform=S, align=True, adjust_scale=True)
    rigid = M.mesh_metrics(rec, gt, pre_transform=S, align=True, adjust_scale=False)
    print("similarity chain: spacing", spacing, "accuracy scaled", scaled["accuracy"], "rigid", rigid["accuracy"], "|T - D|",
          np.abs(scaled["transformation"] - D).max(), np.abs(rigid["transformation"] - D).max())
    assert 0 < scaled["accuracy"] < spacing, (scaled["accuracy"], spacing)
    assert rigid["accuracy"] > spacing, (rigid["accuracy"], spacing)
    with pytest.raises(ValueError):
        M.mesh_metrics(rec, gt, pre_transform=np.diag([1.0, 2.0, 1.0, 1.0]))
    # the command line on files: a stray component on top, removed by --clean
    dirty = mesh_clean.transform_mesh(_blob_with_stray(64), np.linalg.inv(S) @ np.linalg.inv(D))
    inference.write_ply(tmp_path / "rec.ply", dirty)
    inference.write_ply(tmp_path / "gt.ply", gt)
    np.save(tmp_path / "sim3.npy", S)
    expect = M.mesh_metrics(inference.read_ply(tmp_path / "rec.ply"), inference.read_ply(tmp_path / "gt.ply"), pre_transform=S,
                            clean="largest", adjust_scale=True)
    got = M.main([str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "--sim3", str(tmp_path / "sim3.npy"), "--clean", "largest",
                  "--adjust-scale"])
    text = capsys.readouterr().out
    assert all(got[k] == expect[k] for k in _METRICS) and got["components"] == 2
    assert f"accuracy:  {expect['accuracy'] * 100} cm" in text and "components: 2" in text
    assert 0 < got["accuracy"] < spacing
