"""Point-to-plane registration on the device (csrc/mesh_register.hip, nicer_slam_amd/mesh_register.py) against the numpy
statement in tests/register_ref.py: the thirty sums and two counts bit for bit at every n where the order changes shape, the move bit
for bit, the whole loop without a tolerance, and the conditions the reference is pinned to in tests/test_mesh_register_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import eval_ref as E
import register_ref as R

pytestmark = pytest.mark.gpu

KERNELS = ("l2", ("huber", R.K_EXACT), ("tukey", R.K_EXACT))
# where the order changes shape: one lane, one row short of / exactly / one past a row per lane, the same around one tile, and three levels
SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 4096 * 256 + 1]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _assert_system(got, ref, what):
    assert (got["k_corr"], got["k_used"]) == (ref["k_corr"], ref["k_used"]), what
    bad = np.nonzero(_bits(got["sums"]) != _bits(ref["sums"]))[0]
    assert bad.size == 0, (what, bad.tolist(), got["sums"][bad], ref["sums"][bad])
    assert np.array_equal(got["A"], ref["A"]) and np.array_equal(got["b"], ref["b"]), what


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", ["cloud", "surface"])
def test_plane_system_equals_the_reference_bit_for_bit(mode, n):
    """every third row without a correspondence, zero and NaN normals (cloud), a face without area (surface), rows with |r| == k"""
    from nicer_slam_amd.mesh_register import plane_system
    args = (R.synthetic_cloud if mode == "cloud" else R.synthetic_surface)(n, seed=n % 1000)
    dev = {k: torch.from_numpy(v).cuda() for k, v in args.items()}
    rows = R.cloud_rows(**args) if mode == "cloud" else R.surface_rows(**args)
    for kernel in KERNELS:
        _assert_system(plane_system(kernel=kernel, **dev), R.system_from_rows(*rows, kernel), (mode, n, kernel))


@pytest.mark.parametrize("mode", ["cloud", "surface"])
def test_plane_system_without_any_correspondence(mode):
    from nicer_slam_amd.mesh_register import plane_system
    for n in (1, 4097):
        args = (R.synthetic_cloud if mode == "cloud" else R.synthetic_surface)(n, drop="all")
        got = plane_system(kernel=("tukey", R.K_EXACT), **args)
        assert got["k_corr"] == 0 and got["k_used"] == 0 and not _bits(got["sums"]).any()        # thirty times +0.0
        _assert_system(got, R.plane_system(kernel=("tukey", R.K_EXACT), **args), (mode, n))


@pytest.mark.parametrize("n", [4097, 3 * 4096 + 5])
def test_plane_system_on_the_large_coordinate_rows(n):
    """the rows on which a reference with another order, or with one fused multiply-add in r, differs in the bits
    (test_mesh_register_cpu.py)"""
    from nicer_slam_amd.mesh_register import plane_system
    args = R.large_coordinate_cloud(n)
    for kernel in ("l2", ("huber", 1e-6), ("tukey", 3e-6)):
        _assert_system(plane_system(kernel=kernel, **args), R.plane_system(kernel=kernel, **args), (n, kernel))


def test_plane_system_takes_bad_indices_as_no_correspondence():
    from nicer_slam_amd.mesh_register import plane_system
    args = R.synthetic_cloud(300, seed=11)
    args["idx"][::5] = 1000                                                            # one past the last target
    args["idx"][1::7] = -5
    _assert_system(plane_system(**args), R.plane_system(**args), "cloud")
    args = R.synthetic_surface(300, seed=11)
    args["face_idx"][::5] = 500
    args["faces"][7] = (0, 1, 300)                                                     # a face with an index past the last vertex
    args["face_idx"][2::9] = 7
    _assert_system(plane_system(**args), R.plane_system(**args), "surface")


@pytest.mark.parametrize("n", [1, 257])
def test_transform_equals_the_reference_and_its_fp32_rounding(n):
    from nicer_slam_amd.mesh_register import _move
    g = np.random.default_rng(n)
    p = g.normal(0, 3, (n, 3))
    T = E.rigid([0.3, -1.0, 0.5], 7.0, [0.1, -0.2, 0.05])
    cur = torch.from_numpy(p).cuda()
    cur32 = torch.zeros(n, 3, device="cuda")
    _move(cur, T, cur32)
    ref = E.transform(p, T)
    assert np.array_equal(_bits(cur.cpu().numpy()), _bits(ref))
    assert np.array_equal(cur32.cpu().numpy().view(np.uint32), ref.astype(np.float32).view(np.uint32))


# ---- the whole loop ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _box():
    return R.box_case()


def _cuda_box():
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in _box().items() if k != "truth"}


@functools.lru_cache(maxsize=None)
def _device_run(mode, max_corr):
    from nicer_slam_amd.mesh_register import icp_point_to_plane
    c = _cuda_box()
    if mode == "cloud":
        return icp_point_to_plane(c["source"], c["target"], c["normals"], max_corr)
    return icp_point_to_plane(c["source"], (c["verts"], c["faces"]), None, max_corr)


@pytest.mark.parametrize("mode, max_corr", [("cloud", 0.1), ("cloud", 0.03), ("surface", 0.1)])
def test_loop_equals_the_reference_exactly_and_twice(mode, max_corr):
    from nicer_slam_amd.mesh_register import icp_point_to_plane
    c = _box()
    if mode == "cloud":
        ref = R.icp_point_to_plane(c["source"], c["target"], c["normals"], max_corr)
    else:
        ref = R.icp_point_to_plane(c["source"], (c["verts"], c["faces"]), None, max_corr)
    got = _device_run(mode, max_corr)
    print(mode, max_corr, {k: got[k] for k in ("iterations", "fitness", "inlier_rmse", "residual_rmse", "used")})
    for k in ("iterations", "fitness", "inlier_rmse", "residual_rmse", "used", "degenerate"):
        assert got[k] == ref[k], (k, got[k], ref[k])                                    # no tolerance: the order of the sums is fixed
    assert np.array_equal(_bits(got["transformation"]), _bits(ref["transformation"]))
    d = _cuda_box()
    again = (icp_point_to_plane(d["source"], d["target"], d["normals"], max_corr) if mode == "cloud"
             else icp_point_to_plane(d["source"], {"verts": d["verts"], "faces": d["faces"]}, None, max_corr))
    assert np.array_equal(_bits(again["transformation"]), _bits(got["transformation"]))
    assert (again["fitness"], again["inlier_rmse"], again["iterations"]) == (got["fitness"], got["inlier_rmse"], got["iterations"])


def test_loop_with_a_kernel_an_init_and_a_prebuilt_index_equals_the_reference():
    from nicer_slam_amd.mesh_eval import TriIndex
    from nicer_slam_amd.mesh_register import icp_point_to_plane
    c, d = R.box_case(300), None
    init = E.rigid([0, 0, 1], -1.0, [-0.01, 0.0, 0.01])
    ref = R.icp_point_to_plane(c["source"], (c["verts"], c["faces"]), None, 0.1, init=init, kernel=("tukey", 0.03))
    ix = TriIndex(torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["faces"]).cuda())
    got = icp_point_to_plane(c["source"], ix, None, 0.1, init=init, kernel=("tukey", 0.03))
    assert got["iterations"] == ref["iterations"] and got["used"] == ref["used"]
    assert np.array_equal(_bits(got["transformation"]), _bits(ref["transformation"]))


# ---- conditions, on the device ----------------------------------------------------------------------------------------------------

def test_surface_mode_converges_in_six_iterations_below_1e_6():
    out = _device_run("surface", 0.1)
    assert out["iterations"] <= 6 and not out["degenerate"]
    assert np.abs(out["transformation"] - _box()["truth"]).max() < 1e-6


def test_cloud_mode_takes_a_third_of_the_iterations_of_point_to_point():
    from nicer_slam_amd.mesh_eval import icp_point_to_point
    c = _cuda_box()
    point = icp_point_to_point(c["source"], c["target"], 0.1)
    cloud = _device_run("cloud", 0.1)
    assert 3 * cloud["iterations"] <= point["iterations"], (cloud["iterations"], point["iterations"])
    err = lambda r: np.abs(r["transformation"] - _box()["truth"]).max()
    assert err(cloud) < err(point)


def test_degenerate_inputs_on_the_device():
    from nicer_slam_amd.mesh_register import icp_point_to_plane
    from test_mesh_register_cpu import _planes
    for which in (1, 2):
        src, tgt, nrm = _planes(which)
        out = icp_point_to_plane(src, tgt, nrm, 0.1)
        assert out["degenerate"] and out["iterations"] == 0 and np.array_equal(out["transformation"], np.eye(4)), which
        assert out["fitness"] == 1.0 and out["used"] == len(src)
    src = _planes(1)[0]
    v = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    out = icp_point_to_plane(src, (v, f), None, 0.1)
    assert out["degenerate"] and out["iterations"] == 0
    far = icp_point_to_plane(src + np.float32(50), {"verts": v, "faces": f}, None, 0.1)
    assert far["degenerate"] and far["fitness"] == 0.0 and far["inlier_rmse"] == 0.0 and far["used"] == 0
    assert not _device_run("surface", 0.1)["degenerate"] and not _device_run("cloud", 0.1)["degenerate"]


def test_arguments_of_the_public_calls():
    from nicer_slam_amd.mesh_register import icp_point_to_plane, plane_system
    c = _cuda_box()
    with pytest.raises(ValueError):
        icp_point_to_plane(c["source"], c["target"])                                   # a cloud without normals
    with pytest.raises(ValueError):
        icp_point_to_plane(c["source"], (c["verts"], c["faces"]), c["normals"])        # a mesh with normals
    with pytest.raises(ValueError):
        icp_point_to_plane(c["source"], c["target"], c["normals"][:10])
    with pytest.raises(ValueError):
        icp_point_to_plane(c["source"], c["target"], c["normals"], kernel=("huber", 0.0))
    with pytest.raises(ValueError):
        icp_point_to_plane(c["source"][:0], c["target"], c["normals"])
    with pytest.raises(ValueError):
        plane_system(np.zeros((4, 3)))
    zero = icp_point_to_plane(c["source"], c["target"], c["normals"], max_iter=0)
    assert zero["iterations"] == 0 and not zero["degenerate"] and np.array_equal(zero["transformation"], np.eye(4))


# ---- mesh_metrics and the command line --------------------------------------------------------------------------------------------

MOTION = E.rigid([0.2, 1.0, -0.4], 3.0, [0.03, -0.02, 0.025])


@functools.lru_cache(maxsize=None)
def _blob_pair():
    from test_mesh_eval_gpu import _blob_mesh
    gt = _blob_mesh(48)
    moved = torch.from_numpy(E.transform(gt["verts"].cpu().numpy().astype(np.float64), MOTION).astype(np.float32)).cuda()
    return {"verts": moved, "faces": gt["faces"]}, {"verts": gt["verts"], "faces": gt["faces"]}


def test_mesh_metrics_surface_icp_recovers_a_known_motion():
    from nicer_slam_amd import mesh_eval as M
    rec, gt = _blob_pair()
    out = M.mesh_metrics(rec, gt, n_points=2000, icp="surface")
    assert out["icp"] == "surface" and out["icp degenerate"] is False
    assert np.abs(out["transformation"] - np.linalg.inv(MOTION)).max() < 1e-6, np.abs(out["transformation"] - np.linalg.inv(MOTION)).max()
    plane = M.mesh_metrics(rec, gt, n_points=2000, icp="plane")
    assert plane["icp"] == "plane" and plane["icp fitness"] == 1.0 and np.isfinite(plane["transformation"]).all()


def test_mesh_metrics_default_is_the_point_path_and_scale_needs_it():
    from nicer_slam_amd import mesh_eval as M
    rec, gt = _blob_pair()
    a, b = M.mesh_metrics(rec, gt, n_points=2000), M.mesh_metrics(rec, gt, n_points=2000, icp="point")
    assert list(a) == list(b) and "icp" not in a
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])) if k == "transformation" else a[k] == b[k], k
    for icp in ("plane", "surface"):
        with pytest.raises(ValueError):
            M.mesh_metrics(rec, gt, n_points=2000, icp=icp, adjust_scale=True)
    with pytest.raises(ValueError):
        M.mesh_metrics(rec, gt, n_points=2000, icp="symmetric")


def test_command_line(tmp_path, capsys):
    import json
    from nicer_slam_amd import inference, mesh_register
    rec, gt = _blob_pair()
    for name, m in (("src.ply", rec), ("tgt.ply", gt)):
        inference.write_ply(str(tmp_path / name), {"verts": m["verts"].cpu(), "faces": m["faces"].cpu(), "normals": torch.zeros_like(m["verts"]).cpu()})
    r = mesh_register.main([str(tmp_path / "src.ply"), str(tmp_path / "tgt.ply"), "--kernel", "huber:0.05", "--json",
                            "--out-transform", str(tmp_path / "T.npy"), "--out", str(tmp_path / "moved.ply")])
    printed = json.loads(capsys.readouterr().out)
    assert printed["iterations"] == r["iterations"] and np.array_equal(np.array(printed["transformation"]), r["transformation"])
    assert np.array_equal(np.load(tmp_path / "T.npy"), r["transformation"])
    assert np.abs(r["transformation"] - np.linalg.inv(MOTION)).max() < 1e-6
    moved = inference.read_ply(str(tmp_path / "moved.ply"))["verts"]
    # an entry of the 4x4 off by < 1e-6 moves a point of the unit cube by < 4e-6; two fp32 roundings of coordinates below 1 add 1.2e-7
    assert np.abs(moved - gt["verts"].cpu().numpy()).max() < 4e-6 + 1.2e-7
    plane = mesh_register.main([str(tmp_path / "src.ply"), str(tmp_path / "tgt.ply"), "--metric", "plane"])
    assert plane["fitness"] == 1.0 and not plane["degenerate"]
