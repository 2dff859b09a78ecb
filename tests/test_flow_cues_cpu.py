"""Flow ground truth from depth and poses (C ABI Section 13, nicer_slam_amd/flow_cues.py) -- what needs no GPU: the float64
restatement (tests/flow_ref.py) against closed forms and against the renderer's flow_reproject, the reference's pair lists and
files, argument validation of the three entry points, and the conditions of the cases the GPU tests lean on."""
import ctypes
import lzma
import os

import numpy as np
import pytest
import torch

import flow_cases as C
import flow_ref as R


def _both(name):
    c = C.case(name)
    fl, ok = R.induced_flow_ref(c["depth"], c["c2w"], c["K"], [0, 1], [1, 0])
    return c, fl, ok


def test_identity_pose_gives_zero_flow_and_nothing_occluded():
    c, fl, ok = _both("identity")
    assert ok.all()
    assert np.abs(fl).max() < 1e-12
    fo, bo, _, _ = R.consistency_ref(fl[:1], fl[1:], ok[:1], ok[1:])
    assert not fo.any() and not bo.any()


def test_fronto_parallel_plane_under_x_translation_closed_form():
    H, W, d, tx, fx = 11, 17, 2.5, 0.3, 60.0
    depth = np.full((2, H, W), d, np.float32)
    c2w = np.stack([np.eye(4), np.eye(4)])
    c2w[1, 0, 3] = tx
    fl, ok = R.induced_flow_ref(depth, c2w, [fx, 55.0, 8.0, 5.0], [0, 1], [1, 0])
    assert ok.all()
    assert np.abs(fl[0, ..., 0] + fx * tx / d).max() < 1e-12 and np.abs(fl[0, ..., 1]).max() < 1e-12
    assert np.abs(fl[1, ..., 0] - fx * tx / d).max() < 1e-12 and np.abs(fl[1, ..., 1]).max() < 1e-12


@pytest.mark.parametrize("name", ["lateral", "forward_odd"])
def test_renderer_flow_reproject_is_the_same_quantity(name):
    """flow_reproject(uv, pose, K, t, edges) with t = d |v|^2 (v the unnormalised world ray through the pixel at z = 1: get_camera_params
    divides the direction by its SQUARED norm) is the induced flow at the sampled pixels.  flow_reproject divides by (z + 1e-8)
    (network.py:165), a term the geometric flow does not have; it scales the projected pixel by z / (z + 1e-8), which the comparison
    takes out exactly before asking for 1e-9 (left in, it shows as up to ~4e-7 px here -- also asserted, as a bound on the term)."""
    from nicer_slam_amd.model.warp import flow_reproject
    c, fl, ok = _both(name)
    H, W = c["H"], c["W"]
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(H * W, (2, 200), generator=g)
    uv = torch.stack([(idx % W).double(), (idx // W).double()], -1)
    fx, fy, cx, cy = c["K"]
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    K = K[None].repeat(2, 1, 1)
    pose = torch.from_numpy(c["c2w"].copy())
    d = torch.from_numpy(c["depth"].astype(np.float64)).reshape(2, -1).gather(1, idx)
    v2 = ((uv[..., 0] - cx) / fx) ** 2 + ((uv[..., 1] - cy) / fy) ** 2 + 1.0          # |v|^2 (a rotation keeps it)
    edges = (torch.tensor([0, 1]), torch.tensor([1, 0]))
    got = flow_reproject(uv, pose, K, d * v2, edges)
    ref = torch.from_numpy(fl).reshape(2, H * W, 2).gather(1, idx[..., None].expand(-1, -1, 2))
    raw = (got - ref).abs().max().item()
    # the target depth z of every sample, from the restatement's own geometry
    z = []
    for e, (i, j) in enumerate(((0, 1), (1, 0))):
        cam = torch.stack([(uv[i, :, 0] - cx) / fx * d[i], (uv[i, :, 1] - cy) / fy * d[i], d[i], torch.ones_like(d[i])], -1)
        z.append((cam @ pose[i].T @ torch.linalg.inv(pose[j]).T)[:, 2])
    z = torch.stack(z)[..., None]
    undone = (got + uv) * (z + 1e-8) / z - uv
    err = (undone - ref).abs().max().item()
    print(f"{name}: max |flow_reproject - restatement| raw {raw:.3e}, with the 1e-8 of the division taken out {err:.3e}")
    assert err < 1e-9
    assert raw < 1e-6


def test_pair_list_is_the_reference_list():
    from nicer_slam_amd.flow_cues import pair_list
    assert pair_list(45) == [(10, 0), (0, 10), (20, 0), (0, 20), (20, 10), (10, 20), (30, 0), (0, 30), (30, 10), (10, 30), (30, 20),
                             (20, 30), (40, 10), (10, 40), (40, 20), (20, 40), (40, 30), (30, 40)]
    assert pair_list(1) == [] and pair_list(10) == [] and pair_list(11) == [(10, 0), (0, 10)]
    assert pair_list(25, interval=5, rad=0) == [(5, 0), (0, 5), (10, 5), (5, 10), (15, 10), (10, 15), (20, 15), (15, 20)]


def test_build_graph_is_the_reference_graph():
    from nicer_slam_amd.flow_cues import build_graph
    idii, idjj, ii, jj = build_graph([0, 10, 20, 25, 40, 50], device="cpu")
    assert idii.tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 2, 4, 4, 4, 5, 5]
    assert idjj.tolist() == [1, 2, 0, 2, 4, 0, 1, 4, 5, 1, 2, 5, 2, 4]
    assert ii.tolist() == [0, 0, 10, 10, 10, 20, 20, 20, 20, 40, 40, 40, 50, 50]
    assert jj.tolist() == [10, 20, 0, 20, 40, 0, 10, 40, 50, 10, 20, 50, 20, 40]
    assert all(t.dtype == torch.int64 for t in (idii, idjj, ii, jj))
    a, b, _, _ = build_graph([0, 10, 20, 25, 40, 50], placeholder=3, thresh=10, device="cpu")
    assert a.tolist() == [3, 4, 4, 5, 7, 8] and b.tolist() == [4, 3, 5, 4, 8, 7]
    assert all(t.numel() == 0 for t in build_graph([5, 7], device="cpu"))


@pytest.mark.parametrize("compress", [True, False])
def test_pair_files_round_trip(tmp_path, compress):
    from PIL import Image
    from nicer_slam_amd.flow_cues import read_pair, write_pair
    g = np.random.default_rng(0)
    flow, bwd = (g.normal(size=(2, 9, 13, 2)) * 20).astype(np.float32)
    occ, occ_b = (g.uniform(size=(2, 9, 13)) > 0.6).astype(np.uint8)
    write_pair(tmp_path, 20, 0, torch.from_numpy(flow), bwd, occ, torch.from_numpy(occ_b), compress=compress)
    stem = os.path.join(tmp_path, "0020_0000")
    assert sorted(os.listdir(tmp_path)) == ["0020_0000_flow.npy", "0020_0000_flow_bwd.npy", "0020_0000_occ.png", "0020_0000_occ_bwd.png"]
    if compress:
        with lzma.open(stem + "_flow.npy", "rb") as fh:                   # as extract_flows.py writes and the trainer first tries
            assert np.array_equal(np.load(fh), flow)
    else:
        assert np.array_equal(np.load(stem + "_flow.npy"), flow)
    png = Image.open(stem + "_occ.png")
    assert png.mode == "L" and set(np.unique(np.array(png))) <= {0, 255}
    assert np.array_equal(np.array(png.convert("RGB"))[:, :, 0] == 0, occ == 0)          # the trainer's reading of cv2.imread
    f, b, o, ob = read_pair(tmp_path, 20, 0)
    assert f.dtype == np.float32 and np.array_equal(f, flow) and np.array_equal(b, bwd)
    assert np.array_equal(o, occ) and np.array_equal(ob, occ_b)


def test_section13_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib
    EBADARG = 4
    fake = ctypes.c_void_p(4096)
    ind = lib.nsa_flowcue_induced
    assert ind(None, 2, 48, 64, None, 0, None, None, None, 0, 1e-3, None, None, None) == 0                      # no edges: no-op
    assert ind(None, 2, 48, 64, fake, 0, fake, fake, fake, 3, 1e-3, fake, fake, None) == EBADARG                # NULL depth
    assert ind(fake, 2, 48, 64, fake, 0, fake, fake, fake, 3, 1e-3, None, fake, None) == EBADARG                # NULL output
    assert ind(fake, 0, 48, 64, fake, 0, fake, fake, fake, 3, 1e-3, fake, fake, None) == EBADARG                # no frames
    assert ind(fake, 2, 0, 64, fake, 0, fake, fake, fake, 3, 1e-3, fake, fake, None) == EBADARG                 # empty image
    assert ind(fake, 2, 1 << 16, 1 << 15, fake, 0, fake, fake, fake, 3, 1e-3, fake, fake, None) == EBADARG      # H W >= 2^31
    assert ind(fake, 2, 48, 64, fake, 0, fake, fake, fake, 3, -1.0, fake, fake, None) == EBADARG                # near < 0
    assert ind(fake, 2, 48, 64, fake, 0, fake, fake, fake, 3, float("nan"), fake, fake, None) == EBADARG
    assert ind(fake, 2, 48, 64, fake, 0, ctypes.c_void_p(4100), fake, fake, 3, 1e-3, fake, fake, None) == EBADARG   # misaligned doubles
    assert ind(fake, 2, 48, 64, fake, 0, fake, fake, fake, 6_000_000, 1e-3, fake, fake, None) == EBADARG        # 3 blocks x edges >= 2^24
    con = lib.nsa_flowcue_consistency
    assert con(None, None, None, None, 0, 48, 64, 0.01, 0.5, None, None, None) == 0                             # no pairs: no-op
    assert con(fake, fake, None, None, 2, 1, 64, 0.01, 0.5, fake, fake, None) == EBADARG                        # H < 2
    assert con(fake, fake, None, None, 2, 48, 1, 0.01, 0.5, fake, fake, None) == EBADARG                        # W < 2
    assert con(None, None, None, None, 0, 1, 64, 0.01, 0.5, None, None, None) == EBADARG                        # (even with no pairs)
    assert con(fake, fake, fake, None, 2, 48, 64, 0.01, 0.5, fake, fake, None) == EBADARG                       # one validity map
    assert con(fake, None, None, None, 2, 48, 64, 0.01, 0.5, fake, fake, None) == EBADARG                       # NULL bwd
    assert con(fake, fake, None, None, 2, 48, 64, 0.01, 0.5, fake, None, None) == EBADARG                       # NULL output
    assert con(fake, fake, None, None, 2, 48, 64, -0.01, 0.5, fake, fake, None) == EBADARG
    assert con(fake, fake, None, None, 2, 48, 64, 0.01, float("inf"), fake, fake, None) == EBADARG
    assert con(fake, fake, None, None, 3_000_000, 48, 64, 0.01, 0.5, fake, fake, None) == EBADARG              # 6 blocks x pairs >= 2^24
    sel = lib.nsa_flowcue_select
    assert sel(None, None, 0, 3072, None, 4, 97, None, None, None, None) == 0                                   # no edges: no-op
    assert sel(None, None, 5, 3072, None, 4, 0, None, None, None, None) == 0                                    # n = 0: no-op
    assert sel(fake, fake, 5, 0, fake, 4, 97, fake, fake, fake, None) == EBADARG                                # no pixels
    assert sel(fake, fake, 5, 1 << 31, fake, 4, 97, fake, fake, fake, None) == EBADARG
    assert sel(fake, fake, 5, 3072, fake, 0, 97, fake, fake, fake, None) == EBADARG                             # empty batch
    assert sel(fake, fake, 5, 3072, None, 4, 97, fake, fake, fake, None) == EBADARG                             # NULL indices
    assert sel(fake, None, 5, 3072, fake, 4, 97, fake, fake, fake, None) == EBADARG                             # NULL masks
    assert sel(fake, fake, 1 << 24, 3072, fake, 4, 97, fake, fake, fake, None) == EBADARG                       # a block per edge: 2^24


def test_python_entry_points_reject_bad_arguments_before_the_device():
    from nicer_slam_amd import flow_cues as fc
    c = C.case("lateral")
    with pytest.raises(ValueError, match="frame index"):
        fc.induced_flow(c["depth"], c["c2w"], c["K"], [0, 2], [1, 0], device="cpu")
    with pytest.raises(ValueError, match="edges"):
        fc.induced_flow(c["depth"], c["c2w"], c["K"], [0, 1], [1], device="cpu")
    with pytest.raises(ValueError, match="near"):
        fc.induced_flow(c["depth"], c["c2w"], c["K"], [0], [1], near=-1.0, device="cpu")
    with pytest.raises(ValueError, match="c2w"):
        fc.induced_flow(c["depth"], c["c2w"][:1], c["K"], [0], [0], device="cpu")
    with pytest.raises(ValueError, match="both or neither"):
        fc.consistency(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, 2), torch.ones(1, 4, 4))
    with pytest.raises(ValueError, match="same shape"):
        fc.consistency(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 5, 2))
    with pytest.raises(ValueError, match="2 x 2"):
        fc.consistency(torch.zeros(1, 1, 4, 2), torch.zeros(1, 1, 4, 2))
    with pytest.raises(ValueError, match="itself"):
        fc.pair_cues(c["depth"], c["c2w"], c["K"], [(0, 0)], device="cpu")


def test_host_tensors_of_valid_shape_are_refused_and_nothing_is_launched(monkeypatch):
    """The kernels read device memory.  A host tensor of a valid shape must be refused in Python: no entry point of the library is
    reached (every one is replaced by a function that fails the test)."""
    from nicer_slam_amd import flow_cues as fc

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called with host memory")
    monkeypatch.setattr(fc, "lib", NoLaunch())
    c = C.case("lateral")
    fwd, bwd, fv, bv = C.random_flows()
    with pytest.raises(ValueError, match="device"):
        fc.consistency(torch.from_numpy(fwd), torch.from_numpy(bwd))
    with pytest.raises(ValueError, match="device"):
        fc.consistency(torch.from_numpy(fwd), torch.from_numpy(bwd), torch.from_numpy(fv), torch.from_numpy(bv))
    with pytest.raises(ValueError, match="torch tensors"):
        fc.consistency(fwd, bwd)
    with pytest.raises(ValueError, match="device"):
        fc.FlowStore(torch.zeros(3, 12, 2), torch.ones(3, 12, dtype=torch.bool), 3, 4)
    with pytest.raises(ValueError, match="not a GPU"):
        fc.induced_flow(c["depth"], c["c2w"], c["K"], [0, 1], [1, 0], device="cpu")
    with pytest.raises(ValueError, match="not a GPU"):
        fc.pair_cues(c["depth"], c["c2w"], c["K"], [(0, 1)], device="cpu")


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_case_conditions_the_gpu_tests_lean_on(name):
    """Per case and direction: on the analytic pairs 5 - 60 % of the pixels are occluded (both outcomes are exercised), and at most
    1 % of the pixels lie so close to a threshold that the GPU comparisons may skip them -- on the reference alone."""
    c, fl, ok = _both(name)
    fo, bo, fm, bm = R.consistency_ref(fl[:1], fl[1:], ok[:1], ok[1:])                    # the float64 pipeline, unrounded flows
    f32 = fl.astype(np.float32)
    _, _, fm32, bm32 = R.consistency_ref(f32[:1], f32[1:], ok[:1], ok[1:])                # the consistency kernel's own inputs
    for tag, occ, m, m32 in (("fwd", fo, fm, fm32), ("bwd", bo, bm, bm32)):
        share = occ.mean()
        print(f"{name} {tag}: occluded {share:.3f}, smallest margin {m.min():.2e}, within 1e-3: {(m < 1e-3).mean():.4f}, "
              f"fp32-fed within 1e-6: {(m32 < 1e-6).mean():.4f}")
        if name in C.ANALYTIC:
            assert 0.05 <= share <= 0.60
            assert not (m < 1e-3).any()                                                   # the reference skips none there
        assert (m < 1e-3).mean() <= 0.01 and (m32 < 1e-6).mean() <= 0.01
    if "holes" in name:
        assert 0.02 < 1.0 - ok.mean() < 0.2
        bad = ~np.isfinite(c["depth"]) | (c["depth"] <= 0)
        assert np.array_equal(~ok[0], bad[0]) and np.array_equal(~ok[1], bad[1])          # (nothing is near the camera plane)
        assert np.isnan(c["depth"]).any() and np.isinf(c["depth"]).any() and (c["depth"] == 0).any() and (c["depth"] < 0).any()


def test_random_flow_case_conditions():
    fwd, bwd, fv, bv = C.random_flows()
    assert np.abs(fwd).max() <= 8.0 and np.abs(bwd).max() <= 8.9
    for valid in ((None, None), (fv, bv)):
        fo, bo, fm, bm = R.consistency_ref(fwd, bwd, *valid)
        for occ, m in ((fo, fm), (bo, bm)):
            share = occ[:-1].mean()
            print(f"random flows, validity {valid[0] is not None}: occluded {share:.3f} (smooth pairs), within 1e-6: {(m < 1e-6).mean():.5f}")
            assert 0.2 < share < 0.8 and occ[-1].mean() > 0.9
            assert (m < 1e-6).mean() <= 0.01
