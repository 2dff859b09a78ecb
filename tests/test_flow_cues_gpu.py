"""The flow ground-truth kernels (C ABI Section 13: csrc/flow_cues.hip, nicer_slam_amd/flow_cues.py) on the GPU against the float64
restatement tests/flow_ref.py, on the cases of tests/flow_cases.py (whose conditions tests/test_flow_cues_cpu.py asserts)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import flow_cases as C
import flow_ref as R
from helpers import assert_close

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(case, unrounded float64 flows [2, H, W, 2], valid [2, H, W]) of a two-frame case: edge 0 is 0 -> 1, edge 1 is 1 -> 0."""
    c = C.case(name)
    fl, ok = R.induced_flow_ref(c["depth"], c["c2w"], c["K"], [0, 1], [1, 0])
    return c, fl, ok


def _check_flow(flow, valid, ref, ok, what):
    flow, valid = flow.cpu().numpy(), valid.cpu().numpy()
    assert flow.dtype == np.float32 and valid.dtype == np.uint8
    assert np.array_equal(valid != 0, ok), what
    assert set(np.unique(valid)) <= {0, 1}
    err = np.abs(flow.astype(np.float64) - ref)
    tol = ULP * np.maximum(1.0, np.abs(ref))
    print(f"{what}: max err / tol {np.max(err / tol):.3f}, max |flow| {np.abs(ref).max():.2f}, invalid {1 - ok.mean():.3f}")
    assert (err <= tol).all(), what
    assert (flow[~ok] == 0).all(), what


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_induced_flow_matches_float64(name):
    from nicer_slam_amd.flow_cues import induced_flow
    c, fl, ok = _ref(name)
    flow, valid = induced_flow(c["depth"], c["c2w"], c["K"], [0, 1], [1, 0])
    assert flow.shape == (2, c["H"], c["W"], 2) and valid.shape == (2, c["H"], c["W"])
    _check_flow(flow, valid, fl, ok, name)


def test_induced_flow_seven_edges_repeated_frames_per_frame_intrinsics():
    from nicer_slam_amd.flow_cues import induced_flow
    m = C.many_edges()
    fl, ok = R.induced_flow_ref(m["depth"], m["c2w"], m["K"], m["src"], m["dst"])
    flow, valid = induced_flow(torch.from_numpy(m["depth"]).cuda(), torch.from_numpy(m["c2w"]), m["K_matrices"], torch.tensor(m["src"]),
                               np.array(m["dst"]))
    _check_flow(flow, valid, fl, ok, "seven edges")
    # near: a pixel counts only when it lies more than `near` in front of the target camera
    fl2, ok2 = R.induced_flow_ref(m["depth"], m["c2w"], m["K"], m["src"], m["dst"], near=1.7)
    assert 0.05 < (ok & ~ok2).mean() < 0.9
    flow, valid = induced_flow(m["depth"], m["c2w"], m["K_matrices"], m["src"], m["dst"], near=1.7)
    _check_flow(flow, valid, fl2, ok2, "seven edges, near = 1.7")
    e, v = induced_flow(m["depth"], m["c2w"], m["K_matrices"], [], [])
    assert e.shape == (0, m["H"], m["W"], 2) and v.shape == (0, m["H"], m["W"])


def _check_masks(got, ref, margin, eps, what, allow_skips=True):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    skip = margin < eps
    print(f"{what}: occluded {ref.mean():.3f}, skipped {skip.mean():.5f}, differing outside the skips {((got != 0) != ref)[~skip].sum()}")
    assert skip.mean() <= 0.01, what
    if not allow_skips:
        assert not skip.any(), what
    assert np.array_equal((got != 0)[~skip], ref[~skip]), what


@pytest.mark.parametrize("with_valid", [False, True])
def test_consistency_alone_on_random_flows(with_valid):
    from nicer_slam_amd.flow_cues import consistency
    fwd, bwd, fv, bv = C.random_flows()
    valid = (fv, bv) if with_valid else (None, None)
    fo, bo, fm, bm = R.consistency_ref(fwd, bwd, *valid)
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    gf, gb = consistency(t(fwd), t(bwd), t(valid[0]), t(valid[1]))
    _check_masks(gf, fo, fm, 1e-6, f"random fwd, validity {with_valid}")
    _check_masks(gb, bo, bm, 1e-6, f"random bwd, validity {with_valid}")
    # other thresholds, and a single [H, W, 2] pair
    fo, bo, fm, bm = R.consistency_ref(fwd[:1], bwd[:1], alpha=0.05, beta=0.25)
    gf, gb = consistency(t(fwd[0]), t(bwd[0]), alpha=0.05, beta=0.25)
    _check_masks(gf, fo, fm, 1e-6, "alpha 0.05 beta 0.25 fwd")
    _check_masks(gb, bo, bm, 1e-6, "alpha 0.05 beta 0.25 bwd")


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_consistency_alone_on_the_same_fp32_flows(name):
    from nicer_slam_amd.flow_cues import consistency
    c, fl, ok = _ref(name)
    f32 = fl.astype(np.float32)
    fo, bo, fm, bm = R.consistency_ref(f32[:1], f32[1:], ok[:1], ok[1:])
    t = lambda a: torch.from_numpy(a).cuda()
    gf, gb = consistency(t(f32[:1]), t(f32[1:]), t(ok[:1]), t(ok[1:]))
    _check_masks(gf, fo, fm, 1e-6, name + " fwd")
    _check_masks(gb, bo, bm, 1e-6, name + " bwd")


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_pipeline_matches_the_float64_pipeline(name):
    """pair_cues (flows rounded to fp32 between the two kernels) against the float64 pipeline on unrounded flows: the rounding of a
    64-pixel flow is 4e-6, so only a pixel within 1e-3 of a threshold may differ, and the analytic pairs have none."""
    from nicer_slam_amd.flow_cues import pair_cues
    c, fl, ok = _ref(name)
    fo, bo, fm, bm = R.consistency_ref(fl[:1], fl[1:], ok[:1], ok[1:])
    flow, occ = pair_cues(c["depth"], c["c2w"], c["K"], [(0, 1), (1, 0), (0, 1)])            # (a repeated pair: computed once)
    assert flow.shape == (3, c["H"], c["W"], 2) and occ.shape == (3, c["H"], c["W"])
    err = np.abs(flow[:2].cpu().numpy().astype(np.float64) - fl)
    assert (err <= ULP * np.maximum(1.0, np.abs(fl))).all()
    assert torch.equal(flow[2], flow[0]) and torch.equal(occ[2], occ[0])
    _check_masks(occ[0:1], fo, fm, 1e-3, name + " fwd", allow_skips=name not in C.ANALYTIC)
    _check_masks(occ[1:2], bo, bm, 1e-3, name + " bwd", allow_skips=name not in C.ANALYTIC)
    rev_flow, rev_occ = pair_cues(c["depth"], c["c2w"], c["K"], [(1, 0)])                     # one direction asked for
    assert torch.equal(rev_flow[0], flow[1]) and torch.equal(rev_occ[0], occ[1])


def test_select_is_torch_indexing():
    from nicer_slam_amd.flow_cues import FlowStore
    E, n, b = 5, 97, 4
    H, W = C.SIZES["odd"]
    g = torch.Generator().manual_seed(11)
    flows = (torch.randn(E, H * W, 2, generator=g) * 10).cuda()
    masks = (torch.rand(E, H * W, generator=g) > 0.4).cuda()
    s = torch.randint(H * W, (b, n), generator=g)
    s[:, 0], s[:, 1], s[:, 2], s[:, 3] = 0, H * W - 1, -1, H * W
    s[1, 40], s[3, 41] = -(2 ** 40), 2 ** 40
    idii = torch.tensor([0, 2, 2, 3, 0])
    store = FlowStore(flows, masks, H, W)
    f, m = store.select(s, idii)
    rf, rm = R.select_ref(flows, masks, s.cuda(), idii.cuda())
    assert f.shape == (E, n, 2) and f.dtype == torch.float32 and m.shape == (E, n) and m.dtype == torch.bool
    assert torch.equal(f, rf) and torch.equal(m, rm)
    outside = ((s < 0) | (s >= H * W))[idii]
    assert outside.sum() >= 2 * E + 1
    assert (f.cpu()[outside] == 0).all() and not m.cpu()[outside].any()
    inside = ~outside
    e = torch.arange(E)[:, None].expand(E, n)
    assert torch.equal(f.cpu()[inside], flows.cpu()[e[inside], s[idii][inside]])             # plain indexing, bit for bit
    f2, m2 = store.select(s.cuda(), idii.cuda().to(torch.int32))                              # device indices, any integer type
    assert torch.equal(f2, f) and torch.equal(m2, m)
    with pytest.raises(ValueError, match="idii"):
        store.select(s, idii[:2])
    with pytest.raises(ValueError, match="sampling_idx"):
        store.select(s[0], idii)
    f0, m0 = store.select(s[:, :0], idii)                                                     # n = 0: a no-op
    assert f0.shape == (E, 0, 2) and m0.shape == (E, 0)


def test_files_written_from_device_results_read_back_the_same(tmp_path):
    from nicer_slam_amd.flow_cues import FlowStore, build_graph, pair_cues, write_pair
    t = C.three_frames()
    edges = build_graph([0, 10, 20])
    store = FlowStore.from_depth(t["depth_holes"], t["c2w"], t["K"], edges)
    flow, occ = pair_cues(t["depth_holes"], t["c2w"], t["K"], [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)])
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        write_pair(tmp_path, 10 * i, 10 * j, flow[2 * k], flow[2 * k + 1], occ[2 * k], occ[2 * k + 1], compress=k != 1)
        write_pair(tmp_path, 10 * j, 10 * i, flow[2 * k + 1], flow[2 * k], occ[2 * k + 1], occ[2 * k], compress=k != 1)
    back = FlowStore.from_dir(tmp_path, edges)
    assert (back.H, back.W) == (store.H, store.W) == (t["H"], t["W"])
    assert back.flows.is_cuda and torch.equal(back.flows, store.flows) and torch.equal(back.masks, store.masks)
    assert 0.05 < 1.0 - store.masks.float().mean().item() < 0.6


def test_command_line_writes_the_pair_directory(tmp_path):
    """python -m nicer_slam_amd.flow_cues (in process): depth .npy frames + poses -> the files of pair_list(n, interval, rad), which
    FlowStore.from_dir reads back as FlowStore.from_depth makes them."""
    from nicer_slam_amd import flow_cues as fc
    t = C.three_frames()
    os.makedirs(tmp_path / "depth")
    for k, d in enumerate(t["depth_holes"]):
        np.save(tmp_path / "depth" / f"{k:06d}.npy", d)
    np.save(tmp_path / "poses.npy", t["c2w"])
    out = str(tmp_path / "seq_pair")
    fc.main(["--depth", str(tmp_path / "depth"), "--poses", str(tmp_path / "poses.npy"), "--intrinsics", *[repr(float(x)) for x in t["K"]],
             "--out", out, "--interval", "1", "--rad", "2"])
    pairs = fc.pair_list(3, 1, 2)
    assert pairs == [(1, 0), (0, 1), (2, 0), (0, 2), (2, 1), (1, 2)]
    assert sorted(os.listdir(out)) == sorted(f"{i:04d}_{j:04d}_{tag}" for i, j in pairs
                                             for tag in ("flow.npy", "flow_bwd.npy", "occ.png", "occ_bwd.png"))
    ii, jj = [p[0] for p in pairs], [p[1] for p in pairs]
    back = fc.FlowStore.from_dir(out, (ii, jj))
    store = fc.FlowStore.from_depth(t["depth_holes"], t["c2w"], t["K"], (ii, jj))
    assert torch.equal(back.flows, store.flows) and torch.equal(back.masks, store.masks)
    f, fb, o, ob = fc.read_pair(out, 2, 0)
    f2, fb2, o2, ob2 = fc.read_pair(out, 0, 2)
    assert np.array_equal(f, fb2) and np.array_equal(fb, f2) and np.array_equal(o, ob2) and np.array_equal(ob, o2)


def test_store_feeds_the_flow_term_end_to_end():
    """Keyframes 0, 10, 20: build_graph -> FlowStore.from_depth (sensor depth, with holes) -> select at 128 pixels per frame, against
    the renderer's flow (fused.warp.flow) of the true surface, t = d |v|^2.  Where the store says usable the two agree to the
    tolerance of tests/test_warp_gpu.py; the rectangle's shadow is masked; and without the mask the comparison fails (the holes carry
    flow 0), so the mask is what makes the term sound."""
    from nicer_slam_amd.flow_cues import FlowStore, build_graph
    from nicer_slam_amd.fused import warp as fw
    t = C.three_frames()
    H, W = t["H"], t["W"]
    fx, fy, cx, cy = t["K"]
    edges = build_graph([0, 10, 20])
    assert edges[2].tolist() == [0, 0, 10, 10, 20, 20] and edges[3].tolist() == [10, 20, 0, 20, 0, 10]
    store = FlowStore.from_depth(t["depth_holes"], t["c2w"], t["K"], edges)
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(H * W, (3, 128), generator=g)
    gt_flow, gt_mask = store.select(idx, edges[0])
    assert gt_flow.shape == (6, 128, 2) and gt_mask.shape == (6, 128)

    uv = torch.stack([(idx % W).double(), (idx // W).double()], -1)
    d = torch.from_numpy(t["depth"].astype(np.float64)).reshape(3, -1).gather(1, idx)
    v2 = ((uv[..., 0] - cx) / fx) ** 2 + ((uv[..., 1] - cy) / fy) ** 2 + 1.0
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    f32 = lambda x: x.to(torch.float32).cuda()
    rendered = fw.flow(SimpleNamespace(H=H, W=W), f32(uv), f32(torch.from_numpy(t["c2w"])), f32(K[None].repeat(3, 1, 1)),
                       f32(d * v2), edges)
    m = gt_mask.cpu()
    assert 0.3 < m.float().mean().item() < 0.95
    assert_close(rendered.cpu()[m], gt_flow.cpu()[m], 5e-3, 2e-5, "flow on usable pixels")
    with pytest.raises(AssertionError):
        assert_close(rendered, gt_flow, 5e-3, 2e-5, "flow without the mask")

    n_hidden = 0
    for e, (i, j) in enumerate(zip(edges[0].tolist(), edges[1].tolist())):
        hidden = torch.from_numpy(C.hidden_behind_rectangle(t["c2w"][i], t["c2w"][j], t["depth"][i], t["K"])).reshape(-1)[idx[i]]
        n_hidden += int(hidden.sum())
        assert not m[e][hidden].any(), f"edge {e}: a pixel in the rectangle's shadow is marked usable"
    assert n_hidden >= 6
