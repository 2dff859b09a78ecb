"""The keyframe re-projection kernels (csrc/warp_terms.hip, C ABI section 5: nsa_patch_warp_forward / _backward, nsa_flow_forward /
_backward, nsa_masked_l1 and the workspace functions) against float64 (tests/warp_ref64.py), row by row, through the C ABI.

The method is tests/test_gemm_float64_gpu.py's, and the gate is tests/gate64.py (its Pool, with a second yardstick where there is one):
  * e_k = |kernel - float64|, e_32 = |fp32 mode of the same restatement - float64| (the yardstick; tests/test_warp_ref64_cpu.py holds
    that mode to model/warp.py and to the golden, and bounds it on these very inputs),
  * per row, divided by the row's norm: `sampled` rows (target, source, pixel) and `flow` rows (edge, pixel) by max(|float64 row|, 1);
    g_depth rows (source, pixel) by the row's cotangent scale; g_pose / g_w2c rows (one image) by the largest cotangent scale among
    the rows that feed the image; a row whose cotangents are all zero must come out exactly 0,
  * gate: rms(e_k) <= 1.5 rms(e_32) and max(e_k) <= 3 max(e_32), every output finite,
  * the small cases (n = 1, b = 1, the 2 x 2 image) and the per-image pose gradients are POOLED over the cases and judged once.

Kernel order.  g_pose and g_w2c are sums over all threads of an image; the kernel adds them as its header documents -- the xor
butterfly over the 64 lanes of a wave, then k_pose_finish's 21 strided groups of wave partials, then the groups in turn -- where
fp32 autograd adds them in torch's order (a matmul backward and a blocked sum).  Both are valid fp32 orders of the same sum, so
these two quantities have a second yardstick in the kernel's order (warp_ref64.pose_grads_kernel_order) and are gated against the
larger of the two (gate64.gate with kernel_order).  sampled, flow and g_depth are per-thread fixed-order expressions and have the one yardstick.

Inputs: tests/warp_cases.py.  Bitwise: gt_rgb; mask and flat outside the exclusions; everything on a second run.  Left out, counted,
printed and capped (warp_cases.exclusions / check_caps, derived from the restatement alone, asserted on the CPU too): g_depth rows
with a sample within delta of a texel boundary (their cotangents are ZERO in every run, so that the image sums of the pose gates
stay comparable, and their g_depth must then be exactly 0), mask entries with gx or gy within delta of +-1 or tz within delta of 0
(at most 1 % of a case's entries), flat rows within the fp32 rounding bound of 0.01.  Such a flat row takes none of its mask entries
out: they are compared bit for bit with the float64 comparisons, the inside test and the flat bit that the kernel itself returned
for the row (warp_cases.expected_mask).  `sampled` is continuous in the coordinate and has no exclusion.

Every backward runs with a workspace of exactly the size this file derives from b, n, patch and ne (and the workspace functions must
return that size), followed by a guard region that must come back untouched.

Measured on MI355X: DESIGN.md section 7 holds the printed table."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import warp_cases as C
import warp_ref64 as R
from devcall import dev, nan, ptr, st
from gate64 import Pool

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NSA_OK, NSA_EBADARG = 0, 4
GUARD = 4096                     # floats behind every workspace
SENTINEL = -7.25e22


def waves(per_image):
    return -(-per_image // 256) * 4


def patch_workspace(b, n, patch, want_pose):
    """floats nsa_patch_warp_backward indexes: g_cell [b,n,p2] (patch > 1), part_src [b][waves][12], part_w2c [b * waves][b][12]"""
    p2 = patch * patch
    w = waves(n * p2)
    return (b * n * p2 if patch > 1 else 0) + (b * w * 12 + b * w * b * 12 if want_pose else 0)


def flow_workspace(b, n, ne, want_pose):
    """part_src [b][waves][12], part_w2c [b * waves][ne][12]"""
    w = waves(n)
    return b * w * 12 + b * w * ne * 12 if want_pose else 0


def l1_workspace(items):
    """(blocks + 1) (sum, count) doubles, counted in floats; blocks = ceil(items / 256) clamped to 1 .. 256"""
    return (min(max(-(-items // 256), 1), 256) + 1) * 4


class Guarded:
    """a workspace of exactly ``size`` floats followed by a guard region filled with a sentinel"""

    def __init__(self, size):
        self.size = size
        self.t = torch.full((size + GUARD,), SENTINEL, device="cuda")

    def ptr(self):
        return self.t.data_ptr() if self.size else None

    def intact(self):
        return bool((self.t[self.size:] == SENTINEL).all())


class DevWarp:
    def __init__(self, c):
        from nicer_slam_amd._native import WarpDesc
        self.c = c
        self.t = {k: dev(c[k]) for k in ("uv", "pose", "w2c", "K", "depth", "images", "depths")}
        self.t["frame_index"] = dev(c["frame_index"], torch.int32)
        t = self.t
        self.desc = WarpDesc(c["b"], c["n"], c["H"], c["W"], ptr(t["uv"]), ptr(t["pose"]), ptr(t["w2c"]), ptr(t["K"]), ptr(t["depth"]),
                             ptr(t["images"]), ptr(t["depths"]), ptr(t["frame_index"]))

    def ref(self):
        return ctypes.byref(self.desc)


def k_warp_forward(dw):
    from nicer_slam_amd._native import lib, check
    c = dw.c
    b, n, patch = c["b"], c["n"], c["patch"]
    p2 = patch * patch
    sampled, gt_rgb = nan(b, b, n, p2, 3), nan(b, b, n, p2, 3)
    mask = torch.full((b, b, n, p2), 0xCC, device="cuda", dtype=torch.uint8)
    flat = torch.full((b, n), 0xCC, device="cuda", dtype=torch.uint8) if patch > 1 else None
    check(lib.nsa_patch_warp_forward(dw.ref(), patch, ptr(sampled), ptr(mask), ptr(gt_rgb), ptr(flat), st()))
    torch.cuda.synchronize()
    return sampled.cpu(), mask.cpu(), gt_rgb.cpu(), None if flat is None else flat.cpu()


def k_warp_backward(dw, g_sampled, want_pose):
    from nicer_slam_amd._native import lib, check
    c = dw.c
    b, n, patch = c["b"], c["n"], c["patch"]
    size = patch_workspace(b, n, patch, want_pose)
    assert int(lib.nsa_patch_warp_workspace(b, n, patch, int(want_pose))) == size, "nsa_patch_warp_workspace"
    ws = Guarded(size)
    g = dev(g_sampled)
    g_depth = nan(b, n)
    g_pose, g_w2c = (nan(b, 4, 4), nan(b, 4, 4)) if want_pose else (None, None)
    check(lib.nsa_patch_warp_backward(dw.ref(), patch, ptr(g), ptr(g_depth), ptr(g_pose), ptr(g_w2c), ws.ptr(), st()))
    torch.cuda.synchronize()
    assert ws.intact(), f"nsa_patch_warp_backward wrote past its {size} workspace floats"
    return g_depth.cpu(), None if g_pose is None else g_pose.cpu(), None if g_w2c is None else g_w2c.cpu()


def k_flow_forward(dw, ii, jj):
    from nicer_slam_amd._native import lib, check
    ne, n = ii.shape[0], dw.c["n"]
    flow = nan(ne, n, 2)
    check(lib.nsa_flow_forward(dw.ref(), ptr(ii), ptr(jj), ne, ptr(flow), st()))
    torch.cuda.synchronize()
    return flow.cpu()


def k_flow_backward(dw, ii, jj, g_flow, want_pose):
    from nicer_slam_amd._native import lib, check
    c = dw.c
    b, n, ne = c["b"], c["n"], ii.shape[0]
    size = flow_workspace(b, n, ne, want_pose)
    assert int(lib.nsa_flow_workspace(b, n, ne, int(want_pose))) == size, "nsa_flow_workspace"
    ws = Guarded(size)
    g = dev(g_flow)
    g_depth = nan(b, n)
    g_pose, g_w2c = (nan(b, 4, 4), nan(b, 4, 4)) if want_pose else (None, None)
    check(lib.nsa_flow_backward(dw.ref(), ptr(ii) if ne else None, ptr(jj) if ne else None, ne, ptr(g) if ne else None, ptr(g_depth),
                                ptr(g_pose), ptr(g_w2c), ws.ptr(), st()))
    torch.cuda.synchronize()
    assert ws.intact(), f"nsa_flow_backward wrote past its {size} workspace floats"
    return g_depth.cpu(), None if g_pose is None else g_pose.cpu(), None if g_w2c is None else g_w2c.cpu()


def _fwd_norm(ref, rows):
    return ref.detach().reshape(rows, -1).double().norm(dim=1).clamp_min(1.0)


def _judge(pool, prefix, fails):
    """Pool.judge; a zero-cotangent row that is not exactly 0 (an assertion inside the gate) is recorded like a missed gate, so that
    the lines of the other quantities are still printed"""
    try:
        pool.judge(prefix, fails)
    except AssertionError as e:
        print(f"  {prefix}{e}  FAIL")
        fails.append(dict(what=f"{prefix}{e}"))


def _same(a, b_):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b_))


# ------------------------------------------------------------------------------------------------------------------ patch warp
@lru_cache(maxsize=None)
def patch_result(name):
    """one case through the kernels (twice) and through the restatement in both modes, computed once for all tests"""
    c = C.patch_case(name)
    b, n = c["b"], c["n"]
    o64, o32 = C.evaluate(c, F64), C.evaluate(c, F32)
    ex = C.exclusions(c, o64, o32)
    line = C.check_caps(c, ex)
    scale = torch.where(ex["rows"], torch.zeros_like(c["scale"]), c["scale"])          # left-out rows carry zero cotangents
    g = C.g_sampled_of(c, scale)
    dw = DevWarp(c)
    fwd, bwd = k_warp_forward(dw), k_warp_backward(dw, g, True)
    again = k_warp_forward(dw) + k_warp_backward(dw, g, True)
    no_pose = k_warp_backward(dw, g, False)
    g64, g32 = R.backward(o64.sampled, o64.leaves, g), R.backward(o32.sampled, o32.leaves, g)
    ker = R.pose_grads_kernel_order(o32.geo, (g * o32.sampled).sum(), n * c["patch"] ** 2)
    return dict(c=c, o64=o64, o32=o32, ex=ex, line=line, scale=scale, fwd=fwd, bwd=bwd, again=again, no_pose=no_pose, g64=g64, g32=g32,
                ker=ker)


def _patch_rows(name, pool, pose_pool, tag, problems=None):
    """the rows of one case into the pools; what must hold bit for bit goes to ``problems`` (checked by the caller AFTER the gates are
    printed: a wrong kernel then shows its gate lines as well) -> the case's exclusion line"""
    problems = [] if problems is None else problems
    r = patch_result(name)
    c, o64, o32, ex = r["c"], r["o64"], r["o32"], r["ex"]
    b, n = c["b"], c["n"]
    sampled, mask, gt_rgb, flat = r["fwd"]
    g_depth, g_pose, g_w2c = r["bwd"]
    def must(cond, what):
        if not cond:
            problems.append(f"{name}: {what}")

    for what, t in (("sampled", sampled), ("g_depth", g_depth), ("g_pose", g_pose), ("g_w2c", g_w2c)):
        must(bool(torch.isfinite(t).all()), f"{what} is not finite")
    must(torch.equal(gt_rgb, o64.gt_rgb), "gt_rgb is not the reference's bit for bit")
    # (a row whose variance is within the rounding bound of 0.01 takes no mask entry out: its entries are held to the float64
    #  comparisons on gx, gy, tz, the inside test and the flat bit that the kernel itself returned for the row)
    want = C.expected_mask(o64, ex, None if flat is None else flat != 0)
    must(bool(((mask != 0) == want)[~ex["mask"]].all()) and bool((mask <= 1).all()), "mask differs outside the exclusions")
    must(bool(((mask != 0) == want)[C.known_mask_entries(c, ex)].all()), "mask differs on a known-edge row")
    if flat is not None:
        must(bool(((flat != 0) == o64.flat)[~ex["flat"]].all()) and bool((flat <= 1).all()), "flat differs outside the exclusions")
        must(bool(((flat != 0) == o64.flat)[C.known_rows(c)].all()), "flat differs on a known-edge row")
    must(_same(r["fwd"] + r["bwd"], r["again"]), "a second run is not bit-identical")
    must(torch.equal(r["no_pose"][0], g_depth), "g_depth without the pose gradients differs from g_depth with them")
    must(bool((g_pose[:, 3] == 0).all()) and bool((g_w2c[:, 3] == 0).all()), "the bottom row of a pose gradient is not zero")
    if "near_plane" in c["known"]:
        must(bool((sampled[b - 1, 0, c["known"]["near_plane"]] == 0).all()), "the sample on the camera plane is not zero")
    rows = b * b * n
    pool.add(f"{tag}sampled", sampled.reshape(rows, -1), o64.sampled.reshape(rows, -1), o32.sampled.reshape(rows, -1),
             _fwd_norm(o64.sampled, rows))
    pool.add(f"{tag}g_depth", g_depth.reshape(b * n, 1), r["g64"][0].reshape(b * n, 1), r["g32"][0].reshape(b * n, 1),
             r["scale"].reshape(-1), ~ex["rows"].reshape(-1))
    ps, pt = C.pose_norms(r["scale"], torch.ones(b, b, dtype=torch.bool))
    pose_pool.add("g_pose", g_pose.reshape(b, 16), r["g64"][1].reshape(b, 16), r["g32"][1].reshape(b, 16), ps,
                  kernel_order=r["ker"][0].reshape(b, 16))
    pose_pool.add("g_w2c", g_w2c.reshape(b, 16), r["g64"][2].reshape(b, 16), r["g32"][2].reshape(b, 16), pt,
                  kernel_order=r["ker"][1].reshape(b, 16))
    return r["line"]


@pytest.mark.parametrize("name", [k for k in C.PATCH_CASES if k not in C.POOLED_PATCH])
def test_patch_warp_case_vs_float64(name, capsys):
    fails, problems, pool = [], [], Pool()
    line = _patch_rows(name, pool, Pool(), "", problems)         # (the per-image rows: test_pose_gradients_pooled_over_all_cases_vs_float64)
    with capsys.disabled():
        print(f"\n  patch warp {name}: {line}")
        _judge(pool, f"{name}: ", fails)
    assert not fails and not problems, [f["what"] for f in fails] + problems


def test_patch_warp_small_cases_pooled_vs_float64(capsys):
    """n = 1, b = 1 and the 2 x 2 image: rows gathered over the cases and judged once"""
    fails, problems, pool = [], [], Pool()
    lines = [(name, _patch_rows(name, pool, Pool(), "", problems)) for name in C.POOLED_PATCH]
    with capsys.disabled():
        for name, line in lines:
            print(f"\n  patch warp {name}: {line}", end="")
        print()
        _judge(pool, "small patch cases pooled: ", fails)
    assert not fails and not problems, [f["what"] for f in fails] + problems


# ------------------------------------------------------------------------------------------------------------------ flow
@lru_cache(maxsize=None)
def flow_result(name):
    c = C.flow_case(name)
    b, n = c["b"], c["n"]
    o64, o32 = C.evaluate_flow(c, F64), C.evaluate_flow(c, F32)
    g = C.g_flow_of(c, c["edges"])
    dw = DevWarp(c)
    ii, jj = dev(c["idii"], torch.int64), dev(c["idjj"], torch.int64)
    fwd, bwd = k_flow_forward(dw, ii, jj), k_flow_backward(dw, ii, jj, g, True)
    again = (k_flow_forward(dw, ii, jj),) + k_flow_backward(dw, ii, jj, g, True)
    no_pose = k_flow_backward(dw, ii, jj, g, False)
    g64, g32 = R.backward(o64.flow, o64.leaves, g), R.backward(o32.flow, o32.leaves, g)
    onehot = torch.zeros(len(c["edges"]), b, dtype=torch.bool)
    onehot[torch.arange(len(c["edges"])), c["idii"]] = True
    ker = R.pose_grads_kernel_order(o32.geo, (g * o32.flow).sum(), n, slot_source_mask=onehot, slot_target=c["idjj"])
    return dict(c=c, o64=o64, o32=o32, fwd=fwd, bwd=bwd, again=again, no_pose=no_pose, g64=g64, g32=g32, ker=ker)


def _flow_rows(name, pool, pose_pool, problems=None):
    problems = [] if problems is None else problems
    r = flow_result(name)
    c, o64, o32 = r["c"], r["o64"], r["o32"]
    b, n, ne = c["b"], c["n"], len(c["edges"])
    flow = r["fwd"]
    g_depth, g_pose, g_w2c = r["bwd"]
    def must(cond, what):
        if not cond:
            problems.append(f"flow {name}: {what}")

    for what, t in (("flow", flow), ("g_depth", g_depth), ("g_pose", g_pose), ("g_w2c", g_w2c)):
        must(bool(torch.isfinite(t).all()), f"{what} is not finite")
    must(_same((flow,) + r["bwd"], r["again"]), "a second run is not bit-identical")
    must(torch.equal(r["no_pose"][0], g_depth), "g_depth without the pose gradients differs from g_depth with them")
    has_edge = torch.zeros(b, dtype=torch.bool)
    has_edge[c["idii"]] = True
    must(bool((g_depth[~has_edge] == 0).all()) and bool((g_pose[~has_edge] == 0).all()), "a source without an edge has a gradient")
    must(bool((g_pose[:, 3] == 0).all()) and bool((g_w2c[:, 3] == 0).all()), "the bottom row of a pose gradient is not zero")
    feeds = torch.zeros(b, b, dtype=torch.bool)
    feeds[c["idjj"], c["idii"]] = True
    pool.add("flow", flow.reshape(ne * n, 2), o64.flow.reshape(ne * n, 2), o32.flow.reshape(ne * n, 2), _fwd_norm(o64.flow, ne * n))
    pool.add("g_depth", g_depth.reshape(b * n, 1), r["g64"][0].reshape(b * n, 1), r["g32"][0].reshape(b * n, 1),
             torch.where(has_edge[:, None], c["scale"], torch.zeros_like(c["scale"])).reshape(-1))
    ps, pt = C.pose_norms(c["scale"], feeds)
    ps = torch.where(has_edge, ps, torch.zeros_like(ps))
    pose_pool.add("g_pose", g_pose.reshape(b, 16), r["g64"][1].reshape(b, 16), r["g32"][1].reshape(b, 16), ps,
                  kernel_order=r["ker"][0].reshape(b, 16))
    pose_pool.add("g_w2c", g_w2c.reshape(b, 16), r["g64"][2].reshape(b, 16), r["g32"][2].reshape(b, 16), pt,
                  kernel_order=r["ker"][1].reshape(b, 16))


@pytest.mark.parametrize("name", [k for k in C.FLOW_CASES if k not in C.POOLED_FLOW])
def test_flow_case_vs_float64(name, capsys):
    fails, problems, pool = [], [], Pool()
    _flow_rows(name, pool, Pool(), problems)
    with capsys.disabled():
        print(f"\n  flow {name}:")
        _judge(pool, f"flow {name}: ", fails)
    assert not fails and not problems, [f["what"] for f in fails] + problems


def test_flow_small_cases_pooled_vs_float64(capsys):
    fails, problems, pool = [], [], Pool()
    for name in C.POOLED_FLOW:
        _flow_rows(name, pool, Pool(), problems)
    with capsys.disabled():
        print()
        _judge(pool, "small flow cases pooled: ", fails)
    assert not fails and not problems, [f["what"] for f in fails] + problems


def test_pose_gradients_pooled_over_all_cases_vs_float64(capsys):
    """the per-image quantities, judged once per pool: every patch-warp case; the flow cases in which every frame has an edge out and
    an edge in; the flow cases with a frame that has none (its gradient must be exactly 0, which the gate asserts)"""
    fails = []
    whole = lambda k: {a for a, _ in C.FLOW_CASES[k][2]} == {t for _, t in C.FLOW_CASES[k][2]} == set(range(C.FLOW_CASES[k][0]))
    with capsys.disabled():
        print()
        for kind, names, rows in (("patch warp, all cases pooled: ", list(C.PATCH_CASES), lambda k, p: _patch_rows(k, Pool(), p, "")),
                                  ("flow, cases with edges at every frame pooled: ", [k for k in C.FLOW_CASES if whole(k)],
                                   lambda k, p: _flow_rows(k, Pool(), p)),
                                  ("flow, cases with a frame without edges pooled: ", [k for k in C.FLOW_CASES if not whole(k)],
                                   lambda k, p: _flow_rows(k, Pool(), p))):
            pose = Pool()
            for name in names:
                rows(name, pose)
            _judge(pose, kind, fails)
    assert not fails, [f["what"] for f in fails]


def test_flow_without_edges_writes_nothing_forward_and_zeros_backward():
    from nicer_slam_amd._native import lib
    c = C.flow_case("b3 n255 special 5")
    dw = DevWarp(c)
    flow = nan(4)
    assert lib.nsa_flow_forward(dw.ref(), None, None, 0, ptr(flow), st()) == NSA_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(flow).all())
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    g_depth, g_pose, g_w2c = k_flow_backward(dw, none, none, torch.zeros(0, c["n"], 2), True)
    assert bool((g_depth == 0).all()) and bool((g_pose == 0).all()) and bool((g_w2c == 0).all())


# ------------------------------------------------------------------------------------------------------------------ masked L1
def k_masked_l1(pred, target, mask, ch, with_grad=True, misalign=False):
    from nicer_slam_amd._native import lib
    items = pred.shape[0]
    size = l1_workspace(items)
    assert int(lib.nsa_masked_l1_workspace(items)) == size, "nsa_masked_l1_workspace"
    ws = Guarded(size + 2)                                                   # (+ 2: room to hand over a pointer off by one float)
    p, t = dev(pred.reshape(-1)) if items else nan(4), dev(target.reshape(-1)) if items else nan(4)
    m = None if mask is None else dev(mask, torch.uint8)
    loss = nan(1)
    g = torch.full((max(items * ch, 1),), SENTINEL, device="cuda") if with_grad else None
    assert ws.t.data_ptr() % 8 == 0
    rc = lib.nsa_masked_l1(ptr(p), ptr(t), ptr(m) if (m is not None and items) else None, items, ch, ptr(loss), ptr(g),
                           ws.t.data_ptr() + (4 if misalign else 0), st())
    torch.cuda.synchronize()
    assert bool((ws.t[size + 2:] == SENTINEL).all()) and (misalign or bool((ws.t[size:] == SENTINEL).all())), "nsa_masked_l1 wrote past its workspace"
    return rc, loss.cpu()[0], None if g is None else g.cpu(), ws


@pytest.mark.parametrize("items", C.L1_ITEMS)
def test_masked_l1_loss_within_an_ulp_and_gradient_bit_for_bit(items, capsys):
    """the kernel forms |pred - target| in fp32 and sums in double: loss within 1 fp32 ulp of the float64 mean of the fp32-rounded
    differences; g_pred bit for bit sign(d) fl32(1 / (count ch)), 0 where masked or tied; grid-stride loop (items > 65 536) and the
    clamp of the block count (256) on both sides"""
    worst = 0.0
    for ch in C.L1_CH:
        for kind in C.L1_MASKS:
            pred, target, m = C.l1_case(items, ch, kind, 100 * ch + len(kind))
            rc, loss, g, _ws = k_masked_l1(pred, target, m, ch)
            assert rc == NSA_OK, (items, ch, kind)
            ref, g_ref = R.masked_l1(pred, target, m, ch)
            if items == 0 or m is not None and not bool(m.any()):          # (an empty selection, by design or by the draw at items = 1)
                assert bool(torch.isnan(loss)), (items, ch, kind)
                assert items == 0 or bool((g[:items * ch] == 0).all())
                if items == 0:
                    assert float(g[0]) == float(np.float32(SENTINEL))      # nothing launched for the gradient
                continue
            ulp = float(np.spacing(np.float32(float(ref))))
            assert abs(float(loss) - float(ref)) <= ulp, (items, ch, kind, float(loss), float(ref))
            worst = max(worst, abs(float(loss) - float(ref)) / ulp)
            assert torch.equal(g[:items * ch].reshape(items, ch), g_ref), (items, ch, kind)
            again = k_masked_l1(pred, target, m, ch)
            assert float(again[1]) == float(loss) and torch.equal(again[2], g)
    with capsys.disabled():
        print(f"\n  nsa_masked_l1 items = {items}: ch 1, 2, 3 x mask none / all / empty / random: loss off by at most {worst:.2f} fp32 ulp of "
              f"the float64 mean, g_pred bit for bit, NaN on an empty selection")


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_every_bad_argument_is_refused_without_a_launch():
    """every NSA_EBADARG branch of the five entry points, in the order warp_terms.hip tests them: one argument wrong at a time, all
    the others valid"""
    from nicer_slam_amd._native import lib, WarpDesc
    c = C.patch_case("b3 n65 48x33 p5")
    dw = DevWarp(c)
    b, n, patch = c["b"], c["n"], c["patch"]
    p2 = patch * patch
    out = dict(sampled=nan(b, b, n, p2, 3), gt_rgb=nan(b, b, n, p2, 3), g_depth=nan(b, n), g_pose=nan(b, 4, 4), g_w2c=nan(b, 4, 4),
               flow=nan(5, n, 2), loss=nan(1))
    mask = torch.full((b, b, n, p2), 0xCC, device="cuda", dtype=torch.uint8)
    flat = torch.full((b, n), 0xCC, device="cuda", dtype=torch.uint8)
    g = dev(C.g_sampled_of(c))
    ws = Guarded(patch_workspace(b, n, patch, True))
    t = dw.t

    def desc(**change):
        f = dict(b=b, n=n, H=c["H"], W=c["W"], **{k: t[k] for k in ("uv", "pose", "w2c", "K", "depth", "images", "depths", "frame_index")})
        f.update(change)
        return ctypes.byref(WarpDesc(f["b"], f["n"], f["H"], f["W"], *(ptr(f[k]) for k in ("uv", "pose", "w2c", "K", "depth", "images",
                                                                                          "depths", "frame_index"))))

    VALID = object()
    # what every entry point that takes the descriptor refuses (warp_ok): no descriptor, b = 0, n = 0, a missing uv, pose, w2c, K, depth
    bad_desc = [None, desc(b=0), desc(n=0)] + [desc(**{k: None}) for k in ("uv", "pose", "w2c", "K", "depth")]
    ii, jj = dev(torch.tensor([0, 1, 2, 0, 1]), torch.int64), dev(torch.tensor([1, 2, 0, 2, 0]), torch.int64)
    gf = dev(torch.ones(5, n, 2))
    gp, gw = ptr(out["g_pose"]), ptr(out["g_w2c"])

    def fwd(d=VALID, ps=patch, sampled=ptr(out["sampled"]), m=ptr(mask), gt=ptr(out["gt_rgb"]), fl=ptr(flat)):
        return lib.nsa_patch_warp_forward(desc() if d is VALID else d, ps, sampled, m, gt, fl, st())

    def bwd(d=VALID, ps=patch, gs=ptr(g), gd=ptr(out["g_depth"]), gp=gp, gw=gw, w=ws.ptr()):
        return lib.nsa_patch_warp_backward(desc() if d is VALID else d, ps, gs, gd, gp, gw, w, st())

    def ffwd(d=VALID, i=ptr(ii), j=ptr(jj), fl=ptr(out["flow"])):
        return lib.nsa_flow_forward(desc() if d is VALID else d, i, j, 5, fl, st())

    def fbwd(d=VALID, i=ptr(ii), j=ptr(jj), gfl=ptr(gf), gd=ptr(out["g_depth"]), gp=gp, gw=gw, w=ws.ptr()):
        return lib.nsa_flow_backward(desc() if d is VALID else d, i, j, 5, gfl, gd, gp, gw, w, st())

    rcs = {}
    for k, d in enumerate(bad_desc):
        for name, call in (("forward", fwd), ("backward", bwd), ("flow_forward", ffwd), ("flow_backward", fbwd)):
            rcs[f"{name}: descriptor {k}"] = call(d)
    # the patch warp: H < 2, W < 2, no images, patch 0, an even patch, a missing output; patch > 1 without the depth frames / flat
    for name, call in (("forward", fwd), ("backward", bwd)):
        rcs.update({f"{name}: H 1": call(desc(H=1)), f"{name}: W 1": call(desc(W=1)), f"{name}: no images": call(desc(images=None)),
                    f"{name}: patch 0": call(ps=0), f"{name}: patch 4": call(ps=4)})
    rcs.update({"forward: no sampled": fwd(sampled=None), "forward: no mask": fwd(m=None), "forward: no gt_rgb": fwd(gt=None),
                "forward: no depth frames": fwd(desc(depths=None)), "forward: no flat": fwd(fl=None),
                "backward: no g_sampled": bwd(gs=None), "backward: no g_depth": bwd(gd=None),
                "backward: g_pose alone": bwd(gw=None), "backward: g_w2c alone": bwd(gp=None),
                "backward: patch > 1 without a workspace": bwd(gp=None, gw=None, w=None),
                "backward: pose gradients without a workspace": bwd(ps=1, w=None)})
    # the flow (ne = 5): a missing index list, output or cotangent; one pose gradient alone; pose gradients without a workspace
    rcs.update({"flow_forward: no idii": ffwd(i=None), "flow_forward: no idjj": ffwd(j=None), "flow_forward: no flow": ffwd(fl=None),
                "flow_backward: no idii": fbwd(i=None), "flow_backward: no idjj": fbwd(j=None), "flow_backward: no g_flow": fbwd(gfl=None),
                "flow_backward: no g_depth": fbwd(gd=None), "flow_backward: g_pose alone": fbwd(gw=None),
                "flow_backward: g_w2c alone": fbwd(gp=None), "flow_backward: no workspace": fbwd(w=None)})
    # the masked L1: no loss, no workspace, no channels, items without pred / target, a workspace that is not 8-byte aligned
    pred, target, m = C.l1_case(257, 3, "random", 3)
    rc, loss, g1, l1ws = k_masked_l1(pred, target, m, 3, misalign=True)
    assert rc == NSA_EBADARG and bool(torch.isnan(loss)) and bool((g1 == SENTINEL).all()) and bool((l1ws.t == SENTINEL).all())
    assert ws.t.data_ptr() % 8 == 0
    l1 = lambda pr=ptr(g), ta=ptr(g), ch=3, lo=ptr(out["loss"]), w=ws.ptr(): lib.nsa_masked_l1(pr, ta, None, 10, ch, lo, None, w, st())
    rcs.update({"masked_l1: no loss": l1(lo=None), "masked_l1: no workspace": l1(w=None), "masked_l1: no channels": l1(ch=0),
                "masked_l1: no pred": l1(pr=None), "masked_l1: no target": l1(ta=None)})
    torch.cuda.synchronize()
    assert len(rcs) == 8 * 4 + 10 + 11 + 10 + 5
    wrong = [k for k, rc in rcs.items() if rc != NSA_EBADARG]
    assert not wrong, wrong
    # nothing was launched: every output still holds what it was filled with
    assert all(bool(torch.isnan(v).all()) for v in out.values())
    assert bool((mask == 0xCC).all()) and bool((flat == 0xCC).all()) and bool((ws.t == SENTINEL).all())
