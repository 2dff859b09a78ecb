"""The stand-alone hash-grid kernels (csrc/hash_encode.hip: k_grid_forward, k_grid_scatter, k_input_backward, k_grid_second_backward,
with csrc/grid_common.hpp's scatter_x_pair / scatter_span / gather paths under them) against float64 (tests/grid_ref64.py), per
(point, level) and per touched table row.  tests/test_hashenc_gpu.py judges the same outputs on the scale of a whole tensor, where an
error of 100 % of a faint row passes; here every error is divided by a quantity of the inputs of ITS unit:
  * value:                    per (point, level), by the largest |entry| of the cell's corner rows;
  * Jacobian:                 the same, times the level's scale;
  * J q (grad_grad):          the same, times the level's scale and the point's largest |q|;
  * J^T g:                    per point, by the point's cotangent scale c_p times the sum over the levels of scale x that largest |entry|
                              (the table rows span 2^-12 .. 2^12, so the Jacobian of a point does too);
  * table gradients (1st and 2nd order): per touched row, pooled per level and occupancy class (1, 2-8, 9-64, > 64 contributions; a
    class of fewer than POOL_MIN rows joins the next one), in TWO units, both gated:
      "contrib"  the sum over the row's contributions of their norms (float64).  A point on a cell border has t = 0 in fp32 and
                 t = +-1e-7 in float64 (u scale rounds once in fp32): its contributions to the far corners are 0 in any fp32
                 evaluation and 1e-14 |g| in float64 -- an error of 100 % of a contribution that is nothing.  Kernel and yardstick
                 share that (e_32 max = 1 in such pools), so in this unit alone those pools would pass anything;
      "cell"     the sum over the row's contributing points of what the point sends into its cell, |g[b, l]| (second order:
                 |g[b, l]| max|q_b| scale), whatever the corner's weight: e_32 is 1e-7 .. 1e-6 in every pool, and a row that is
                 wrong by a percent of its point's cotangent fails.
The gate is tests/gate64.py: rms(e_k) <= 1.5 rms(e_32) and max(e_k) <= 3 max(e_32), all finite, with
e_k = |kernel - float64| and e_32 = |C oracle - float64|; the table gradients have a second fp32 yardstick in the kernels' order of
summation and are gated against the larger of the two (gate64.gate with kernel_order; class Rows says why).  Rows no in-range point touches keep their prior content bit for bit, from a
zeroed buffer and from one pre-filled with a pattern (the ABI accumulates into it).  Without a reference: a permutation of the points
passes the same gate and leaves the untouched rows alone; cotangents times 2^k scale rows of occupancy 1 by exactly 2^k.
Which scatter path the inputs walk is counted by grid_ref64.paths and asserted in tests/test_grid_ref64_cpu.py.
The second half holds the table gradients of the fused mapping kernels (nsa_sdfnet_backward_params, nsa_colour_backward_params) to
tests/ref64.py with grid="exact" in the same units.  Measured figures and the mutants this file catches: DESIGN.md section 7."""
import numpy as np
import pytest
import torch

import grid_ref64 as G
from devcall import ptr, st
from gate64 import fwd_norm, gate
from gemm_cases import KINK, cot, scaled
from mlp_calls import Net, explicit, k_colour_forward, k_sdf_forward, one_per_ray, to_hl

pytestmark = pytest.mark.gpu

TINY, _spec = G.TINY, G.spec_of

BATCHES = (1, 63, 64, 65, 255, 256, 257, 4123)
POOL_MIN = 32
CLASSES = ((1, 1), (2, 8), (9, 64), (65, 1 << 62))


# ------------------------------------------------------------------------------------------------------------------ kernels
def k_suite(spec, emb, u, g, q, prefill=None, parts="all"):
    """the three entry points through hashencoder/backend.py; layouts of grid_ref64.  parts: all | table (no J^T g: calc_grad_inputs
    = 0) | inputs (no table: grad_embeddings = NULL, grad2_embeddings = NULL)"""
    from nicer_slam_amd.hashencoder.backend import _backend
    dev = "cuda"
    B, D, L, C = u.shape[0], 3, spec.num_levels, spec.level_dim
    S, H = float(np.log2(spec.per_level_scale)), spec.base_resolution
    ud, ed, off = u.to(dev), emb.to(dev), spec.offsets.to(dev)
    out = torch.full((L, B, C), float("nan"), device=dev)
    dy = torch.full((B, L * D * C), float("nan"), device=dev)
    _backend.hash_encode_forward(ud, ed, off, out, B, D, C, L, S, H, True, dy)
    gl = g.permute(1, 0, 2).contiguous().to(dev)
    fresh = lambda: torch.zeros_like(ed) if prefill is None else prefill.to(dev).clone()
    gt = fresh() if parts != "inputs" else None
    gu = torch.full((B, D), float("nan"), device=dev)
    _backend.hash_encode_backward(gl, ud, ed, off, gt, B, D, C, L, S, H, parts != "table", dy, gu)
    gg = torch.full((L, B, C), float("nan"), device=dev)
    g2 = fresh() if parts != "inputs" else None
    _backend.hash_encode_second_backward(gl, ud, ed, off, B, D, C, L, S, H, True, dy, q.to(dev).contiguous(), gg, g2)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()
    return dict(y=out.permute(1, 0, 2).cpu(), J=dy.view(B, L, D, C).cpu(), gu=gu.cpu(), gt=cpu(gt), gg=gg.permute(1, 0, 2).cpu(), g2=cpu(g2))


# ------------------------------------------------------------------------------------------------------------------ inputs + references
def inputs(spec, B, seed=0):
    u, emb = G.points(B, spec, seed), G.table(spec, seed)
    gen = torch.Generator().manual_seed(4000 + seed)
    c = G.point_scales(B, seed)
    g = (torch.randn(B, spec.num_levels, spec.level_dim, generator=gen).double() * c[:, None, None]).float()
    cq = G.point_scales(B, seed + 1)
    q = (torch.randn(B, 3, generator=gen).double() * cq[:, None]).float()
    return u, emb, g, q, c


class Case:
    """inputs, float64 reference, fp32 yardstick and the norms of one (geometry, B); built once per module and never changed"""

    def __init__(self, name, B):
        self.name, self.B = name, B
        self.spec = spec = _spec(name)
        self.u, self.emb, self.g, self.q, self.c = inputs(spec, B)
        self.plan = plan = G.Plan(self.u, spec)
        u64, e64, g64, q64 = self.u.double(), self.emb.double(), self.g.double(), self.q.double()
        y, J = G.encode(plan, u64, e64)
        gu, gt, n1 = G.backward(plan, u64, g64, J, with_norms=True)
        gg, g2, n2 = G.second_backward(plan, u64, g64, J, q64, with_norms=True)
        self.ref = dict(y=y, J=J, gu=gu, gt=gt, gg=gg, g2=g2)
        self.row_norm, self.row_count = dict(gt=n1[0], g2=n2[0]), n1[1]
        self.row_unit = dict(gt=n1[2], g2=n2[2])
        self.y32 = G.oracle_suite(spec, self.emb, self.u, self.g, self.q)
        self.yker = dict(gt=G.kernel_order_scatter(plan, G.kernel_order_contribs(plan, self.u, self.g)),
                         g2=G.kernel_order_scatter(plan, G.kernel_order_contribs(plan, self.u, self.g, self.q)))
        L = spec.num_levels
        rowmax = torch.stack([e64[plan.rows[l]].abs().amax(dim=(1, 2)) for l in range(L)], dim=1)          # [B, L]
        rowmax = torch.where(plan.inside[:, None], rowmax, torch.zeros_like(rowmax))
        scale = torch.tensor([float(v.scale) for v in plan.lv], dtype=G.F64)
        self.cell_norm = dict(y=rowmax.reshape(-1), J=(rowmax * scale).reshape(-1),
                              gg=(rowmax * scale * q64.abs().amax(dim=1, keepdim=True)).reshape(-1))
        self.point_norm = self.c * (rowmax * scale).sum(dim=1)
        self.touched = self.row_count > 0

    def pools(self):
        """[(label, row indices)]: every touched row in exactly one.  Per level the occupancy classes, each at least POOL_MIN rows
        (smaller ones join the next class, the last one the previous pool; what a whole level cannot fill goes to one pool over all
        levels).  The tiny tables have 2 .. 32 rows a level: their classes run over all levels, and `Rows` pools them over all the
        tiny geometries and batch sizes of a test."""
        if self.name in TINY:
            cls = [(f"occupancy {lo}-{hi if hi < 1 << 62 else ''}", torch.nonzero((self.row_count >= lo) & (self.row_count <= hi)).reshape(-1))
                   for lo, hi in CLASSES]
            return [(a, b) for a, b in cls if b.numel()]
        return level_pools(self.plan.lv, self.row_count)


def level_pools(lvs, count):
    """[(label, rows)]: per level the occupancy classes, each at least POOL_MIN rows (smaller ones join the next class, the last one
    the previous pool; what a whole level cannot fill goes to one pool over all levels)"""
    out, rest = [], []
    for l, lv in enumerate(lvs):
        cnt = count[lv.row0:lv.row0 + lv.rows]
        mine, held = [], torch.zeros(0, dtype=torch.int64)
        for lo, hi in CLASSES:
            rows = torch.cat([held, torch.nonzero((cnt >= lo) & (cnt <= hi)).reshape(-1) + lv.row0])
            if rows.numel() >= POOL_MIN:
                mine.append([f"level {l} occupancy {lo}-{hi if hi < 1 << 62 else ''}", rows])
                held = rows[:0]
            else:
                held = rows
        if held.numel():
            if mine:
                mine[-1][1] = torch.cat([mine[-1][1], held])
            else:
                rest.append(held)
        out += mine
    if rest:
        out.append(["levels with too few rows", torch.cat(rest)])
    return [(a, b) for a, b in out]


def merged_classes(count):
    """[(label, rows)] over a whole table: the occupancy classes, one of fewer than POOL_MIN rows joined to the next (the last: to the
    previous)"""
    out, held, lo0 = [], torch.zeros(0, dtype=torch.int64), None
    for lo, hi in CLASSES:
        idx = torch.cat([held, torch.nonzero((count >= lo) & (count <= hi)).reshape(-1)])
        lo0 = lo if lo0 is None else lo0
        if idx.numel() >= POOL_MIN:
            out.append([f"occupancy {lo0}-{hi if hi < 1 << 62 else ''}", idx])
            held, lo0 = idx[:0], None
        else:
            held = idx
    if held.numel():
        if out:
            out[-1][1] = torch.cat([out[-1][1], held])
        else:
            out.append(["all rows", held])
    return [(a, b) for a, b in out]


class Rows:
    """table rows gathered under a label over several cases (padded to a common width with zeros on all sides), judged once, against
    the larger of two fp32 yardsticks: the C oracle (point after point, every operation rounded on its own) and the kernels' order --
    grid_ref64.kernel_order_scatter (the run merge, wave after wave) on grid_ref64.kernel_order_contribs (the complements 1 - w as
    ONE fused multiply-add, which is what the compiler makes of the kernels' `1.0f - w[d]`: traced on MI355X at a point with
    t = 0.9999981 on a level of the colour grid, where the unfused form gives a weight of exactly 0, the fused one 1.4e-11 and float64
    3.0e-12 -- 100 % and 372 % of a contribution that is nothing on the scale of its point's cotangent).  Neither is the order in which the atomics of different waves reach a row -- that is the hardware's and
    changes from run to run; on a row with thousands of contributions of 2^-30 .. 2^30 the three orders differ like three draws."""

    def __init__(self):
        self.items = {}

    def add(self, label, *tensors):
        self.items.setdefault(label, []).append([t.reshape(t.shape[0], -1).double() for t in tensors])

    def judge(self, fails):
        for label, items in self.items.items():
            width = max(i[0].shape[1] for i in items)
            got, ref, y32, yker = (torch.cat([torch.nn.functional.pad(i[k], (0, width - i[k].shape[1])) for i in items]) for k in range(4))
            norm = torch.cat([i[4].reshape(-1) for i in items])
            gate(label, got, ref, y32, norm, failures=fails, kernel_order=yker)


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(name, B):
        if (name, B) not in memo:
            memo[(name, B)] = Case(name, B)
        return memo[(name, B)]
    return get


def names_of(group):
    return list(TINY) if group == "tiny" else [group]


def check(case, got, tag, fails, rows, table_only=False):
    c = case
    L, B = c.spec.num_levels, c.B
    flat = lambda t: t.reshape(B * L, -1)
    if not table_only:
        for k in ("y", "J", "gg"):
            gate(f"{tag}: {k} per (point, level)", flat(got[k]), flat(c.ref[k]), flat(c.y32[k]), c.cell_norm[k], failures=fails)
        gate(f"{tag}: J^T g per point", got["gu"], c.ref["gu"], c.y32["gu"], c.point_norm.clone(), failures=fails)
    seen = 0
    for k in ("gt", "g2"):
        for label, idx in c.pools():
            seen += idx.numel()
            for unit, norm in (("contrib", c.row_norm), ("cell", c.row_unit)):
                where = tag.replace(c.name, "tiny tables").split(" B ")[0] if c.name in TINY else tag
                rows.add(f"{where}: {k} {label} / {unit}", got[k][idx], c.ref[k][idx], c.y32[k][idx], c.yker[k][idx], norm[k][idx])
        assert bool((got[k][~c.touched] == 0).all()), f"{tag}: {k} wrote a row that no in-range point touches"
    assert seen == 2 * int(c.touched.sum()), "a touched row is in no pool or in two"


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("group", ["coarse", "fine", "colour_small", "tiny"])
def test_operator_vs_float64_row_by_row(group, cases, capsys):
    fails, rows = [], Rows()
    with capsys.disabled():
        print()
        for name in names_of(group):
            for B in BATCHES:
                c = cases(name, B)
                got = k_suite(c.spec, c.emb, c.u, c.g, c.q)
                check(c, got, f"{name} B {B}", fails, rows)
                out = ~c.plan.inside
                if bool(out.any()):
                    for k in ("y", "J", "gg", "gu"):
                        assert float(got[k][out].abs().max()) == 0, f"{name} B {B}: {k} of an out-of-range point is not exactly zero"
        rows.judge(fails)
    assert not fails, [f["what"] for f in fails]


@pytest.mark.parametrize("group", ["coarse", "fine", "colour_small", "tiny"])
def test_untouched_rows_prefilled_and_each_output_alone(group, cases, capsys):
    fails, rows = [], Rows()
    for name in names_of(group):
        _prefilled_and_alone(cases(name, 4123), fails, rows)
    with capsys.disabled():
        print()
        rows.judge(fails)
    assert not fails, [f["what"] for f in fails]


def _prefilled_and_alone(c, fails, rows):
    name = c.name
    gen = torch.Generator().manual_seed(9)
    pre = (torch.randint(1, 1 << 20, c.emb.shape, generator=gen).float() * 2.0 ** -10) * torch.where(torch.rand(c.emb.shape, generator=gen) < 0.5, -1.0, 1.0)
    got = k_suite(c.spec, c.emb, c.u, c.g, c.q, prefill=pre)
    zero = k_suite(c.spec, c.emb, c.u, c.g, c.q)
    n_add = c.row_count.double()[:, None]
    for k in ("gt", "g2"):
        assert torch.equal(got[k][~c.touched], pre[~c.touched]), f"{k}: a row that no in-range point touches changed"
        # touched rows: the prior content plus the same sum, added in some order: each of the n additions rounds at most 2^-24 of the
        # magnitude the row can reach, |prior| + sum of |contributions|; the zero-filled run carries the same bound without the prior
        bound = (2 * n_add + 2) * 2.0 ** -24 * (pre.abs().double() + c.row_norm[k][:, None])
        err = (got[k].double() - pre.double() - zero[k].double()).abs()
        assert bool((err <= bound)[c.touched].all()), f"{k}: accumulation into a pre-filled row, worst {float((err / bound.clamp_min(1e-300))[c.touched].max()):.3g} of the bound"
    tab = k_suite(c.spec, c.emb, c.u, c.g, c.q, parts="table")
    inp = k_suite(c.spec, c.emb, c.u, c.g, c.q, parts="inputs")
    check(c, tab, f"{name} table alone", fails, rows, table_only=True)
    for k in ("y", "J", "gg", "gu"):
        assert torch.equal(inp[k], zero[k]), f"{k} changes when the table gradients are not asked for"
    for k in ("y", "J", "gg"):
        assert torch.equal(tab[k], zero[k]), f"{k} changes when J^T g is not asked for"


@pytest.mark.parametrize("group", ["coarse", "fine", "colour_small", "tiny"])
def test_permutation_and_power_of_two_scaling(group, cases, capsys):
    """(on the tiny tables no row has a single contribution at B = 4123: there the scaling check covers J^T g only)"""
    fails, rows = [], Rows()
    for name in names_of(group):
        _permuted_and_scaled(cases(name, 4123), fails, rows)
    with capsys.disabled():
        print()
        rows.judge(fails)
    assert not fails, [f["what"] for f in fails]


def _permuted_and_scaled(c, fails, rows):
    name = c.name
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(11))
    inv = torch.argsort(perm)
    got = k_suite(c.spec, c.emb, c.u[perm].contiguous(), c.g[perm].contiguous(), c.q[perm].contiguous())
    for k in ("y", "J", "gg", "gu"):
        got[k] = got[k][inv]
    base = k_suite(c.spec, c.emb, c.u, c.g, c.q)
    for k in ("y", "J", "gg", "gu"):
        assert torch.equal(got[k], base[k]), f"{k} of a point depends on its place in the batch"
    check(c, got, f"{name} permuted", fails, rows, table_only=True)
    once = c.row_count == 1
    assert int(once.sum()) > 0 or name.startswith("tiny")
    for k2 in (3, -20, 40):                       # 2^30 |g| 2^40 and the sums over it stay far below 2^127, 2^-30 |g| 2^-20 w far above 2^-126
        f = 2.0 ** k2
        scaled = k_suite(c.spec, c.emb, c.u, c.g * f, c.q)
        for k in ("gt", "g2"):
            assert torch.equal(scaled[k][once], base[k][once] * f), f"{k}: cotangents x 2^{k2} do not scale a row of one contribution by exactly 2^{k2}"
        assert torch.equal(scaled["gu"], base["gu"] * f)


def test_shipped_colour_geometry_sparse_scatter(capsys):
    """The shipped colour grid (16 x 2, 16 -> 2048, 2^24 rows a level, 1 GiB; the uint32 stride wrap at resolution 2048) at B = 4123:
    value, Jacobian, J q, J^T g and both table scatters.  The references hold the touched rows only (grid_ref64.compact); the fp32
    yardstick is grid_ref64's fp32 mode (bit for bit the C oracle's value and Jacobian, the oracle's order of summation), since the
    oracle's own dense tables do not fit a test.  The untouched rows are checked on the device: from a zeroed buffer and from a
    pre-filled one the touched rows are overwritten and the rest compared."""
    from nicer_slam_amd.hashencoder.backend import _backend
    from oracle import render_ref as R
    dev = "cuda"
    spec = R.make_grid_spec(16, 2, 16, 2048, 24)
    B, D, L, C = 4123, 3, 16, 2
    S, H = float(np.log2(spec.per_level_scale)), spec.base_resolution
    u = G.points(B, spec)
    plan = G.Plan(u, spec)
    uniq, small = G.compact(plan)
    K = uniq.numel()
    gen = torch.Generator().manual_seed(41)
    vals = (torch.randn(K, C, generator=gen) * torch.exp2(torch.rand(K, 1, generator=gen) * 24 - 12)).contiguous()
    c, cq = G.point_scales(B, 3), G.point_scales(B, 4)
    g = (torch.randn(B, L, C, generator=gen).double() * c[:, None, None]).float()
    q = (torch.randn(B, 3, generator=gen).double() * cq[:, None]).float()
    res = {}
    for dt in (G.F64, torch.float32):
        ud, ed, gd, qd = u.to(dt), vals.to(dt), g.to(dt), q.to(dt)
        y, J = G.encode(small, ud, ed)
        gu, gt, n1 = G.backward(small, ud, gd, J, n_rows=K, with_norms=True)
        gg, g2, n2 = G.second_backward(small, ud, gd, J, qd, n_rows=K, with_norms=True)
        res[dt] = dict(y=y, J=J, gu=gu, gt=gt, gg=gg, g2=g2, n=(n1, n2))
    ref, y32 = res[G.F64], res[torch.float32]
    n1, n2 = ref["n"]
    rowmax = torch.stack([vals.double()[small.rows[l]].abs().amax(dim=(1, 2)) for l in range(L)], dim=1)
    rowmax = torch.where(plan.inside[:, None], rowmax, torch.zeros_like(rowmax))
    scale = torch.tensor([float(v.scale) for v in plan.lv], dtype=G.F64)
    norm = dict(y=rowmax.reshape(-1), J=(rowmax * scale).reshape(-1), gg=(rowmax * scale * q.double().abs().amax(dim=1, keepdim=True)).reshape(-1))
    uniq_d = uniq.to(dev)

    def run(fill):
        emb = torch.zeros(spec.n_rows, C, device=dev)
        emb[uniq_d] = vals.to(dev)
        ud, off = u.to(dev), spec.offsets.to(dev)
        out, dy = torch.full((L, B, C), float("nan"), device=dev), torch.full((B, L * D * C), float("nan"), device=dev)
        _backend.hash_encode_forward(ud, emb, off, out, B, D, C, L, S, H, True, dy)
        gl = g.permute(1, 0, 2).contiguous().to(dev)
        gt, gu = torch.full((spec.n_rows, C), fill, device=dev), torch.full((B, D), float("nan"), device=dev)
        _backend.hash_encode_backward(gl, ud, emb, off, gt, B, D, C, L, S, H, True, dy, gu)
        g2, gg = torch.full((spec.n_rows, C), fill, device=dev), torch.full((L, B, C), float("nan"), device=dev)
        _backend.hash_encode_second_backward(gl, ud, emb, off, B, D, C, L, S, H, True, dy, q.to(dev).contiguous(), gg, g2)
        torch.cuda.synchronize()
        got = dict(y=out.permute(1, 0, 2).cpu(), J=dy.view(B, L, D, C).cpu(), gu=gu.cpu(), gg=gg.permute(1, 0, 2).cpu())
        for k, t in (("gt", gt), ("g2", g2)):
            got[k] = t[uniq_d].cpu() - fill
            t[uniq_d] = fill                                      # overwrite the touched rows: the whole table is the fill again
            assert bool((t == fill).all()), f"{k}: a row that no in-range point touches changed (buffer filled with {fill})"
        return got
    got = run(0.0)
    fails, rows = [], Rows()
    with capsys.disabled():
        print()
        flat = lambda t: t.reshape(B * L, -1)
        for k in ("y", "J", "gg"):
            gate(f"shipped colour grid: {k} per (point, level)", flat(got[k]), flat(ref[k]), flat(y32[k]), norm[k], failures=fails)
        gate("shipped colour grid: J^T g per point", got["gu"], ref["gu"], y32["gu"], c * (rowmax * scale).sum(dim=1), failures=fails)
        pos = lambda r: int(torch.searchsorted(uniq, torch.tensor(r)))
        lvs = [v._replace(row0=pos(v.row0), rows=pos(v.row0 + v.rows) - pos(v.row0)) for v in plan.lv]     # the levels' slices of the compact rows
        for k, n in (("gt", n1), ("g2", n2)):
            seen = 0
            for label, idx in level_pools(lvs, n[1]):
                seen += idx.numel()
                for unit, nm in (("contrib", n[0]), ("cell", n[2])):
                    rows.add(f"shipped colour grid: {k} {label} / {unit}", got[k][idx], ref[k][idx], y32[k][idx], y32[k][idx], nm[idx])
            assert seen == K
        rows.judge(fails)
    assert not fails, [f["what"] for f in fails]
    run(0.375)            # (pre-filled: only the untouched rows are judged; the touched ones carry the fill's rounding)


# ------------------------------------------------------------------------------------------------------------------ fused SDF sites
# nsa_sdfnet_backward_params' g_table (csrc/sdf_net.hpp::table_grad_scatter, csrc/sdf_net4.hpp::table_grad_scatter4): per corner row
# ONE value  w_corner hb + k_corner dl  -- the value path plus the table's share of the double backward through grad sdf.  float64 and
# the fp32 yardstick are tests/ref64.py with grid="exact" (sdf_table_grad), on the golden model with perturbed weights
# (mlp_calls.Net).  Its grids are small (4 levels of 64 rows, 8 levels up to 32^3 capped at 2^10), so thousands of
# contributions meet in a row: the classes are pooled over the levels, and the second yardstick is the same fp32 rows summed by the
# run merge of 64 consecutive points (a valid order, not these kernels' exact one: they tile 16 / 32 points).
def k_sdf_table(net, which, tile, x, g_sdf, g_feat, g_grad, prefill=None):
    import ctypes
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import mapping
    P = x.shape[0]
    xd = x.cuda().contiguous()
    gd, _keep, pk = net.sdf(which, tile)
    emb = getattr(net.model.implicit_network, which).encoding.embeddings
    gs = g_sdf.cuda().contiguous() if g_sdf is not None else None
    gf = to_hl(g_feat) if g_feat is not None else None
    gg = g_grad.cuda().contiguous() if g_grad is not None else None
    g_x = torch.zeros(P, 3, device="cuda")
    g_table = torch.zeros_like(emb) if prefill is None else prefill.cuda().clone()
    emit = torch.full((lib.nsa_sdfnet_emit_rows_tile(gd.n_hidden, tile), mapping.emit_ld(P)), float("nan"), device="cuda")
    pts = explicit(xd)
    check(lib.nsa_sdfnet_backward_params(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), ptr(gs), ptr(gf), ptr(gg), 0,
                                         g_x.data_ptr(), g_table.data_ptr(), emit.data_ptr(), emit.shape[1], st()))
    torch.cuda.synchronize()
    return g_x.cpu(), g_table.cpu()


def shipped_geometry(fx, g):
    """Net(edit=...): the golden model with the SHIPPED grid geometries -- coarse 4 x 8 at 32 -> 32, fine 8 x 4 at 32 -> 128 (2^19 rows:
    four dense non-power-of-two LV_SUBONCE levels, three hashed ones), colour at `colour_small` (16 x 2 at 16 -> 512, 2^19) -- and
    tables of rand(-1, 1) x 0.05 (colour 0.5) x a per-row factor 2^U(-8, 0).  The MLP shapes do not change."""
    from oracle import render_ref as R
    for key, meta, geo, amp in (("implicit_network.coarse", "meta_coarse_grid", (4, 8, 32, 32, 19), 0.05),
                                ("implicit_network.fine", "meta_fine_grid", (8, 4, 32, 128, 19), 0.05),
                                ("rendering_network", "meta_colour_grid", (16, 2, 16, 512, 19), 0.5)):
        L, C, base, end, logmap = geo
        spec = R.make_grid_spec(L, C, base, end, logmap)
        fx[meta] = np.array([base, end, logmap] + ([L, C] if "colour" not in meta else []), dtype=np.int64)
        row = torch.exp2(-8.0 * torch.rand(spec.n_rows, 1, generator=g))
        fx[f"param_{key}.encoding.embeddings"] = ((torch.rand(spec.n_rows, C, generator=g) * 2 - 1) * amp * row).numpy()
        fx[f"param_{key}.encoding.offsets"] = spec.offsets.numpy()


@pytest.fixture(scope="module", params=["golden", "shipped"])
def net(request):
    n = Net(edit=shipped_geometry if request.param == "shipped" else None)
    n.geometry = request.param
    return n


def table_pools(net, plan, count):
    """the shipped geometries have rows of every occupancy on every level: classes per level.  The golden model's grids are small (4
    levels of 64 rows; 8 and 16 levels capped at 2^10 rows): per level a class holds a few dozen rows at most, each fed by one or two
    draws of the MLP's own error -- measured per level on MI355X: colour level 5, occupancy 1, 37 rows, e_k 1.58e-7 against e_32
    9.4e-8 rms (ratio 1.69), where the same class over the whole table (80 rows) stands at 1.17.  So there the classes run over the
    whole table."""
    return level_pools(plan.lv, count) if net.geometry == "shipped" else merged_classes(count)


def spread_copies(x, divide_factor):
    """grid_ref64.points repeats single points (257, 65 and 50 copies).  In the stand-alone operator a copy adds the same fp32 row again,
    but behind an MLP a copy is the MLP's SAME rounding error again: rows fed by 255 copies would be judged on one draw (measured:
    the four worst rows of a pool of 96, e_k 3.2e-5 against e_32 1.0e-5, all fed by the 257 copies).  So the copies step along x by
    2^-21 in unit coordinates: 257 steps are 1/60 of the finest cell, the rows and the runs stay, the draws differ."""
    x = x.clone()
    for lo, hi in ((0, 257), (300, 365), (2401, 2501)):
        x[lo:hi, 0] += torch.arange(hi - lo, dtype=torch.float32) * (2.0 ** -20 * divide_factor)
    return x.contiguous()


def _sdf_case(net, which, fam):
    import ref64
    spec = getattr(net.cfg, which)
    P = 4123
    x = spread_copies((G.points(P, spec.grid) * 2.0 - 1.0) * spec.divide_factor, spec.divide_factor)
    c = G.point_scales(P, 7)
    gs = scaled(cot(P, 21, ()), c) if fam in ("all", "sdf") else None
    gf = scaled(cot(P, 22, (64,)), c) if fam in ("all", "feat") else None
    gg = scaled(cot(P, 23, (3,)), c) if fam in ("all", "grad") else None
    r_x, r_t, plan = ref64.sdf_table_grad(net.params, net.cfg, x, which, gs, gf, gg)
    y_x, y_t, plan32 = ref64.sdf_table_grad(net.params, net.cfg, x, which, gs, gf, gg, dtype=torch.float32)
    # every row's contributions, float64 (norms) and fp32 (the second order of summation)
    u = (x.double() / spec.divide_factor + 1) / 2

    def rows_of(plan, u):
        value = [r[1] for r in plan.record if r[0] == "first"][-1]
        second = [r for r in plan.record if r[0] == "second"]
        con = G.kernel_order_contribs(plan, u, value)
        unit = [value[:, l].double().norm(dim=1) for l in range(plan.L)]
        for _tag, dl, q in second:
            extra = G.kernel_order_contribs(plan, u, dl, q)
            con = [a + b for a, b in zip(con, extra)]
            unit = [a + dl[:, l].double().norm(dim=1) * q.double().abs().amax(dim=1) * float(plan.lv[l].scale) for l, a in enumerate(unit)]
        return con, unit
    con, unit = rows_of(plan, u)
    table, norms = G.scatter_contribs(plan, con, unit)
    assert float((table - r_t).abs().max()) <= 1e-12 * float(r_t.abs().max()), "the recorded contributions do not add up to the table gradient"
    con32, _unit = rows_of(plan32, u.float())
    y_ker = G.kernel_order_scatter(plan32, con32)
    return dict(x=x, c=c, g=(gs, gf, gg), ref=(r_x, r_t), y32=(y_x, y_t), y_ker=y_ker, norms=norms, plan=plan)


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_fused_sdf_table_gradient_row_by_row(net, which, capsys):
    fails, rows = [], Rows()
    with capsys.disabled():
        print()
        for fam in ("all", "sdf", "feat", "grad"):
            cs = _sdf_case(net, which, fam)
            count = cs["norms"][1]
            touched = count > 0
            for tile in (16, 32):
                g_x, g_t = k_sdf_table(net, which, tile, cs["x"], *cs["g"])
                tag = f"sdfnet_backward_params {net.geometry} {which} t{tile} {fam}"
                gate(f"{tag}: d/dx per point", g_x, cs["ref"][0], cs["y32"][0], cs["c"].clone(), failures=fails)
                assert bool((g_t[~touched] == 0).all()), f"{tag}: g_table wrote a row that no in-range point touches"
                for label, idx in table_pools(net, cs["plan"], count):
                    for unit, norm in (("contrib", cs["norms"][0]), ("cell", cs["norms"][2])):
                        rows.add(f"{tag}: g_table {label} / {unit}", g_t[idx], cs["ref"][1][idx], cs["y32"][1][idx], cs["y_ker"][idx], norm[idx])
                if fam == "all":
                    pre = torch.full_like(g_t, 0.375)
                    _gx, g_p = k_sdf_table(net, which, tile, cs["x"], *cs["g"], prefill=pre)
                    assert torch.equal(g_p[~touched], pre[~touched]), f"{tag}: a pre-filled row that no in-range point touches changed"
        rows.judge(fails)
    assert not fails, [f["what"] for f in fails]


# ------------------------------------------------------------------------------------------------------------------ fused colour site
# nsa_colour_backward_params' g_table (csrc/colour_bwd_body.inc): the value path alone -- the colour network has no double backward.
# Points within KINK of a ReLU kink may take the other branch in fp32 (as in tests/test_gemm_float64_gpu.py): the rows they touch
# are left out of the gate and only have to be finite.
def k_colour_table(net, x, d, normals, feat, g_rgb, grid_grad, prefill=None):
    import ctypes
    from nicer_slam_amd._native import lib, check
    from nicer_slam_amd.fused import mapping
    P = x.shape[0]
    _rgb, (o, dd, _z, grad, fh, save) = k_colour_forward(net, x, d, normals, feat)
    pts, _keep_z = one_per_ray(o, dd)
    gd, _keep, pk = net.colour()
    emb = net.model.rendering_network.encoding.embeddings
    gr = g_rgb.cuda().contiguous()
    g_feat = torch.full((((P + 31) // 32) * 2048,), float("nan"), device="cuda")
    g_grad, g_x, g_dir = (torch.zeros(P, 3, device="cuda") for _ in range(3))
    g_table = torch.zeros_like(emb) if prefill is None else prefill.cuda().clone()
    emit = torch.full((lib.nsa_colour_emit_rows(), mapping.emit_ld(P)), float("nan"), device="cuda")
    check(lib.nsa_colour_backward_params(ctypes.byref(pts), ctypes.byref(gd), pk.data_ptr(), grad.data_ptr(), fh.data_ptr(),
                                         save.data_ptr(), gr.data_ptr(), grid_grad, g_feat.data_ptr(), g_grad.data_ptr(),
                                         g_x.data_ptr(), g_dir.data_ptr(), g_table.data_ptr(), emit.data_ptr(), emit.shape[1], st()))
    torch.cuda.synchronize()
    return g_x.cpu(), g_table.cpu()


def test_fused_colour_table_gradient_row_by_row(net, capsys):
    import ref64
    from oracle import render_ref as R
    cfg = net.cfg
    P = 4123
    x = spread_copies((G.points(P, cfg.colour_grid) * 2.0 - 1.0) * cfg.colour_divide_factor, cfg.colour_divide_factor)
    gen = torch.Generator().manual_seed(31)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1).contiguous()
    normals, feat = torch.randn(P, 3, generator=gen), torch.randn(P, 64, generator=gen) * 0.3
    c = G.point_scales(P, 9)
    g_rgb = scaled(cot(P, 32, (3,)), c)
    keep = R.colour_relu_margin(net.params, cfg, x, normals, d, feat) >= KINK
    assert int((~keep).sum()) <= P // 50, int((~keep).sum())
    ref, r_t, plan = ref64.colour_table_grad(net.params, cfg, x, normals, d, feat, g_rgb)
    y32, y_t, plan32 = ref64.colour_table_grad(net.params, cfg, x, normals, d, feat, g_rgb, dtype=torch.float32)
    u = (x.double() / cfg.colour_divide_factor + 1) / 2
    value = plan.record[-1][1]
    assert [r[0] for r in plan.record] == ["first"]
    table, norms = G.scatter_contribs(plan, G.kernel_order_contribs(plan, u, value), [value[:, l].norm(dim=1) for l in range(plan.L)])
    assert float((table - r_t).abs().max()) <= 1e-12 * float(r_t.abs().max())
    y_ker = G.kernel_order_scatter(plan32, G.kernel_order_contribs(plan32, u.float(), plan32.record[-1][1]))
    count = norms[1]
    touched = count > 0
    near_kink = torch.zeros_like(touched)
    for l in range(plan.L):
        near_kink[plan.rows[l][~keep & plan.inside].reshape(-1)] = True
    fails, rows = [], Rows()
    with capsys.disabled():
        print(f"\n  colour: {int((~keep).sum())} of {P} points within {KINK} of a ReLU kink; the {int(near_kink.sum())} rows they touch are left out")
        g_x, g_t = k_colour_table(net, x, d, normals, feat, g_rgb, 1)
        gate(f"colour_backward_params {net.geometry} grid_grad 1: d/dx per point", g_x, ref["x"], y32["x"], c.clone(), keep, failures=fails)
        assert bool(torch.isfinite(g_t).all()) and bool((g_t[~touched] == 0).all()), "g_table wrote a row that no in-range point touches"
        judged = count.clone()
        judged[near_kink] = 0
        for label, idx in table_pools(net, plan, judged):
            for unit, norm in (("contrib", norms[0]), ("cell", norms[2])):
                rows.add(f"colour_backward_params {net.geometry}: g_table {label} / {unit}", g_t[idx], r_t[idx], y_t[idx], y_ker[idx], norm[idx])
        rows.judge(fails)
    assert not fails, [f["what"] for f in fails]
    pre = torch.full_like(g_t, -0.625)
    _gx, g_p = k_colour_table(net, x, d, normals, feat, g_rgb, 1, prefill=pre)
    assert torch.equal(g_p[~touched], pre[~touched]), "a pre-filled row that no in-range point touches changed"
    _gx, g_0 = k_colour_table(net, x, d, normals, feat, g_rgb, 0, prefill=pre)
    assert torch.equal(g_0, pre), "grid_grad = 0 touches the colour table gradient"


# ------------------------------------------------------------------------------------------------------------------ fused forwards
# Value and Jacobian of the grids inside nsa_sdfnet_forward (the gather paths of the fused callers): sdf, grad sdf and feature against
# tests/ref64.py with grid="exact", per point, with the gate and the norm of tests/test_gemm_float64_gpu.py.  The points are
# grid_ref64.points: u = 0 and u = 1 faces (the dense index wrap at (1, 1, 1), the upper face of the dense non-power-of-two levels),
# interior cell borders, out-of-range points (zero grid features), runs.
@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_fused_sdf_forward_through_the_exact_grid(net, which, capsys):
    import ref64
    spec = getattr(net.cfg, which)
    x = (G.points(4123, spec.grid) * 2.0 - 1.0) * spec.divide_factor
    k = torch.arange(2600, 2664)
    x[k, k % 3] = spec.divide_factor                               # 64 uniform points moved onto a u = 1 face
    x = x.contiguous()
    plan = G.Plan(((x / spec.divide_factor + 1) / 2).contiguous(), spec.grid)
    assert int(plan.face1.sum()) >= 68 and int((~plan.inside).sum()) >= 40
    ref = ref64.sdf_forward(net.params, net.cfg, x, (which,), grid="exact")
    y32 = ref64.sdf_forward(net.params, net.cfg, x, (which,), dtype=torch.float32, grid="exact")
    # the layout repeats points (257, 65 and 50 copies); a point's outputs do not depend on its neighbours (tests/test_gemm_float64_gpu.py
    # holds that bit for bit), so a copy is the same draw again and each distinct point is judged once
    _u, first = np.unique(x.numpy(), axis=0, return_index=True)
    distinct = torch.zeros(x.shape[0], dtype=torch.bool)
    distinct[torch.from_numpy(first)] = True
    on = torch.from_numpy(plan.face1) & distinct
    fails = []
    with capsys.disabled():
        print()
        for tile in (16, 32):
            out = k_sdf_forward(net, which, tile, x)
            for k, r, y in zip(("sdf", "grad", "feat"), ref, y32):
                gate(f"sdfnet_forward {net.geometry} {which} tile {tile} exact grid: {k}", out[k], r, y, fwd_norm(r), keep=distinct, failures=fails)
                gate(f"sdfnet_forward {net.geometry} {which} tile {tile} exact grid, u = 1 face: {k}", out[k], r, y, fwd_norm(r), keep=on,
                     failures=fails)
    assert not fails, [f["what"] for f in fails]
