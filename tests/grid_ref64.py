"""The multi-resolution grid encoder in plain, dtype-generic torch (test infrastructure): value, explicit Jacobian, first backward
(J^T g and the table scatter) and the second backward (J q and the second-order table scatter), in float64 or float32.

It restates the reference encoder (hashencoder.cu, as oracle/hashenc_oracle.c restates it) statement by statement:
  * level geometry: scale = exp2f(l S) H - 1 as an fp32 number, res = ceil(scale) + 1;
  * row index: uint32 arithmetic in numpy -- the stride loop with wrap-around, the xor-prime hash, the modulo;
  * weights: smoothstep w = t^2 (3 - 2 t) and dw = 6 t (1 - t); the corner weight is the running product ((1 wx) wy) wz;
  * the 2^D-corner sum runs corner 0 .. 2^D - 1, the Jacobian row face by face as (wt (hi - lo)) dw.
In float32 every statement is one rounded torch operation in the oracle's order, so value and Jacobian equal the C oracle's bit for
bit (tests/test_grid_ref64_cpu.py); the scatters add in (point, corner) order like the oracle's loops.

What is discrete comes from the fp32 inputs, in every dtype: the in-range test 0 <= u <= 1 on the fp32 unit coordinate ``u32`` and
cell = trunc(fl32(u32 scale)).  In float64 the fraction is t = u scale - cell from the promoted values; where fp32 rounded
u scale across a cell border t is a hair below 0 or above 1.  Nothing is left out there: w(0) = 0, w(1) = 1 and dw(0) = dw(1) = 0, so
value and Jacobian are continuous across the border and the cell fp32 chose is as good as its neighbour to within that hair squared.

The derivative structure mirrors oracle/render_ref.py::_Encode / _EncodeBwd: the backward of the backward gives J q to the cotangent
and the second-order scatter to the table and nothing to x -- the grid-Hessian term is dropped as the reference drops it
(hashgrid.py:134).

``paths`` derives, from the integer arithmetic alone, which lanes of the scatter kernels (csrc/grid_common.hpp: scatter_x_pair,
scatter_span) take which path for a batch; tests/test_grid_ref64_cpu.py asserts the counts non-zero on the inputs of
tests/test_grid_float64_gpu.py.  ``kernel_order_scatter`` is the kernels' order of summation in fp32, the second yardstick of that file."""
from collections import namedtuple

import numpy as np
import torch

F64 = torch.float64
PRIMES = (1, 2654435761, 805459861)
INVALID = -1                                    # the key of a lane with nothing to add
Level = namedtuple("Level", "scale res row0 rows hashed")
# (levels, channels, base resolution, finest resolution, log2 of the row cap) of the row-by-row tests
GEOMS = {"coarse": (4, 8, 32, 32, 19), "fine": (8, 4, 32, 128, 19), "colour_small": (16, 2, 16, 512, 19), "c8": (6, 8, 16, 96, 15)}
TINY = {f"tiny{lm}_c{C}": (4, C, 4, 32, lm) for lm in (1, 3, 5) for C in (2, 4)}


def spec_of(name):
    from oracle import render_ref as R
    return R.make_grid_spec(*{**GEOMS, **TINY}[name])


def levels(spec):
    """Per level: scale (np.float32), res, row0, rows, hashed -- hashencoder.cu:179-181 and the stride loop of :56-70."""
    S = np.float32(np.log2(spec.per_level_scale))
    off = [int(o) for o in spec.offsets]
    out = []
    for l in range(spec.num_levels):
        e = np.float32(l) * S                                             # (float)level * S, one fp32 rounding
        scale = np.float32(np.float32(np.exp2(np.float64(e))) * np.float32(spec.base_resolution)) - np.float32(1.0)
        res = int(np.ceil(scale)) + 1
        rows = off[l + 1] - off[l]
        stride, d = 1, 0
        while d < spec.input_dim and stride <= rows:
            stride = (stride * res) & 0xFFFFFFFF
            d += 1
        out.append(Level(np.float32(scale), res, off[l], rows, stride > rows))
    return out


def level_row(lv, q, D):
    """Row inside the level of the integer corner coordinates q [N, D] (uint32) -> uint32 [N]  (get_grid_index, :54-73)."""
    q = q.astype(np.uint32)
    with np.errstate(over="ignore"):
        stride, idx, d = np.uint32(1), np.zeros(q.shape[0], np.uint32), 0
        while d < D and int(stride) <= lv.rows:
            idx = idx + q[:, d] * stride
            stride = np.uint32((int(stride) * lv.res) & 0xFFFFFFFF)
            d += 1
        if int(stride) > lv.rows:
            idx = np.zeros(q.shape[0], np.uint32)
            for d in range(D):
                idx = idx ^ (q[:, d] * np.uint32(PRIMES[d]))
    return idx % np.uint32(lv.rows)


class Plan:
    """Everything discrete of one batch: inside [B] (bool), per level the cell [B, D] (int64, 0 for points out of range) and the
    table row (row0 included) of every corner [B, 2^D] (int64; corner bit d set <=> +1 along dim d)."""

    def __init__(self, u32, spec):
        assert u32.dtype == torch.float32
        u32 = u32.detach()
        self.spec, self.lv = spec, levels(spec)
        self.B, self.D = u32.shape
        self.L, self.C = spec.num_levels, spec.level_dim
        self.inside = ((u32 >= 0) & (u32 <= 1)).all(dim=1)
        self.face1 = ((u32 == 1).any(dim=1) & self.inside).numpy()           # in range and on a u = 1 face
        self.cell, self.rows = [], []
        for lv in self.lv:
            p = u32 * torch.tensor(float(lv.scale), dtype=torch.float32)      # fl32(u scale)
            cell = torch.where(self.inside[:, None], p.floor(), torch.zeros_like(p)).to(torch.int64)
            cn = cell.numpy().astype(np.uint32)
            r = np.empty((self.B, 1 << self.D), np.int64)
            for corner in range(1 << self.D):
                bits = np.array([(corner >> d) & 1 for d in range(self.D)], np.uint32)
                r[:, corner] = level_row(lv, cn + bits[None, :], self.D).astype(np.int64) + lv.row0
            self.cell.append(cell)
            self.rows.append(torch.from_numpy(r))


def _weights(plan, l, u):
    """t, w, dw [B, D] in u's dtype; the fraction of the cell the fp32 inputs chose."""
    t = u * torch.tensor(float(plan.lv[l].scale), dtype=u.dtype) - plan.cell[l].to(u.dtype)
    return t * t * (3.0 - 2.0 * t), 6.0 * t * (1.0 - t)


def _corner_weight(w, corner, D, start=None, skip=None):
    wt = torch.ones_like(w[:, 0]) if start is None else start
    for d in range(D):
        if d == skip:
            continue
        wt = wt * (w[:, d] if (corner >> d) & 1 else 1.0 - w[:, d])
    return wt


def encode(plan, u, emb, jac=True):
    """-> y [B, L, C], J [B, L, D, C] (d y / d u; None without jac).  u: the unit coordinates in the working dtype."""
    B, D, L, C = plan.B, plan.D, plan.L, plan.C
    dt = u.dtype
    y = torch.zeros(B, L, C, dtype=dt)
    J = torch.zeros(B, L, D, C, dtype=dt) if jac else None
    ins = plan.inside[:, None]
    for l in range(L):
        w, dw = _weights(plan, l, u)
        v = emb[plan.rows[l]]                                              # [B, 2^D, C]
        acc = torch.zeros(B, C, dtype=dt)
        for corner in range(1 << D):
            acc = acc + _corner_weight(w, corner, D)[:, None] * v[:, corner]
        y[:, l] = torch.where(ins, acc, torch.zeros_like(acc))
        if not jac:
            continue
        scale = torch.full((B,), float(plan.lv[l].scale), dtype=dt)
        for gd in range(D):
            acc = torch.zeros(B, C, dtype=dt)
            for face in range(1 << (D - 1)):
                lo = 0
                for nd in range(D - 1):
                    d = nd + 1 if nd >= gd else nd
                    lo |= ((face >> nd) & 1) << d
                wt = _corner_weight(w, lo, D, start=scale, skip=gd)
                acc = acc + wt[:, None] * (v[:, lo | (1 << gd)] - v[:, lo]) * dw[:, gd:gd + 1]
            J[:, l, gd] = torch.where(ins, acc, torch.zeros_like(acc))
    return y, J


def _scatter(plan, l, contrib, n_rows, out, norms=None, unit=None):
    """out[row] += contrib[b, corner] in (point, corner) order, in-range points only; norms = per row (sum of the contributions' norms,
    their number, sum of the contributing points' units [B]: what a point sends into its CELL, whatever the corner's weight)."""
    sel = plan.inside
    idx = plan.rows[l][sel].reshape(-1)
    val = contrib[sel].reshape(-1, contrib.shape[-1])
    out.index_add_(0, idx, val)
    if norms is not None:
        norms[0].index_add_(0, idx, val.double().norm(dim=1))
        norms[1].index_add_(0, idx, torch.ones_like(idx))
        norms[2].index_add_(0, idx, unit.double()[sel].repeat_interleave(contrib.shape[1]))


def backward(plan, u, g, J=None, n_rows=None, with_norms=False):
    """g [B, L, C] -> (J^T g [B, D] or None, table gradient [n_rows, C]) and, with_norms, per table row the sum over its contributions
    of their Euclidean norm (float64), their number, and the sum of the contributing points' |g[b, l]| (_scatter)."""
    B, D, L, C = plan.B, plan.D, plan.L, plan.C
    n_rows = plan.spec.n_rows if n_rows is None else n_rows
    gt = torch.zeros(n_rows, C, dtype=g.dtype)
    norms = (torch.zeros(n_rows, dtype=F64), torch.zeros(n_rows, dtype=torch.int64), torch.zeros(n_rows, dtype=F64)) if with_norms else None
    for l in range(L):
        w, _dw = _weights(plan, l, u)
        contrib = torch.stack([_corner_weight(w, corner, D)[:, None] * g[:, l] for corner in range(1 << D)], dim=1)
        _scatter(plan, l, contrib, n_rows, gt, norms, g[:, l].norm(dim=1))
    gu = None
    if J is not None:
        gu = torch.zeros(B, D, dtype=g.dtype)
        for d in range(D):
            r = torch.zeros(B, dtype=g.dtype)
            for l in range(L):
                for c in range(C):
                    r = r + g[:, l, c] * J[:, l, d, c]
            gu[:, d] = r
    return (gu, gt, norms) if with_norms else (gu, gt)


def second_backward(plan, u, g, J, q, n_rows=None, with_norms=False):
    """q [B, D] (the cotangent of J^T g) -> (J q [B, L, C], second-order table gradient [n_rows, C])  (hashencoder.cu:405-625)."""
    B, D, L, C = plan.B, plan.D, plan.L, plan.C
    n_rows = plan.spec.n_rows if n_rows is None else n_rows
    dt = g.dtype
    gg = torch.zeros(B, L, C, dtype=dt)
    for d in range(D):
        gg = gg + q[:, None, d:d + 1] * J[:, :, d]
    g2 = torch.zeros(n_rows, C, dtype=dt)
    norms = (torch.zeros(n_rows, dtype=F64), torch.zeros(n_rows, dtype=torch.int64), torch.zeros(n_rows, dtype=F64)) if with_norms else None
    for l in range(L):
        w, dw = _weights(plan, l, u)
        scale = torch.full((B,), float(plan.lv[l].scale), dtype=dt)
        cache = [torch.zeros(B, C, dtype=dt) for _ in range(1 << D)]
        for gd in range(D):
            for face in range(1 << (D - 1)):
                lo = 0
                for nd in range(D - 1):
                    d = nd + 1 if nd >= gd else nd
                    lo |= ((face >> nd) & 1) << d
                wt = _corner_weight(w, lo, D, start=scale, skip=gd)
                v = wt[:, None] * g[:, l] * q[:, gd:gd + 1] * dw[:, gd:gd + 1]
                cache[lo | (1 << gd)] = cache[lo | (1 << gd)] + v
                cache[lo] = cache[lo] - v
        _scatter(plan, l, torch.stack(cache, dim=1), n_rows, g2, norms, g[:, l].norm(dim=1) * q.abs().amax(dim=1) * float(plan.lv[l].scale))
    return (gg, g2, norms) if with_norms else (gg, g2)


def scatter_contribs(plan, contribs, units, dtype=F64):
    """per-corner rows contribs[l] [B, 2^D, C] and per-point units[l] [B] -> (table gradient, (sum of norms, count, sum of units)):
    for sites that add value path and double-backward share as ONE row per corner (the fused SDF kernels)"""
    n_rows = plan.spec.n_rows
    out = torch.zeros(n_rows, plan.C, dtype=dtype)
    norms = (torch.zeros(n_rows, dtype=F64), torch.zeros(n_rows, dtype=torch.int64), torch.zeros(n_rows, dtype=F64))
    for l in range(plan.L):
        _scatter(plan, l, contribs[l].to(dtype), n_rows, out, norms, units[l])
    return out, norms


def compact(plan):
    """-> (rows [K] sorted, a copy of the plan whose corner rows index into them): the touched rows of a table too large to hold
    densely on the host; pass n_rows = K to backward / second_backward with it"""
    import copy
    uniq = torch.unique(torch.cat([r[plan.inside].reshape(-1) for r in plan.rows]))
    small = copy.copy(plan)
    small.rows = [torch.searchsorted(uniq, r.contiguous()).clamp_max(uniq.numel() - 1) for r in plan.rows]
    return uniq, small


# ------------------------------------------------------------------------------------------------- the differentiable pair
class _EncodeBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, u, emb, plan, J):
        gu, gt = backward(plan, u.detach(), g.detach().reshape(plan.B, plan.L, plan.C), J, emb.shape[0])
        if hasattr(plan, "record"):
            plan.record.append(("first", g.detach().reshape(plan.B, plan.L, plan.C)))
        ctx.save_for_backward(g, u, J)
        ctx.plan, ctx.n_rows = plan, emb.shape[0]
        return gu, gt

    @staticmethod
    def backward(ctx, q, _gg_table_unused):
        g, u, J = ctx.saved_tensors
        p = ctx.plan
        gg, g2 = second_backward(p, u.detach(), g.detach().reshape(p.B, p.L, p.C), J, q, ctx.n_rows)
        if hasattr(p, "record"):
            p.record.append(("second", g.detach().reshape(p.B, p.L, p.C), q.detach()))
        return gg.reshape(g.shape), None, g2, None, None          # nothing to x: the grid-Hessian term is dropped


class _Encode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, emb, plan):
        y, J = encode(plan, u.detach(), emb.detach())
        ctx.save_for_backward(u, emb, J)
        ctx.plan = plan
        return y.reshape(plan.B, plan.L * plan.C)

    @staticmethod
    def backward(ctx, g):
        u, emb, J = ctx.saved_tensors
        gu, gt = _EncodeBwd.apply(g.contiguous(), u, emb, ctx.plan, J)
        return gu, gt, None


def grid_features(u, emb, spec, u32=None, plan=None):
    """Differentiable features [B, L C] of the unit coordinates u (any dtype); the discrete part comes from u32 (default: u itself,
    which must then be fp32)."""
    plan = plan or Plan(u if u32 is None else u32, spec)
    return _Encode.apply(u, emb, plan)


# ------------------------------------------------------------------------------------------------- the fp32 yardstick
def oracle_suite(spec, emb, u, g, q):
    """the C oracle (fp32) on the same inputs, in this module's layouts: y, gg [B, L, C]; J [B, L, D, C]; gu [B, D]; gt, g2 [rows, C]"""
    B, D, L, C = u.shape[0], 3, spec.num_levels, spec.level_dim
    S, H = float(np.log2(spec.per_level_scale)), spec.base_resolution
    out, dy = torch.empty(L, B, C), torch.empty(B, L * D * C)
    from oracle.hashenc import OracleBackend as O
    O.hash_encode_forward(u, emb, spec.offsets, out, B, D, C, L, S, H, True, dy)
    gl = g.permute(1, 0, 2).contiguous()
    gt, gu = torch.zeros_like(emb), torch.zeros(B, D)
    O.hash_encode_backward(gl, u, emb, spec.offsets, gt, B, D, C, L, S, H, True, dy, gu)
    gg, g2 = torch.zeros(L, B, C), torch.zeros_like(emb)
    O.hash_encode_second_backward(gl, u, emb, spec.offsets, B, D, C, L, S, H, True, dy, q.contiguous(), gg, g2)
    return dict(y=out.permute(1, 0, 2), J=dy.view(B, L, D, C), gu=gu, gt=gt, gg=gg.permute(1, 0, 2), g2=g2)


# ------------------------------------------------------------------------------------------------- the kernels' order of summation
def _span_scan(key, val):
    """scatter_span's run merge for many waves at once: key [n, 64] (INVALID: nothing to add), val [n, 64, W] fp32 -> (send [n, 64],
    the run sums at the runs' last lanes).  A Hillis-Steele scan: in step off every lane adds the value of lane - off if both are in
    the same segment; a segment starts at lane 0, at a change of key, and at every INVALID lane."""
    head = np.ones(key.shape, bool)
    head[:, 1:] = (key[:, 1:] != key[:, :-1]) | (key[:, 1:] == INVALID)
    seg = np.cumsum(head, axis=1)
    off = 1
    while off < 64:
        take = np.zeros(key.shape, bool)
        take[:, off:] = seg[:, off:] == seg[:, :-off]
        o = np.zeros_like(val)
        o[:, off:] = val[:, :-off]
        val = np.where(take[..., None], val + o, val)
        off <<= 1
    tail = np.ones(key.shape, bool)
    tail[:, :-1] = head[:, 1:]
    return tail & (key != INVALID), val


def _emit(table, send, row, val):
    np.add.at(table, row[send], val[send])                     # unbuffered: one fp32 addition after the other, in (wave, lane) order


def kernel_order_scatter(plan, contrib):
    """The table scatter of k_grid_scatter / k_grid_second_backward<SCATTER> (csrc/hash_encode.hip) statement by statement in fp32:
    contrib[l] = [B, 2^D, C] fp32 per-corner rows -> table gradient [n_rows, C].  Per level and x-neighbour corner pair: the wave of 64
    consecutive points sends adjacent rows as one span (scatter_x_pair: the halves swapped on a `down` pair), run-merged by
    _span_scan's scan, and the others as two single rows with a scan each.  The order in which the atomics of different waves reach
    a row is the hardware's; here wave after wave."""
    B, D, C = plan.B, plan.D, plan.C
    n = -(-B // 64)
    table = np.zeros((plan.spec.n_rows, C), np.float32)
    ins = np.zeros(n * 64, bool)
    ins[:B] = plan.inside.numpy()

    def waves(a, fill):
        out = np.full((n * 64,) + a.shape[1:], fill, a.dtype)
        out[:B] = a
        return out.reshape((n, 64) + a.shape[1:])
    for l in range(plan.L):
        r, v = plan.rows[l].numpy(), contrib[l].numpy().astype(np.float32)
        for yz in range(1 << (D - 1)):
            r0, r1 = waves(r[:, 2 * yz], 0), waves(r[:, 2 * yz + 1], 0)
            v0, v1 = waves(v[:, 2 * yz], 0), waves(v[:, 2 * yz + 1], 0)
            valid = ins.reshape(n, 64)
            up, down = valid & (r1 == r0 + 1), valid & (r0 == r1 + 1)
            adj = up | down
            lo = np.where(down[..., None], v1, v0)
            hi = np.where(down[..., None], v0, v1)
            key = np.where(adj, np.where(down, r1, r0), INVALID)
            send, val = _span_scan(key, np.concatenate([lo, hi], axis=2))
            _emit(table, send, key, val[..., :C])
            _emit(table, send, key + 1, val[..., C:])
            single = valid & ~adj
            if single.any():
                for rr, vv in ((r0, v0), (r1, v1)):
                    key = np.where(single, rr, INVALID)
                    send, val = _span_scan(key, vv.copy())
                    _emit(table, send, key, val)
    return torch.from_numpy(table)


def _fused_complement(plan, l, u):
    """1 - w as the compiler forms it in the kernels' `1.0f - w[d]` with w = (t t) (3 - 2 t): ONE fused multiply-add, 1 - (t t) (3 - 2 t)
    rounded once (the product of two fp32 numbers is exact in float64).  Near t = 1 the unfused form rounds w to 1 and gives 0 where
    this one gives 3 (1 - t)^2 to a few per cent: a different and equally valid fp32 evaluation."""
    t = u * torch.tensor(float(plan.lv[l].scale), dtype=u.dtype) - plan.cell[l].to(u.dtype)
    return (1.0 - (t * t).double() * (3.0 - 2.0 * t).double()).float()


def _corner_weight_fused(w, nw, corner, D, start=None, skip=None):
    wt = torch.ones_like(w[:, 0]) if start is None else start
    for d in range(D):
        if d != skip:
            wt = wt * (w[:, d] if (corner >> d) & 1 else nw[:, d])
    return wt


def kernel_order_contribs(plan, u, g, q=None):
    """per-corner rows as the scatter kernels form them: first order w_corner g; second order the scalar k_corner = sum over
    (gd, face) of +- ((scale w w) q_gd) dw_gd, then k_corner g.  In fp32 the complements 1 - w are the fused ones (_fused_complement);
    in float64 this is the plain arithmetic."""
    D, out = plan.D, []
    for l in range(plan.L):
        w, dw = _weights(plan, l, u)
        if u.dtype == torch.float32:
            nw = _fused_complement(plan, l, u)
            cw = lambda corner, **kw: _corner_weight_fused(w, nw, corner, D, **kw)
        else:
            cw = lambda corner, **kw: _corner_weight(w, corner, D, **kw)
        if q is None:
            out.append(torch.stack([cw(corner)[:, None] * g[:, l] for corner in range(1 << D)], dim=1))
            continue
        scale = torch.full((plan.B,), float(plan.lv[l].scale), dtype=u.dtype)
        k = [torch.zeros(plan.B, dtype=u.dtype) for _ in range(1 << D)]
        for gd in range(D):
            for face in range(1 << (D - 1)):
                lo = 0
                for nd in range(D - 1):
                    d = nd + 1 if nd >= gd else nd
                    lo |= ((face >> nd) & 1) << d
                t = cw(lo, start=scale, skip=gd) * q[:, gd] * dw[:, gd]
                k[lo | (1 << gd)] = k[lo | (1 << gd)] + t
                k[lo] = k[lo] - t
        out.append(torch.stack([k[corner][:, None] * g[:, l] for corner in range(1 << D)], dim=1))
    return out


# ------------------------------------------------------------------------------------------------- which path does a lane take


def paths(plan, lanes=64, block=256):
    """Counts, over all levels and x-neighbour corner pairs, of the paths of scatter_x_pair / scatter_span for the batch in its given
    order (lane = point index % 64; the fused sites tile differently, but the classes below exist for them at the same inputs)."""
    B, D = plan.B, plan.D
    b = np.arange(B)
    ins = plan.inside.numpy()
    n = dict(up=0, down=0, single_hashed_odd_x=0, single_dense_wrap=0, run_pairs=0, full_wave_runs=0, equal_across_wave=0,
             equal_across_block=0, equal_across_invalid=0, up_next_to_down=0, corners_collide=0, face_dense_nonpow2=0)
    for l, lv in enumerate(plan.lv):
        r = plan.rows[l].numpy() - lv.row0
        pow2 = lv.rows & (lv.rows - 1) == 0
        distinct = np.array([len(set(row)) for row in r])
        n["corners_collide"] += int(((distinct < (1 << D)) & ins).sum())
        if not lv.hashed and not pow2:
            n["face_dense_nonpow2"] += int(plan.face1.sum())
        for yz in range(1 << (D - 1)):
            r0, r1 = r[:, 2 * yz], r[:, 2 * yz + 1]
            up, down = (r1 == r0 + 1) & ins, (r0 == r1 + 1) & ins
            single = ins & ~up & ~down
            n["up"] += int(up.sum())
            n["down"] += int(down.sum())
            odd = (plan.cell[l][:, 0].numpy() & 1) == 1
            if lv.hashed:
                n["single_hashed_odd_x"] += int((single & odd).sum())
            else:
                n["single_dense_wrap"] += int(single.sum())
            key = np.where(up, r0, np.where(down, r1, INVALID))
            same_wave = (b[:-1] // lanes) == (b[1:] // lanes)
            eq = (key[:-1] == key[1:]) & (key[:-1] != INVALID)
            n["run_pairs"] += int((eq & same_wave).sum())
            n["equal_across_wave"] += int((eq & ~same_wave).sum())
            n["equal_across_block"] += int((eq & ((b[1:] % block) == 0)).sum())
            n["up_next_to_down"] += int((eq & same_wave & (up[:-1] != up[1:])).sum())
            if B >= 3:
                gap = (key[:-2] == key[2:]) & (key[:-2] != INVALID) & (key[1:-1] == INVALID) & ((b[:-2] // lanes) == (b[2:] // lanes))
                n["equal_across_invalid"] += int(gap.sum())
            for w0 in range(0, B - lanes + 1, lanes):
                k = key[w0:w0 + lanes]
                n["full_wave_runs"] += int(k[0] != INVALID and (k == k[0]).all())
    return n


# ------------------------------------------------------------------------------------------------- the inputs of the row-by-row tests
def _morton(u, bits=10):
    q = np.clip((u.numpy().astype(np.float64) * (1 << bits)).astype(np.int64), 0, (1 << bits) - 1)
    code = np.zeros(q.shape[0], np.int64)
    for k in range(bits):
        for d in range(3):
            code |= ((q[:, d] >> k) & 1) << (3 * k + (2 - d))
    return code


def points(B, spec, seed=0):
    """Unit coordinates [B, 3] (fp32) out of one fixed layout of 4123 (= 16 x 256 + 27) points: all of it, or for a smaller B the B
    points from 192 on (65 copies of one point -- a full wave and one lane more -- then ray samples) with, from 16 points on, five
    lanes given to the other families (an out-of-range point between two copies, u = 1, u = 0, a uniform point, a cell border):
        0 ..  256   257 copies of one point (a run that fills wave 0, equal rows across the wave boundaries 63|64, 127|128, 191|192 and
                    the block boundary 255|256), with lanes 70 and 133 out of range (u in (1, 1.5] resp. u < 0 in one coordinate)
                    between two lanes of equal row, and 65 copies of a second point from 300
      257 .. 1280   8 rays of 128 consecutive samples, step 1/16 of the finest cell
     1281 .. 2304   the same samples in Morton order
     2305 .. 2400   points exactly at u = 0, at u = 1 (single coordinates and all three), and on interior cell borders of every level
     2401 .. 2500   out of range in one coordinate, interleaved with in-range copies of one point
     the rest       uniform."""
    N = 4123
    g = torch.Generator().manual_seed(1000 + seed)
    lv = levels(spec)
    u = torch.rand(N, 3, generator=g)
    p0 = torch.tensor([0.3217, 0.6121, 0.4409])
    u[0:257] = p0
    u[300:365] = torch.tensor([0.7143, 0.2087, 0.5511])
    u[70, 1] = 1.25
    u[133, 2] = -0.125
    finest = float(lv[-1].scale)
    o = torch.rand(8, 1, 3, generator=g) * 0.6 + 0.2
    d = torch.nn.functional.normalize(torch.randn(8, 1, 3, generator=g), dim=-1)
    s = torch.arange(128, dtype=torch.float32).reshape(1, 128, 1) * (1.0 / (16.0 * finest))
    rays = (o + s * d).reshape(-1, 3).clamp(0.0, 1.0)
    u[257:1281] = rays
    u[1281:2305] = rays[torch.from_numpy(np.argsort(_morton(rays), kind="stable"))]
    k = 2305
    for face in (0.0, 1.0):
        for dim in range(3):
            u[k, dim] = face
            k += 1
        u[k] = face
        k += 1
    for l, v in enumerate(lv):                      # u scale an exact integer on level l: u = m / scale rounded so that fl32(u scale) == m
        for m in (1, int(v.scale) // 2, int(v.scale) - 1):
            if m < 1 or k >= 2400:
                continue
            c = np.float32(m) / v.scale
            for cand in (c, np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-1))):
                if np.float32(cand) * v.scale == np.float32(m):
                    u[k, l % 3] = float(cand)
                    k += 1
                    break
    u[2401:2501] = torch.tensor([0.5511, 0.3217, 0.8087])
    out = torch.arange(2402, 2501, 2)
    u[out, out % 3] = torch.where(out % 4 == 0, 1.0 + torch.rand(out.shape[0], generator=g) * 0.5, -torch.rand(out.shape[0], generator=g) - 1e-3)
    u[2500, 0] = 1.5
    if B == N:
        return u.contiguous()
    idx = torch.arange(192, 192 + B)
    if B >= 16:                     # one lane of every other family: out of range, u = 1, u = 0, uniform, a cell border
        at = 64 if B >= 128 else 0  # (from 128 points on behind the first wave, which stays one run)
        idx[torch.tensor([5, 9, 11, 13, 14]) + at] = torch.tensor([70, 2309, 2305, 3000, 2314])
    return u[idx].contiguous()


def table(spec, seed=0):
    """randn times a per-row factor 2^U(-12, 12)"""
    g = torch.Generator().manual_seed(2000 + seed)
    e = torch.rand(spec.n_rows, 1, generator=g) * 24 - 12
    return (torch.randn(spec.n_rows, spec.level_dim, generator=g) * torch.exp2(e)).contiguous()


def point_scales(n, seed=0):
    """c_p = 2^U(-30, 30); within the first half neighbours alternate 2^30 / 2^-30; every 97th point 0"""
    g = torch.Generator().manual_seed(3000 + seed)
    e = torch.randint(-30, 31, (n,), generator=g).double()
    h = torch.arange(n // 2)
    e[h] = torch.where(h % 2 == 0, 30.0, -30.0).double()
    c = torch.exp2(e)
    c[torch.arange(n) % 97 == 5] = 0.0
    return c
