"""Operands for tests/test_optim_float64_gpu.py and tests/test_optim_ref64_cpu.py: Adam states by operand class, weight-norm layer
tables, crafted points for the voxel counter and the Morton keys, and the judging of an Adam step class by class.

Adam classes, interleaved element by element (cycle A B C D E F G A rotated by the seed: every 16-byte group mixes them, class E is 1/8
of the elements); signs random, 2^U(a,b) log-uniform:
  A typical        s = 2^U(-20,6), g = s N(0,1), m0 = 0.5 s N(0,1), v0 = s^2 U(0.2,2)
  B untouched row  A with g = 0 exactly
  C never touched  g = m0 = v0 = 0: p bit-identical, m = v = 0 (equality, not the gate)
  D eps regime     sd = eps 2^U(-3,3), |g| = sd, v0 = sd^2 U(0.2,2), m0 = 0.5 sd N(0,1)   (eps: the case's own)
  E subnormal      |g| = 2^U(-70,-64), v0 = 2^U(-140,-128) (subnormal), m0 = 0.5 |g| N(0,1): p gated, m and v reported only
  F large          |g| = 2^U(64.6,66), v0 = 2^U(100,120), |m0| = 2^U(50,60): (w2 g) g is finite in fp32, g g is not
  G cancelling     A with g = m0 (1 + U(-1e-3,1e-3))
p0 cycles through exactly 0, +-2^U(-60,-20) and 0.1 N(0,1) (period 3 against the classes' 8)."""
import numpy as np
import torch

import optim_ref64 as R
from gate64 import gate, report

F32, F64 = torch.float32, torch.float64
CLASSES = "ABCDEFG"
CYCLE = "ABCDEFGA"
TINY = 2.0 ** -126

# (b1, b2, eps, lr)
HYPER = {"project": (0.9, 0.99, 1e-15, 0.04), "tracker": (0.9, 0.999, 1e-8, 0.005), "b1=0": (0.0, 0.99, 1e-15, 0.04),
         "lr=0": (0.9, 0.99, 1e-15, 0.0)}
STEPS = (1, 2, 7, 1000, 100000)
TABLE_N = (1, 3, 4, 5, 1023, 1024, 1025, 2051)     # every n % 4, both sides of the 256-group block, the block-0 tail


def adam_case(n, seed, eps, classes=CLASSES, b1=0.9):
    """-> dict(p0, g, m0, v0: fp32 [n]; cls: uint8 [n] holding ord(class)).  classes: the classes that occur (others are skipped in the
    cycle, e.g. "BC" for the zero-gradient forms).  b1: the case's beta1 -- where the draw makes the NEW first moment cancel,
    |b1 m0 + (1 - b1) g| < max(|m0|, |g|) / 16, m0 takes the other sign: p is judged relative to |p64 - p0|, which is proportional to
    that moment, so on such an element (one in ~20 of classes A, D, E) the rounding of m alone, magnified without bound, would decide
    the maximum for kernel and yardstick alike -- a coin toss between two correct evaluations, not a judgement.  (Where that is not
    enough -- b1 = 0, the new moment is g alone -- |m0| is reduced to |g|; not where g = 0: class B keeps its momentum, its new moment
    and its update are exactly 0 for b1 = 0 in every evaluation.)"""
    rng = np.random.default_rng(seed)
    cyc = [c for c in CYCLE if c in classes]
    cls = np.array([ord(c) for c in cyc], dtype=np.uint8)[(np.arange(n) + seed) % len(cyc)]
    sign = lambda: rng.choice([-1.0, 1.0], n)
    s = 2.0 ** rng.uniform(-20, 6, n)
    g, m0, v0 = s * rng.standard_normal(n), 0.5 * s * rng.standard_normal(n), s * s * rng.uniform(0.2, 2, n)
    is_ = lambda c: cls == ord(c)
    g[is_("B")] = 0.0
    for a in (g, m0, v0):
        a[is_("C")] = 0.0
    sd = R.f32(eps) * 2.0 ** rng.uniform(-3, 3, n)
    d = is_("D")
    g[d], v0[d], m0[d] = (sign() * sd)[d], (sd * sd * rng.uniform(0.2, 2, n))[d], (0.5 * sd * rng.standard_normal(n))[d]
    e = is_("E")
    ge = 2.0 ** rng.uniform(-70, -64, n)
    g[e], v0[e], m0[e] = (sign() * ge)[e], (2.0 ** rng.uniform(-140, -128, n))[e], (0.5 * ge * rng.standard_normal(n))[e]
    f = is_("F")
    g[f], v0[f], m0[f] = (sign() * 2.0 ** rng.uniform(64.6, 66, n))[f], (2.0 ** rng.uniform(100, 120, n))[f], \
        (sign() * 2.0 ** rng.uniform(50, 60, n))[f]
    gg = is_("G")
    g[gg] = (m0 * (1 + rng.uniform(-1e-3, 1e-3, n)))[gg]
    b1 = R.f32(b1)
    cancels = lambda: np.abs(b1 * m0 + (1 - b1) * g) < np.maximum(np.abs(m0), np.abs(g)) / 16
    m0[cancels()] *= -1.0
    still = cancels() & (g != 0)         # (a small b1: the new moment is the gradient, and |g| << |m0|; class B keeps its momentum)
    m0[still] = (np.sign(m0) * np.abs(g))[still]
    kind = np.arange(n) % 3
    p0 = np.where(kind == 0, 0.0, np.where(kind == 1, sign() * 2.0 ** rng.uniform(-60, -20, n), 0.1 * rng.standard_normal(n)))
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    return dict(p0=t(p0), g=t(g), m0=t(m0), v0=t(v0), cls=torch.from_numpy(cls), n=n, seed=seed)


def next_gradient(case, m_state, b1, div=1.0):
    """the raw gradient of a LATER step of a sequence, from a fresh case of the same class layout and the state the kernel left: class G
    follows the state's own first moment, and the cancelling rule of adam_case holds for (m_state, g / div) -- by the gradient's sign"""
    g, cls = case["g"].double().clone(), case["cls"]
    gg = cls == ord("G")
    rng = np.random.default_rng(case["seed"] + 17)
    g[gg] = (m_state.double() * torch.from_numpy(1 + rng.uniform(-1e-3, 1e-3, case["n"])) * div)[gg]
    b1, m = R.f32(b1), m_state.double()
    cancels = (b1 * m + (1 - b1) * g / div).abs() < torch.maximum(m.abs(), (g / div).abs()) / 16
    g[cancels] *= -1.0
    return g.float()


def adam_norms(case, r64):
    """per-element norms of (m, v, p): max(|m0|, |g|), max(v0, v64), max(|p0|, |p64 - p0|), each floored at 2^-126"""
    m64, v64, p64 = r64
    d = lambda k: case[k].double()
    return (torch.maximum(d("m0").abs(), d("g").abs()).clamp_min(TINY), torch.maximum(d("v0"), v64).clamp_min(TINY),
            torch.maximum(d("p0").abs(), (p64 - d("p0")).abs()).clamp_min(TINY))


class AdamJudge:
    """Adam results judged class by class and once pooled: a class with >= 64 elements in a case is gated on the spot, smaller ones
    are gathered over the cases and gated in ``finish``.  Class C is held to equality; class E's m and v are reported, not gated.
    The gate and the report are tests/gate64.py's, with the camera order as second yardstick unless ``table_order_only``."""

    def __init__(self, failures, caught=None, table_order_only=False):
        self.failures, self.table_order_only = failures, table_order_only
        self.pool, self.summary = {}, {}
        self.caught = caught             # optional set: the (quantity, class) pairs that FAILED are added instead of `failures`

    def _gate(self, what, rows, key=None):
        got, ref, y_a, y_b, norm = (torch.cat([r[i] for r in rows]) for i in range(5))
        if key is not None:              # the worst ratios per (quantity, class), for the summary table
            e_k, e_a, e_b = ((x - ref).abs() / norm for x in (got, y_a, y_b))
            rms = lambda e: float((e ** 2).mean().sqrt())
            rms_32, max_32 = max(rms(e_a), rms(e_b)), max(float(e_a.max()), float(e_b.max()))
            s = self.summary.setdefault(key, dict(gates=0, n=0, rms_k=0.0, max_k=0.0, rms_ratio=0.0, max_ratio=0.0))
            ratio = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else float("inf"))
            s.update(gates=s["gates"] + 1, n=s["n"] + norm.numel(), rms_k=max(s["rms_k"], rms(e_k)), max_k=max(s["max_k"], float(e_k.max())),
                     rms_ratio=max(s["rms_ratio"], ratio(rms(e_k), rms_32)), max_ratio=max(s["max_ratio"], ratio(float(e_k.max()), max_32)))
        fails = []
        ok = gate(what, got[:, None], ref[:, None], y_a[:, None], norm, torch.ones_like(norm, dtype=torch.bool), fails,
                  None if self.table_order_only else y_b[:, None])
        (self.failures if self.caught is None else []).extend(fails)
        return ok

    def add(self, tag, case, got, r64, y_table, y_camera):
        """got, r64, y_table, y_camera: (m, v, p) triples; the gate takes the larger of the two yardsticks' errors -- a kernel with ONE documented
        order is handed that yardstick twice, which makes the two-yardstick gate the plain one"""
        cls, norms = case["cls"], adam_norms(case, r64)
        c_ = cls == ord("C")
        if bool(c_.any()):
            still = torch.equal(got[2][c_], case["p0"][c_]) and bool((got[0][c_] == 0).all()) and bool((got[1][c_] == 0).all())
            if self.caught is not None and not still:
                self.caught.add(("p", "C"))
            assert still or self.caught is not None, f"{tag}: a never-touched element (class C) moved"
        for qi, q in enumerate("mvp"):
            for c in CLASSES:
                sel = cls == ord(c)
                if c == "C" or not bool(sel.any()):
                    continue
                row = tuple(x[qi].double()[sel] for x in (got, r64, y_table, y_camera)) + (norms[qi][sel],)
                if not bool(torch.isfinite(row[0]).all()):
                    assert self.caught is not None, f"{tag}: {q} of class {c} is not finite"
                    self.caught.add((q, c))
                    continue
                if c == "E" and q != "p":
                    self.pool.setdefault((q, c, "report"), []).append(row)
                    continue
                self.pool.setdefault((q, "pooled", "gate"), []).append(row)
                if int(sel.sum()) >= 64:
                    if not self._gate(f"{tag}: {q} class {c}", [row], (q, c)) and self.caught is not None:
                        self.caught.add((q, c))
                else:
                    self.pool.setdefault((q, c, "gate"), []).append(row)

    def finish(self, tag):
        """gates what was pooled; -> the summary lines, one per quantity"""
        for (q, c, how), rows in sorted(self.pool.items()):
            if how == "report":
                got, ref, y_a, _y_b, norm = (torch.cat([r[i] for r in rows]).cpu() for i in range(5))
                report(f"{tag}: {q} class {c}", got[:, None], ref[:, None], y_a[:, None], norm, torch.ones_like(norm, dtype=torch.bool))
            elif not self._gate(f"{tag}: {q} class {c} (over cases)", rows, (q, c)) and self.caught is not None:
                self.caught.add((q, c))
        self.pool = {}
        lines = []
        for q in "mvp":                  # one line per quantity: the worst gate of any class (and of the pooled one), class in brackets
            rows = {c: s for (q_, c), s in self.summary.items() if q_ == q}
            if not rows:
                continue
            own = [s for c, s in rows.items() if c != "pooled"] or list(rows.values())
            worst = lambda k: max((s[k], c) for c, s in rows.items())
            lines.append(f"  == {tag:<50s} {q}  gates {sum(s['gates'] for s in rows.values()):4d}  elements {sum(s['n'] for s in own):9d}  "
                  f"e_k rms <= {worst('rms_k')[0]:.2e} max <= {worst('max_k')[0]:.2e}   x yardstick: rms <= {worst('rms_ratio')[0]:.2f} "
                  f"({worst('rms_ratio')[1]})  max <= {worst('max_ratio')[0]:.2f} ({worst('max_ratio')[1]})")
        self.summary = {}
        return lines


# ------------------------------------------------------------------------------------------------------------------ weight norm
WN_COLS = (1, 3, 63, 64, 65, 257)
WN_ROWS = (1, 2, 65)


def wn_layers(n_layers, seed):
    """[(v, g, bias)] fp32: cols and rows cycle through WN_COLS x WN_ROWS from the seed; elements +-2^U(-20,20) within a row; in every
    layer row 0 has a single non-zero entry (when cols > 1), g cycles positive / negative / zero"""
    rng = np.random.default_rng(seed)
    layers = []
    for l in range(n_layers):
        cols, rows = WN_COLS[(l + seed) % len(WN_COLS)], WN_ROWS[(l + seed // 2) % len(WN_ROWS)]
        v = rng.choice([-1.0, 1.0], (rows, cols)) * 2.0 ** rng.uniform(-20, 20, (rows, cols))
        if cols > 1:
            keep = v[0, cols // 2]
            v[0] = 0.0
            v[0, cols // 2] = keep
        g = rng.standard_normal(rows) * 2.0 ** rng.uniform(-3, 3, rows)
        g[(np.arange(rows) + l) % 5 == 1] *= -1.0
        g[(np.arange(rows) + l) % 7 == 3] = 0.0
        b = rng.standard_normal(rows)
        layers.append(tuple(torch.from_numpy(a.astype(np.float32)) for a in (v, g, b)))
    return layers


def wn_cotangent(layers, seed):
    """-> (g_flat fp32 [total + 1], c [total rows] float64 per-row scales): rows scaled by 2^U(-30,30) (objective_cases.scales: every
    97th zero, and global row 2 zero); in every layer the LAST row's gW is parallel to v (the cancelling case)"""
    import objective_cases as C
    g = torch.Generator().manual_seed(seed)
    n_rows = sum(v.shape[0] for v, _g, _b in layers)
    c = C.scales(n_rows, g)
    if n_rows > 2:
        c[2] = 0.0
    parts, r0 = [], 0
    for v, _g, _b in layers:
        rows, cols = v.shape
        gw = torch.randn(rows, cols, generator=g, dtype=F64)
        gw[-1] = v[-1].double() / v[-1].double().norm() * 1.5
        cr = c[r0:r0 + rows]
        parts += [(gw * cr[:, None]).float().reshape(-1), (torch.randn(rows, generator=g, dtype=F64) * cr).float()]
        r0 += rows
    return torch.cat(parts + [torch.zeros(1)]), c


# ------------------------------------------------------------------------------------------------------------------ voxels and keys
VOXEL_P = (1, 63, 64, 65, 257)
VOXEL_RES = (1, 37, 64, 1024)


def _neighbours(x):
    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])


def crafted_coordinates(nan=False):
    """fp32 coordinates on the cell boundaries k / 32 - 1 and both fp32 neighbours, +-0.99f and both neighbours, -0.0, +-1, +-1.5"""
    k = np.arange(0, 65, dtype=np.float32) / np.float32(32) - np.float32(1)
    c = np.concatenate([_neighbours(k), _neighbours([0.99, -0.99]), np.array([-0.0, 0.0, 1.0, -1.0, 1.5, -1.5], dtype=np.float32)])
    if nan:
        c = np.concatenate([c, np.array([np.nan, 3.0, -3.0, 0.998046875, 0.9999999], dtype=np.float32)])
    return c.astype(np.float32)


def crafted_points(P, seed, nan=False):
    """[P,3] fp32: every coordinate drawn from crafted_coordinates (some points all-inside so that they count)"""
    rng = np.random.default_rng(seed)
    c = crafted_coordinates(nan)
    inside = c[np.abs(c) <= np.float32(0.99)]
    x = rng.choice(c, (P, 3))
    x[::2] = rng.choice(inside, (P, 3))[::2]
    return x.astype(np.float32)


def run_points(kind):
    """runs for the wave-merging scatter: 'same' 64 identical points; 'straddle' a run of 40 equal points across the wave boundary at
    64 inside 128; 'alternate' two voxels alternating over 130 points"""
    a, b = np.array([0.5, -0.25, 0.125], dtype=np.float32), np.array([-0.75, 0.96875, 0.0], dtype=np.float32)
    if kind == "same":
        return np.tile(a, (64, 1))
    if kind == "straddle":
        x = np.random.default_rng(5).uniform(-0.98, 0.98, (128, 3)).astype(np.float32)
        x[44:84] = a
        return x
    assert kind == "alternate"
    return np.stack([a if i % 2 == 0 else b for i in range(130)])
