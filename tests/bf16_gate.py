"""The per-point gate that holds a bf16-operand kernel to the float64-accumulating bf16 reference (test infrastructure, no GPU needed:
tests/test_ref64_bf16_cpu.py proves on the CPU that it passes the correct fp32 emulations and refuses five subtly wrong ones,
tests/test_gemm_bf16_gpu.py applies it to the HIP kernels).

A bf16-operand result cannot be held to float64 by one flat per-point tolerance: an operand within working-precision noise of a bf16
rounding boundary rounds the other way in any two correct implementations, and that point then moves by a whole bf16 effect.  The
reference (tests/ref64.py, quant mode) therefore records every point's ROUNDING MARGIN (distance of each of its rounded operands
to the nearest boundary, in units of that operand's measured fp32 noise: ref64.Margin), and the points are split:

  kept points (ref64.Margin.kept(THRESHOLD)): no flip allowance.  With e_k = |kernel - B64| and the yardstick e_y = |ref64(quant, fp32) - B64|
      (B64: the float64-accumulating bf16 reference), both per point and divided by the point's norm,
          rms(e_k) <= 1.5 rms(e_y)   and   max(e_k) <= 3 max(e_y)            (the fp32 suite's factors)
      where at most KEPT_LOOSE = 0.5 % of the kept points may instead fall under the left-out rule (they are taken out of e_k);
  left-out points: every one within 1.0 x the tensor's largest per-point bf16 effect  max_p |B64 - float64|;
  all judged points: at most LOOSE_FWD = 2 % (forward) / LOOSE_BWD = 5 % (backward) may exceed the fp32 bound 3 max(e_y).

THRESHOLD comes from the reference alone: the smallest value of LADDER at which both correct fp32 emulations (natural and permuted
summation order) stay within the kept-point gate for every kernel family, while every family keeps at least MIN_SHARE of its judged
points and MIN_KEPT points (tests/test_ref64_bf16_cpu.py::test_threshold_is_the_smallest_of_the_ladder_that_holds)."""
import torch

from gate64 import fwd_norm, per_point        # noqa: F401  (fwd_norm: the suites take the forward norm from here)

LADDER = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0, 300.0)
THRESHOLD = 3.0
KEPT_LOOSE, LOOSE_FWD, LOOSE_BWD = 0.005, 0.02, 0.05
MIN_SHARE, MIN_KEPT = 0.10, 400
REPORT = []


def gate(what, got, b64, y32, f64, norm, margin, backward, keep=None, failures=None, threshold=None, quiet=False, second=None):
    """got: the result under test; b64 / y32 / f64: the float64-accumulating bf16 reference, the fp32-accumulating one and plain
    float64; norm [P]: what a point's error is divided by (rows with norm 0 must be exactly 0 in ``got`` and are left out);
    margin: the ref64.Margin of the references; keep: rows to judge at all (colour kernels: off the ReLU kinks).
    second: a second, equally valid fp32 yardstick (the other summation order): the quantity is then judged against the larger of the
    two rms(e_y) and, independently, the larger of the two max(e_y) -- gate64.gate's kernel_order rule.  The per-point weight
    gradients need it: there the two correct fp32 emulations refuse EACH OTHER under one yardstick (coarse, g_sdf alone: rms ratio 1.58
    on dW0 against the limit 1.5; tests/test_ref64_bf16_cpu.py)."""
    threshold = THRESHOLD if threshold is None else threshold
    got, b64, y32, f64 = (t.reshape(t.shape[0], -1).double() for t in (got, b64, y32, f64))
    zero = norm == 0
    r = dict(what=what, ok=False)
    if bool(zero.any()) and not bool((got[zero] == 0).all()):
        r["why"] = "a point with all-zero cotangents has a non-zero output"
        return _done(r, failures, quiet)
    judged = ~zero if keep is None else (~zero & keep)
    nz = norm.clone().double()
    nz[zero] = 1
    e_k, e_y, eff = per_point(got - b64, nz), per_point(y32 - b64, nz), per_point(b64 - f64, nz)
    kept = judged & margin.kept(threshold)
    n_j, n_k = int(judged.sum()), int(kept.sum())
    r.update(n=n_j, kept=n_k / max(n_j, 1))
    if n_k < MIN_KEPT or n_k < MIN_SHARE * n_j:
        r["why"] = f"only {n_k} of {n_j} judged points kept"
        return _done(r, failures, quiet)
    rms = lambda e: float((e ** 2).mean().sqrt()) if e.numel() else 0.0
    bound = 3.0 * float(e_y[kept].max())                                  # "the fp32 bound" of this tensor
    rms_y = rms(e_y[kept])
    if second is not None:
        e_2 = per_point(second.reshape(second.shape[0], -1).double() - b64, nz)
        bound, rms_y = max(bound, 3.0 * float(e_2[kept].max())), max(rms_y, rms(e_2[kept]))
    effect = max(float(eff[judged].max()), bound)
    moved = kept & ~(e_k <= bound)                                        # kept points that claim the left-out rule (NaN included)
    strict = kept & ~moved
    loose = judged & ~(e_k <= bound)
    flips = e_k[loose]
    r.update(rms_k=rms(e_k[strict]), rms_y=rms_y, max_k=float(e_k[strict].max()) if bool(strict.any()) else 0.0,
             max_y=bound / 3.0, moved=int(moved.sum()) / n_k, loose=int(loose.sum()) / n_j,
             flip=(float(flips.max()) / effect if flips.numel() else 0.0), effect=effect,
             finite=bool(torch.isfinite(got[judged]).all()))
    cap = LOOSE_BWD if backward else LOOSE_FWD
    why = []
    if not r["finite"]:
        why.append("non-finite output")
    if r["rms_k"] > 1.5 * r["rms_y"]:
        why.append("kept points: rms")
    if r["moved"] > KEPT_LOOSE:
        why.append(f"kept points: {int(moved.sum())} of {n_k} beyond 3 max(e_y)")
    if not r["flip"] <= 1.0:
        why.append("a point beyond the largest bf16 effect")
    if r["loose"] > cap:
        why.append(f"{int(loose.sum())} of {n_j} points beyond the fp32 bound")
    r["ok"], r["why"] = not why, "; ".join(why)
    return _done(r, failures, quiet)


def _done(r, failures, quiet):
    REPORT.append(r)
    if not quiet:
        print(line(r))
    if failures is not None and not r["ok"]:
        failures.append(r)
    return r["ok"]


def line(r):
    if "rms_k" not in r:
        return f"  {r['what']:<60s} FAIL ({r.get('why')})"
    return (f"  {r['what']:<60s} n={r['n']:5d}  e_k rms {r['rms_k']:.2e} max {r['max_k']:.2e}   e_y rms {r['rms_y']:.2e} max {r['max_y']:.2e}"
            f"   kept {r['kept']:.3f}  loose {r['loose']:.4f}  flip/effect {r['flip']:.2f}  {'ok' if r['ok'] else 'FAIL (' + r['why'] + ')'}")
