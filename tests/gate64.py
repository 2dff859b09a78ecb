"""The float64 gate of every "hold X to float64" suite (test infrastructure, pure torch: tests/test_gate64_cpu.py holds it on the CPU).

Per row (point, ray, image, table row, element block): e_k = |kernel - float64| and e_32 = |fp32 yardstick - float64|, both divided by
the row's norm (a backward output: the row's cotangent scale; a forward output: fwd_norm of the float64 output).  A quantity passes if
    rms(e_k) <= 1.5 rms(e_32)   and   max(e_k) <= 3 max(e_32)   and every judged row of the kernel output is finite.
A row whose norm is 0 (all-zero cotangents) must be exactly 0 in the kernel output and is left out.  Where the kernel's documented
operation order is a second, equally valid fp32 evaluation (``kernel_order``), the quantity is judged against the larger of the two
yardsticks' rms and, independently, the larger of their maxima.  A gate over one or three rows is a coin toss between two correctly
rounded results: Pool gathers the rows of a quantity over several cases and judges them once."""
import torch


def per_point(e, norm):
    return e.reshape(e.shape[0], -1).double().norm(dim=1) / norm


def fwd_norm(ref):
    return ref.detach().reshape(ref.shape[0], -1).double().norm(dim=1).clamp_min(1.0)


def _rms(e):
    return float((e ** 2).mean().sqrt())


def gate(what, got, ref, y32, norm, keep=None, failures=None, kernel_order=None):
    """per-row errors of kernel (got) and yardstick (y32) against float64 (ref), divided by norm [P]; rows with norm 0 must be
    exactly 0 in the kernel output and are left out; keep: rows to judge; kernel_order: a second fp32 yardstick, in the kernel's
    documented order (the line then carries both yardsticks' figures).  Prints one line; -> ok, and the record goes to ``failures``
    if not."""
    both = (y32,) if kernel_order is None else (y32, kernel_order)
    got, ref, *both = (t.reshape(t.shape[0], -1).double() for t in (got, ref, *both))
    zero = norm == 0
    if bool(zero.any()):
        assert bool((got[zero] == 0).all()), f"{what}: a point with all-zero cotangents has a non-zero output"
    sel = ~zero if keep is None else (~zero & keep)
    nz = norm.clone()
    nz[zero] = 1
    e_k = per_point(got - ref, nz)[sel]
    e_y = [per_point(y - ref, nz)[sel] for y in both]
    finite = bool(torch.isfinite(got[sel]).all())
    r = dict(what=what, n=int(sel.sum()), rms_k=_rms(e_k), rms_32=max(_rms(e) for e in e_y), max_k=float(e_k.max()),
             max_32=max(float(e.max()) for e in e_y), finite=finite)
    r["ok"] = ok = finite and r["rms_k"] <= 1.5 * r["rms_32"] and r["max_k"] <= 3.0 * r["max_32"]
    line = (f"  {what:<58s} n={r['n']:6d}  e_k rms {r['rms_k']:.2e} max {r['max_k']:.2e}   e_32 rms {r['rms_32']:.2e} "
            f"max {r['max_32']:.2e}  {'ok' if ok else 'FAIL'}")
    if kernel_order is not None:
        (e_r, e_o) = e_y
        line += (f"   (e_32 reference order rms {_rms(e_r):.2e} max {float(e_r.max()):.2e}, kernel order rms "
                 f"{_rms(e_o):.2e} max {float(e_o.max()):.2e})")
    print(line)
    if failures is not None and not ok:
        failures.append(r)
    return ok


def report(what, got, ref, y32, norm, keep):
    """a line in gate's format WITHOUT a verdict, for a quantity that no fp32 evaluation determines (rounding noise on both sides)"""
    got, ref, y32 = (t.detach().cpu().reshape(t.shape[0], -1).double() for t in (got, ref, y32))
    e_k, e_32 = per_point(got - ref, norm)[keep], per_point(y32 - ref, norm)[keep]
    print(f"  {what:<58s} n={int(keep.sum()):6d}  e_k rms {_rms(e_k):.2e} max {float(e_k.max()):.2e}   e_32 rms {_rms(e_32):.2e} "
          f"max {float(e_32.max()):.2e}  reported, not gated")


class Pool:
    """rows of one quantity gathered over several cases (padded to a common width with zeros on all three sides), judged once"""

    def __init__(self):
        self.rows = {}

    def add(self, what, got, ref, y32, norm, keep=None, kernel_order=None):
        """kernel_order: a second fp32 yardstick in the kernel's documented operation order; a quantity that has one in any of its
        cases is gated against the larger of the two yardsticks' errors (a case without one counts its only yardstick twice)"""
        P = got.shape[0]
        flat = [t.detach().cpu().reshape(P, -1).double() for t in (got, ref, y32, y32 if kernel_order is None else kernel_order)]
        keep = torch.ones(P, dtype=torch.bool) if keep is None else keep
        self.rows.setdefault(what, []).append((flat, norm.double(), keep, kernel_order is not None))

    def judge(self, prefix, failures):
        for what, items in self.rows.items():
            width = max(f[0].shape[1] for f, _n, _k, _a in items)
            pad = lambda t: torch.nn.functional.pad(t, (0, width - t.shape[1]))
            got, ref, y32, alt = (torch.cat([pad(f[i]) for f, _n, _k, _a in items]) for i in range(4))
            norm, keep = torch.cat([n for _f, n, _k, _a in items]), torch.cat([k for _f, _n, k, _a in items])
            gate(prefix + what, got, ref, y32, norm, keep, failures, alt if any(a for _f, _n, _k, a in items) else None)
