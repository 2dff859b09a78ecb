"""tests/gate64.py on synthetic tensors of 64 rows (no GPU): the reference is 0 and every error a small multiple of a power of two,
so each ratio below is exact and a boundary can be met with equality.  What the "hold X to float64" GPU suites rely on: the factors
1.5 (rms) and 3 (max), each judged on its own; zero-norm rows exactly 0 and left out; every judged row finite; the second yardstick
raising the rms bound and the max bound independently; Pool judging the padded concatenation; and the printed lines, which DESIGN.md
section 7 quotes, byte for byte those of the gate before it had a module of its own."""
import pytest
import torch

import gate64 as G

N = 64
Y = 2.0 ** -20                                  # the yardstick's error in every row unless a test says otherwise
ABOVE = 1.0 + 2.0 ** -30                        # "just above": a million ulps, far from any rounding of the gate's own arithmetic
REF = torch.zeros(N, 1, dtype=torch.float64)
ONES = torch.ones(N, dtype=torch.float64)


def rows(value=0.0, **at):
    """[N, 1] of ``value`` with single rows set: rows(r5=1.0)"""
    t = torch.full((N, 1), value, dtype=torch.float64)
    for k, v in at.items():
        t[int(k[1:])] = v
    return t


def judged(got, y32=None, norm=ONES, **kw):
    """-> (ok, the failure record or None)"""
    fails = []
    ok = G.gate("q", got, REF, rows(Y) if y32 is None else y32, norm, failures=fails, **kw)
    assert ok == (not fails)
    return ok, (fails[0] if fails else None)


def test_rms_boundary():
    assert judged(rows(1.5 * Y))[0]
    ok, r = judged(rows(1.5 * Y * ABOVE))
    assert not ok and r["rms_k"] > 1.5 * r["rms_32"] and r["max_k"] <= 3.0 * r["max_32"]


def test_max_boundary_with_the_rms_condition_met():
    assert judged(rows(r9=3.0 * Y))[0]
    ok, r = judged(rows(r9=3.0 * Y * ABOVE))
    assert not ok and r["max_k"] > 3.0 * r["max_32"] and r["rms_k"] <= 1.5 * r["rms_32"] and r["finite"]
    assert r["rms_k"] == 3.0 * Y * ABOVE / 8                               # one row of 64: rms = value / 8


def test_zero_norm_rows_must_be_exactly_zero_and_are_left_out(capsys):
    norm = ONES.clone()
    norm[5] = 0.0
    with pytest.raises(AssertionError, match="non-zero output"):
        G.gate("q", rows(r5=2.0 ** -140), REF, rows(Y), norm)
    assert G.gate("q", rows(Y), REF, rows(Y), ONES) and " n=    64 " in capsys.readouterr().out
    assert G.gate("q", rows(Y, r5=0.0), REF, rows(Y), norm) and " n=    63 " in capsys.readouterr().out
    # the row is left out on the yardstick's side as well: its error of 1 there would carry any kernel error past both bounds
    assert not G.gate("q", rows(1.5 * Y * ABOVE, r5=0.0), REF, rows(Y, r5=1.0), norm)


def test_non_finite_values_fail_only_in_judged_rows():
    keep = torch.ones(N, dtype=torch.bool)
    keep[7] = False
    for bad in (float("nan"), float("inf")):
        ok, r = judged(rows(Y, r7=bad))
        assert not ok and not r["finite"]
        assert judged(rows(Y, r7=bad), keep=keep)[0]
    assert not judged(rows(Y, r7=float("nan")), keep=~keep)[0]


def test_two_yardsticks_give_the_rms_bound_and_the_max_bound_independently():
    y_ref, y_ker = rows(Y), rows(r3=4.0 * Y)                                # rms Y, max Y  |  rms Y / 2, max 4 Y
    got = rows(r0=12.0 * Y)                                                 # rms 1.5 Y, max 12 Y: on both bounds at once
    ok, r = judged(got, y_ref)
    assert not ok and r["max_k"] > 3.0 * r["max_32"] and r["rms_k"] <= 1.5 * r["rms_32"]
    ok, r = judged(got, y_ker)
    assert not ok and r["rms_k"] > 1.5 * r["rms_32"] and r["max_k"] <= 3.0 * r["max_32"]
    assert judged(got, y_ref, kernel_order=y_ker)[0] and judged(got, y_ker, kernel_order=y_ref)[0]
    ok, r = judged(rows(r0=12.0 * Y * ABOVE), y_ref, kernel_order=y_ker)
    assert not ok and (r["rms_32"], r["max_32"]) == (Y, 4.0 * Y)


@pytest.mark.parametrize("scale,want", [(1.0, True), (ABOVE, False)])
def test_pool_judges_the_padded_concatenation(scale, want, capsys):
    """two cases of widths 1 and 3 (24 and 40 rows): one row of the wide case on the max bound (its three columns 1, 2, 2 x Y:
    norm 3 Y), the pool's verdict and line are gate's on the zero-padded [64, 3]"""
    a, b = (torch.zeros(24, 1, dtype=torch.float64), torch.zeros(40, 3, dtype=torch.float64))
    b[11] = torch.tensor([1.0, 2.0, 2.0], dtype=torch.float64) * Y * scale
    ya, yb = torch.full((24, 1), Y, dtype=torch.float64), torch.zeros(40, 3, dtype=torch.float64)
    yb[:, 1] = Y
    pool, fails = G.Pool(), []
    pool.add("q", a, torch.zeros_like(a), ya, torch.ones(24))
    pool.add("q", b, torch.zeros_like(b), yb, torch.ones(40))
    pool.judge("pooled: ", fails)
    line = capsys.readouterr().out
    pad = lambda t: torch.nn.functional.pad(t, (0, 3 - t.shape[1]))
    direct = []
    ok = G.gate("pooled: q", torch.cat([pad(a), b]), torch.zeros(N, 3, dtype=torch.float64), torch.cat([pad(ya), yb]), ONES, failures=direct)
    assert ok == want == (not fails) and fails == direct
    assert line == capsys.readouterr().out and " n=    64 " in line


def fixed():
    """an input with every feature at once: three columns, row norms 2^-3 .. 2^3, four zero-norm rows, a keep mask"""
    i = torch.arange(N, dtype=torch.float64)
    cols = lambda *c: torch.stack(c, 1)
    ref = cols((i * 37) % 11 - 5, (i * 17) % 7 - 3, (i * 5) % 13 - 6)
    y32 = ref + 2.0 ** -22 * cols((i * 3) % 5 - 2, (i * 7) % 3 - 1, i % 4 - 1.5)
    yker = ref + 2.0 ** -22 * cols((i * 11) % 7 - 3, i % 5 - 2, (i * 13) % 4 - 1.5)
    got = ref + 2.0 ** -22 * cols((i * 19) % 9 - 4, (i * 23) % 5 - 2, (i * 29) % 6 - 2.5)
    full = torch.exp2(i % 7 - 3)
    norm = full.clone()
    norm[::16] = 0.0
    got[::16] = 0.0
    mild = ref + 0.25 * (got - ref)
    mild[::16] = 0.0
    return dict(got=got.float(), mild=mild.float(), ref=ref, y32=y32.float(), yker=yker.float(), norm=norm, full=full, keep=i % 5 != 0)


# recorded from the gate, gate_larger and report of the commit before this module existed, on fixed()
LINES = """\
  one yardstick, all rows                                    n=    60  e_k rms 6.29e-07 max 2.70e-06   e_32 rms 1.77e-06 max 5.72e-06  ok
  one yardstick: kept rows of a quantity with a long name that runs past the column n=    48  e_k rms 2.78e-06 max 8.53e-06   e_32 rms 1.75e-06 max 5.72e-06  FAIL
  one yardstick, failing                                     n=    48  e_k rms 1.01e-05 max 2.98e-05   e_32 rms 1.75e-06 max 5.72e-06  FAIL
  two yardsticks                                             n=    48  e_k rms 2.78e-06 max 8.53e-06   e_32 rms 3.05e-06 max 8.74e-06  ok   (e_32 reference order rms 1.75e-06 max 5.72e-06, kernel order rms 3.05e-06 max 8.74e-06)
  two yardsticks, failing                                    n=    48  e_k rms 1.01e-05 max 2.98e-05   e_32 rms 3.05e-06 max 8.74e-06  FAIL   (e_32 reference order rms 1.75e-06 max 5.72e-06, kernel order rms 3.05e-06 max 8.74e-06)
  a report                                                   n=    48  e_k rms 2.78e-06 max 8.53e-06   e_32 rms 1.75e-06 max 5.72e-06  reported, not gated
"""


def test_printed_lines_are_those_of_the_gate_before_it_moved(capsys):
    f = fixed()
    G.gate("one yardstick, all rows", f["mild"], f["ref"], f["y32"], f["norm"])
    G.gate("one yardstick: kept rows of a quantity with a long name that runs past the column", f["got"], f["ref"], f["y32"], f["norm"], f["keep"])
    G.gate("one yardstick, failing", f["got"] * 1.0000005, f["ref"], f["y32"], f["norm"], f["keep"], [])
    G.gate("two yardsticks", f["got"], f["ref"], f["y32"], f["norm"], f["keep"], [], kernel_order=f["yker"])
    G.gate("two yardsticks, failing", f["got"] * 1.0000005, f["ref"], f["y32"], f["norm"], f["keep"], [], kernel_order=f["yker"])
    G.report("a report", f["got"], f["ref"], f["y32"], f["full"], f["keep"] & (f["norm"] != 0))
    assert capsys.readouterr().out == LINES
