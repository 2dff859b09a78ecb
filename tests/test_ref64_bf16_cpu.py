"""The bf16-operand mode of tests/ref64.py and the gate of tests/bf16_gate.py, on the CPU (no GPU needed).

(1) ref64(quant, fp32) is oracle/render_ref.py with mlp_precision = "bf16" / "bf16_colour" on the same points: forward and
    backward, both SDF networks and the colour network; kept points to the fp32 bound, the rest within the flip bound.
(2) The gate bites: four deliberately wrong emulations (ref64.FAULTS: weights truncated instead of rounded, the cotangent operand of
    the derivative GEMMs left unrounded, one 8-wide operand group taken from the neighbouring point at every 16th point, the sdf row
    rounded like the others) fail it; the two correct fp32 emulations (natural and permuted summation order) pass it, on every
    kernel family of tests/test_gemm_bf16_gpu.py (tests/bf16_cases.py::all_cases, N = 4 123 points).
(3) The margin threshold is fixed against the reference alone: bf16_gate.THRESHOLD is the smallest value of bf16_gate.LADDER at
    which both correct emulations stay within the gate for every family while every family keeps >= 10 % of its judged points and
    >= 400 points.
(4) The same on the PER-POINT WEIGHT GRADIENTS (tests/bf16_cases.py::weight_grad_cases: what the emission rows of the _params twins
    encode), judged with both fp32 summation orders as yardsticks (bf16_gate.gate, ``second``): a third correct emulation passes in
    every layer of every family of both SDF networks and the colour network; under ONE yardstick the correct emulations refuse each
    other (coarse, g_sdf alone: dW0); "truncated weights", "unrounded cotangents" and "rounded emission rows" (g (x) x formed from
    the rounded vectors: the oracle's _LinQ, which the MAP bodies by design do not do) are refused in at least one layer of every
    family they reach.

MEASURED (this module; full_vis_eval with every weight_v perturbed by 0.05; margin in units of the operand's measured fp32 noise,
ref64.Margin).  Both correct emulations within the gate on every family: only at THRESHOLD = 3 of the ladder 1e-4, 3e-4, ..., 300 --
at 1 and below rounding flips remain among the kept points (e.g. sdf backward fine, all three: e_y max 4.9e-2 c_p against 1.0e-4 at
3), at 10 and above the g_grad-alone families keep fewer than 400 points (fine: 77).  Kept at 3, of 4 123 points per family:
  sdf forward coarse / fine / pair                 3660 (0.89) / 2809 (0.68) / 2509 (0.61)
  sdf backward coarse: all three / g_sdf / g_feat / g_grad alone / independent scales / g_sdf 2^20..2^40 / c_p in [1/8, 8]
                                                   3172 (0.77) / 3396 (0.82) / 3380 (0.82) / 972 (0.24) / 2689 (0.65) / 3446 (0.84) / 3217 (0.78)
  sdf backward fine:   the same families           1634 (0.40) / 2285 (0.55) / 2225 (0.54) / 476 (0.12) / 1470 (0.36) / 2332 (0.57) / 1679 (0.41)
  colour forward / backward / colour + coarse backward   4023 (0.98) / 3917 (0.95) / 3146 (0.76)
In units of the operand's own bf16 spacing (Quant.margin) a threshold of 1e-3 keeps 0.16 of the fine backward's points and leaves
flips of 5e-3 c_p among them; in units of the measured noise the kept points of an fp32 emulation that is not one of the noise
samples agree with the reference to 1.0e-4 c_p (rms 1.7e-5) there and to 3e-7 of the output's norm in the forwards.
"""
import copy

import pytest
import torch

import bf16_cases as C
import bf16_gate as G
import gemm_cases
import ref64
from oracle import render_ref as R
from mlp_calls import perturbed


@pytest.fixture(scope="module")
def model():
    _fx, cfg, params = perturbed()
    return params, cfg


@pytest.fixture(scope="module")
def judged(model):
    """name -> (case, references, a permuted-order emulation that is NOT one of the margin's noise samples, norm, backward?, keep):
    computed once for (2) and (3)"""
    params, cfg = model
    out = {}
    for name, (call, norm, backward, colour) in C.all_cases(params, cfg).items():
        r = C.refs(call)
        out[name] = (call, r, C.emulate(call, order=("permuted", 1)), norm, backward, C.kink_keep(r) if colour else None)
    return out


def _gate_case(name, entry, got, threshold=None, quiet=True):
    """every output tensor of one case through the gate -> all ok?"""
    _call, r, _perm, norm, backward, keep = entry
    ok = True
    for k in r.b64:
        n = G.fwd_norm(r.b64[k]) if norm is None else norm
        ok &= G.gate(f"{name}: {k}", got[k], r.b64[k], r.y32[k], r.f64[k], n, r.margin, backward, keep, threshold=threshold, quiet=quiet)
    return ok


# ------------------------------------------------------------------------------------------------------------------ (1) the oracle
def _hold_to_oracle(what, theirs, r, k, keep=None):
    """ref64(quant, fp32) against the oracle: kept points to the fp32 bound (tests/test_ref64_cpu.py::_close), the rest within the
    largest bf16 effect of the tensor"""
    a, b, b64, f64 = (t.detach().double().reshape(t.shape[0], -1) for t in (r.y32[k], theirs, r.b64[k], r.f64[k]))
    keep = torch.ones(a.shape[0], dtype=torch.bool) if keep is None else keep
    scale = b.abs().amax(1, keepdim=True).clamp_min(1e-3 * float(b.abs().max()))
    err = ((a - b).abs() / scale).amax(1)
    kept = r.margin.kept(G.THRESHOLD) & keep
    assert int(kept.sum()) >= 0.1 * a.shape[0], f"{what}: {int(kept.sum())} points kept"
    assert float(err[kept].max()) <= 2e-5, f"{what}: kept points {float(err[kept].max()):.2e}"
    effect = float(((b64 - f64).abs() / scale)[keep].max())
    assert float(err[keep].max()) <= max(effect, 2e-5), f"{what}: {float(err[keep].max()):.2e} beyond the bf16 effect {effect:.2e}"


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_quant_sdf_networks_equal_the_bf16_oracle_in_fp32(model, which):
    params, cfg = model
    n = 1500
    x = gemm_cases.cube_points(n, 3)
    nets, prefix = (which,), ref64.NETS[which]
    xs = x.clone()
    so, fo, go = R._net_outputs(params, prefix, getattr(cfg, which), xs, True)
    r = C.refs(C.sdf_forward_case(params, cfg, x, nets))
    for k, o in zip(("sdf", "grad", "feat"), (so[:, 0], go, fo)):
        _hold_to_oracle(f"{which} {k}", o, r, k)
    cot = (gemm_cases.cot(n, 4, ()), gemm_cases.cot(n, 5, (64,)), gemm_cases.cot(n, 6, (3,)))
    for use in ((0, 1, 2), (0,), (1,), (2,)):
        g = [c if i in use else None for i, c in enumerate(cot)]
        (theirs,) = torch.autograd.grad(sum((c * y).sum() for c, y in zip(g, (so[:, 0], fo, go)) if c is not None), xs, retain_graph=True)
        _hold_to_oracle(f"{which} d/dx of cotangents {use}", theirs, C.refs(C.sdf_backward_case(params, cfg, x, nets, *g)), "x")


@pytest.mark.parametrize("precision", ["bf16", "bf16_colour"])
@pytest.mark.parametrize("grid_grad", [0, 1])
def test_quant_colour_network_equals_the_bf16_oracle_in_fp32(model, precision, grid_grad):
    params, cfg = model
    cq = copy.copy(cfg)
    cq.mlp_precision = precision                       # (the colour network is the same in both modes)
    n = 1500
    i = C.inputs(params, cfg, n)
    x, d, normals, feat = i.x, i.d, i.normals, i.feat
    g_rgb = gemm_cases.cot(n, 7, (3,))
    ins = [t.clone().requires_grad_(True) for t in (x, normals, d, feat)]
    rgb_o = R.colour_net(params, cq, *ins, color_stage="highfreq" if grid_grad else "base")
    _hold_to_oracle("rgb", rgb_o, C.refs(C.colour_forward_case(params, cfg, x, d, normals, feat)), "rgb")
    theirs = torch.autograd.grad((g_rgb * rgb_o).sum(), ins)
    r = C.refs(C.colour_backward_case(params, cfg, x, d, normals, feat, g_rgb, grid_grad))
    keep = r.relu_margin >= 1e-5                       # (the ReLU kinks: masks decided by rounding, as tests/test_ref64_cpu.py)
    assert int((~keep).sum()) <= n // 100
    for k, o in zip(("x", "normals", "dirs", "feat"), theirs):
        _hold_to_oracle(f"d/d {k}", o, r, k, keep)


def test_rounding_is_one_rounding_to_nearest_even_and_the_margin_is_the_distance_to_the_boundary():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -30, 0.0, -3.0e-5, 1.0 + 2.0 ** -9], dtype=torch.float64)
    r, m = ref64.rne_bf16(x)
    # ties to even: 1 + 2^-8 -> 1, 1 + 3 x 2^-8 -> 1 + 2^-6; just above a tie (invisible in fp32): up
    assert r.tolist()[:5] == [1.0, 1.0, 1.015625, 1.0078125, 0.0]
    assert m.tolist()[:2] == [0.5, 0.0] and m[4] == 0.5 and abs(float(m[3]) - 2.0 ** -23) < 1e-12 and m[6] == 0.25
    y = torch.randn(4096, dtype=torch.float32) * 3
    assert torch.equal(ref64.rne_bf16(y)[0], y.to(torch.bfloat16).float())


# ------------------------------------------------------------------------------------------------------------------ (2) the gate bites
def test_both_correct_emulations_pass_the_gate_on_every_family(judged, capsys):
    G.REPORT.clear()
    bad = []
    with capsys.disabled():
        print()
        for name, entry in judged.items():
            for label, got in (("natural", entry[1].y32), ("permuted", entry[1].perm), ("permuted, other order", entry[2])):
                if not _gate_case(f"[{label}] {name}", entry, got, quiet=(label != "permuted, other order")):
                    bad.append((label, name))
    assert not bad, bad


FAULT_CASES = {"truncated weights": ("sdf forward fine", "sdf backward fine: all three x c_p", "colour forward"),
               "unrounded cotangents": ("sdf forward fine", "sdf backward coarse: all three x c_p", "colour backward grid_grad 1"),
               "neighbour's operand group": ("sdf forward fine", "sdf backward fine: g_feat alone x c_p", "colour forward"),
               "rounded sdf row": ("sdf forward coarse", "sdf forward pair", "sdf backward fine: g_sdf alone x c_p")}


@pytest.mark.parametrize("fault", ref64.FAULTS)
def test_a_subtly_wrong_emulation_fails_the_gate(judged, fault, capsys):
    with capsys.disabled():
        print()
        for name in FAULT_CASES[fault]:
            entry = judged[name]
            assert not _gate_case(f"[{fault}] {name}", entry, C.emulate(entry[0], fault=fault), quiet=False), \
                f"the gate accepts '{fault}' on {name}"


# ------------------------------------------------------------------------------------------------------------------ (3) the threshold
def test_threshold_is_the_smallest_of_the_ladder_that_holds(judged, capsys):
    holds = {}
    for t in G.LADDER:
        holds[t] = all(_gate_case(name, entry, got, threshold=t) for name, entry in judged.items() for got in (entry[1].y32, entry[1].perm, entry[2]))
    shares = {name: float((entry[1].margin.kept(G.THRESHOLD) & (entry[5] if entry[5] is not None else True) &
                           ((entry[3] != 0) if entry[3] is not None else True)).double().sum()) for name, entry in judged.items()}
    with capsys.disabled():
        print("\n  ladder -> both correct emulations within the gate on every family:", holds)
        for name, n in shares.items():
            print(f"  {name:<64s} kept {int(n):5d} = {n / C.N:.3f} of {C.N}")
    assert G.THRESHOLD == min(t for t in G.LADDER if holds[t]), holds
    for name, n in shares.items():
        assert n >= G.MIN_KEPT and n >= G.MIN_SHARE * C.N, (name, n)


# ------------------------------------------------------------------------------------------------------------------ (4) weight gradients
WEIGHT_GRAD_FAULTS = ("truncated weights", "unrounded cotangents", "rounded emission rows")


@pytest.fixture(scope="module")
def weight_grad_cases(model):
    params, cfg = model
    return C.weight_grad_cases(params, cfg)


def _layers_ok(r, got, norm, keep, second, what=None):
    """layer -> does ``got`` pass the backward gate there? (second: both summation orders as yardsticks)"""
    return {k: G.gate(f"{what}: {k}", got[k], r.b64[k], r.y32[k], r.f64[k], norm, r.margin, True, keep, quiet=what is None,
                      second=r.perm[k] if second else None) for k in r.b64 if k.startswith("[dW")}


@pytest.mark.parametrize("network", ["coarse", "fine", "colour"])
def test_weight_gradient_gate_passes_the_correct_emulations_and_refuses_the_wrong_ones(weight_grad_cases, network, capsys):
    """MEASURED (N = 4 123, both yardsticks): the third emulation passes everywhere; "truncated weights" is refused in every layer of
    every family; "rounded emission rows" in dW0 of every family; "unrounded cotangents" wherever a feature or gradient cotangent is
    present, in the fine network also with g_sdf alone (dW0, dW1) -- in the coarse network with g_sdf alone it does not reach the
    weight gradients at all (the only derivative GEMM there is the one towards x), and the test says so instead of demanding it.
    Under one yardstick the permuted emulation is refused on dW0 of coarse "g_sdf alone" (the reason for ``second``)."""
    single_refusals = []
    with capsys.disabled():
        print()
        for name, (call, norm, _backward, colour) in weight_grad_cases.items():
            if not name.startswith(f"weight gradients {network}"):
                continue
            r = C.refs(call)
            keep = C.kink_keep(r) if colour else None
            kept = r.margin.kept(G.THRESHOLD) & (norm != 0) & (keep if keep is not None else True)
            assert int(kept.sum()) >= G.MIN_KEPT, (name, int(kept.sum()))
            third = C.emulate(call, order=("permuted", 1))
            for label, got in (("natural", r.y32), ("permuted", r.perm), ("permuted, other order", third)):
                ok = _layers_ok(r, got, norm, keep, True, f"[{label}] {name}" if got is third else None)
                assert all(ok.values()), f"the gate refuses the correct emulation '{label}' on {name}: {ok}"
                if not all(_layers_ok(r, got, norm, keep, False).values()):
                    single_refusals.append((label, name))
            for k in r.b64:                                  # the value path as a forward quantity
                if k.startswith("H"):
                    assert G.gate(f"{name}: {k}", third[k], r.b64[k], r.y32[k], r.f64[k], G.fwd_norm(r.b64[k]), r.margin, False, keep, quiet=True)
            for fault in WEIGHT_GRAD_FAULTS:
                wrong = C.emulate(call, fault=fault)
                reached = any(not torch.equal(wrong[k], r.y32[k]) for k in wrong if k.startswith("[dW"))
                ok = _layers_ok(r, wrong, norm, keep, True)
                print(f"  [{fault}] {name}: " + ("refused in " + ", ".join(k for k, v in ok.items() if not v) if not all(ok.values())
                                                   else "does not reach the weight gradients" if not reached else "ACCEPTED"))
                assert not reached or not all(ok.values()), f"the gate accepts '{fault}' on {name}"
                if fault != "unrounded cotangents":
                    assert reached, f"'{fault}' does not reach {name}"
            del r, third
        print(f"  under ONE yardstick a correct emulation is refused on: {single_refusals}")
    if network == "coarse":
        assert ("permuted", "weight gradients coarse: g_sdf alone x c_p") in single_refusals, "one yardstick suffices: drop bf16_gate.gate's second"


def test_second_yardstick_only_ever_loosens_towards_the_other_correct_order():
    """bf16_gate.gate(second=...): without it nothing changes; with it the rms and the bound are the larger of the two orders'"""
    g = torch.Generator().manual_seed(5)
    P = 2000
    b64 = torch.randn(P, 8, generator=g, dtype=torch.float64)
    y1, y2 = b64 + 1e-6 * torch.randn(P, 8, generator=g, dtype=torch.float64), b64 + 2e-6 * torch.randn(P, 8, generator=g, dtype=torch.float64)
    margin = type("M", (), {"kept": lambda self, t: torch.ones(P, dtype=torch.bool)})()
    norm = torch.ones(P, dtype=torch.float64)
    args = lambda got, y: (got, b64, y, b64 + 1e-3, norm, margin, True)
    G.REPORT.clear()
    assert not G.gate("y2 against y1", *args(y2, y1), quiet=True)
    assert G.gate("y2 against y1 and y2", *args(y2, y1), quiet=True, second=y2) and G.gate("y1 against both", *args(y1, y2), quiet=True, second=y1)
    one, two = G.REPORT[0], G.REPORT[1]
    assert two["rms_y"] > one["rms_y"] and two["max_y"] > one["max_y"] and abs(two["rms_y"] / one["rms_y"] - 2) < 0.2
    assert not G.gate("3 x y2 against both", *args(b64 + 3.2 * (y2 - b64), y1), quiet=True, second=y2)
