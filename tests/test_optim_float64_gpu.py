"""The kernels that turn gradients into parameters against float64 (tests/optim_ref64.py), through the C ABI: the nine launch forms of
Adam (csrc/map_tail.hip: nsa_adam_table_step / _clear / _zero_grad in their float4, scalar and non-temporal forms, nsa_adam_multi_step;
csrc/track_tail.hip: nsa_adam_step / _scaled and the steps inside nsa_track_tail and nsa_track_finish), nicer_slam_amd.optim.Adam itself,
the tracker's two reductions, the flat weight norm and its backward, and -- exactly -- the voxel counter and the Morton keys.

The method is tests/test_gemm_float64_gpu.py's, the gate tests/gate64.py: e_k = |kernel - float64|, e_32 = |fp32 yardstick - float64|, per element
(or per row) divided by a norm taken from the float64 side; rms(e_k) <= 1.5 rms(e_32) and max(e_k) <= 3 max(e_32), everything finite.
Adam is judged class by class (tests/optim_cases.py: typical, untouched row, never touched, eps regime, subnormal, large, cancelling): the
kernels of map_tail.hip against the fp32 order documented above their adam_one, the camera kernels of track_tail.hip against the larger of
that order and their own documented one (gate64.gate with kernel_order); the norms are max(|m0|, |g|), max(v0, v64) and max(|p0|, |p64 - p0|).  Class C is held to equality.  Class E's moments are reported, not gated.

Every buffer a kernel may write (and every gradient it reads) lies between 8 sentinel floats on either side that must come back bit for bit.
tests/test_optim_ref64_cpu.py holds the references to torch and shows that the classes catch fourteen mutants.
Measured on MI355X: DESIGN.md section 7 holds the printed summary."""
import ctypes
import time

import numpy as np
import pytest
import torch

import objective_cases as OC
import optim_cases as C
import optim_ref64 as R
from devcall import st
from gate64 import Pool

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
PAD = 8
SENTINEL = 0x4B3C2D1E
NSA_OK, NSA_EBADARG = 0, 4


def _lib():
    from nicer_slam_amd._native import lib
    return lib


class Buf:
    """n elements on the device between PAD sentinel words on either side; shift = 1 moves the view off the 16-byte grid by one float"""

    def __init__(self, data=None, n=None, shift=0, dtype=torch.float32, fill=None):
        self.n = int(data.numel() if data is not None else n)
        self.lo = PAD + shift
        self.words = torch.full((self.lo + self.n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.t = self.words[self.lo:self.lo + self.n].view(dtype)
        if data is not None:
            self.t.copy_(data.reshape(-1).to(dtype))
        elif fill is not None:
            self.t.fill_(fill)
        assert self.words.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        return self.t.cpu()

    def intact(self):
        return bool((self.words[:self.lo] == SENTINEL).all()) and bool((self.words[self.lo + self.n:] == SENTINEL).all())


def _intact(what, *bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b.intact(), f"{what}: the words around buffer {i} changed"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _refs(case, t, hyper, lr_step=0, gamma=1.0, g64=None, camera=False):
    """-> (float64, fp32 yardstick, second fp32 yardstick).  The kernels of map_tail.hip have ONE yardstick, the order documented above
    their adam_one (handed over twice: the two-yardstick gate is then the plain one); camera=True (k_adam and the steps inside the tracker tails)
    adds the order documented in track_tail.hip, and the larger error counts."""
    b1, b2, eps, lr = hyper
    a = (case["m0"], case["v0"], t, lr, b1, b2, eps, lr_step, gamma)
    g = case["g"]
    y_table = R.adam_step(case["p0"], g, *a, dtype=F32)
    return (R.adam_step(case["p0"], g if g64 is None else g64, *a), y_table,
            R.adam_step(case["p0"], g, *a, dtype=F32, order="camera") if camera else y_table)


def _judge(failures):
    return C.AdamJudge(failures)


def _finish(judge, tag, capsys):
    """the pooled gates (their lines stay captured, like every single gate's), then the summary, shown"""
    lines = judge.finish(tag)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------------------------ table forms
FORMS = {"step": "nsa_adam_table_step", "clear": "nsa_adam_table_step_clear", "zero_grad": "nsa_adam_table_step_zero_grad"}


def run_table(form, case, t, hyper, shift=(0, 0, 0, 0), what=""):
    """-> (m, v, p) on the CPU; the sentinels, the gradient's fate (untouched / cleared) and the return code are asserted"""
    b1, b2, eps, lr = hyper
    p, g, m, v = (Buf(case[k], shift=s) for k, s in zip(("p0", "g", "m0", "v0"), shift))
    if form == "zero_grad":
        assert not bool(case["g"].any())
        rc = _lib().nsa_adam_table_step_zero_grad(p.ptr, m.ptr, v.ptr, case["n"], t, lr, b1, b2, eps, st())
    else:
        rc = getattr(_lib(), FORMS[form])(p.ptr, g.ptr, m.ptr, v.ptr, case["n"], t, lr, b1, b2, eps, st())
    assert rc == NSA_OK, (what, rc)
    _intact(what, p, g, m, v)
    if form == "clear":
        assert not bool(g.t.any()), f"{what}: the consumed gradient does not read zero everywhere"
    else:
        assert torch.equal(_bits(g.cpu()), _bits(case["g"])), f"{what}: the gradient changed"
    return m.cpu(), v.cpu(), p.cpu()


def _check_lr0(name, case, got):
    if name == "lr=0":                             # p bit for bit, while the moments move (class B: both decay, whatever the draw)
        assert torch.equal(_bits(got[2]), _bits(case["p0"]))
        b = case["cls"] == ord("B")
        assert bool((got[0][b] != case["m0"][b]).all()) and bool((got[1][b] != case["v0"][b]).all())


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(C.HYPER))
def test_table_forms_vs_float64(form, name, capsys):
    hyper = C.HYPER[name]
    classes = "BC" if form == "zero_grad" else C.CLASSES
    failures = []
    judge = _judge(failures)
    for t in C.STEPS:
        for n in C.TABLE_N:
            for rep in range(16 if n <= 5 else 1):         # (the small sizes: 16 draws each, pooled over the cases)
                case = C.adam_case(n, 1000 * t + 16 * n + rep, hyper[2], classes, b1=hyper[0])
                tag = f"{form} {name} t={t} n={n}"
                got = run_table(form, case, t, hyper, what=tag)
                judge.add(tag, case, got, *_refs(case, t, hyper))
                _check_lr0(name, case, got)
    _finish(judge, f"table {form} {name}", capsys)
    assert not failures, [f["what"] for f in failures]


SHIFTS = {"p": (1, 0, 0, 0), "g": (0, 1, 0, 0), "m": (0, 0, 1, 0), "v": (0, 0, 0, 1)}


@pytest.mark.parametrize("form", list(FORMS))
def test_scalar_forms_one_misaligned_pointer_at_a_time(form, capsys):
    """a view offset by one float in ONE of p, g, m, v takes the element-per-thread kernels; n = 2^21 + 257: the grid-stride loop's
    second trip (the grid is capped at 8192 blocks of 256)"""
    hyper = C.HYPER["project"]
    classes = "BC" if form == "zero_grad" else C.CLASSES
    failures = []
    judge = _judge(failures)
    for which, shift in SHIFTS.items():
        if form == "zero_grad" and which == "g":
            continue
        for n, t in ((1, 1), (5, 2), (1025, 7), (2051, 1000)):
            case = C.adam_case(n, 31 * n + t, hyper[2], classes, b1=hyper[0])
            tag = f"scalar {form} {which} off by a float n={n}"
            judge.add(tag, case, run_table(form, case, t, hyper, shift, tag), *_refs(case, t, hyper))
    n = (1 << 21) + 257
    case = C.adam_case(n, 5, hyper[2], classes, b1=hyper[0])
    tag = f"scalar {form} n=2^21+257"
    judge.add(tag, case, run_table(form, case, 7, hyper, (0, 0, 1, 0), tag), *_refs(case, 7, hyper))
    _finish(judge, f"scalar {form}", capsys)
    assert not failures, [f["what"] for f in failures]


def test_table_forms_bad_arguments_and_n_zero():
    lib, hyper = _lib(), C.HYPER["project"]
    b1, b2, eps, lr = hyper
    case = C.adam_case(64, 3, eps)
    bufs = [Buf(case[k]) for k in ("p0", "g", "m0", "v0")]
    p, g, m, v = (b.ptr for b in bufs)
    before = [b.words.clone() for b in bufs]
    for fn in (lib.nsa_adam_table_step, lib.nsa_adam_table_step_clear):
        assert fn(p, g, m, v, 64, 0, lr, b1, b2, eps, st()) == NSA_EBADARG              # step = 0
        for i in range(4):                                                             # a pointer off by 2 bytes
            a = [p, g, m, v]
            a[i] += 2
            assert fn(*a, 60, 1, lr, b1, b2, eps, st()) == NSA_EBADARG
        assert fn(p, g, m, v, 0, 1, lr, b1, b2, eps, st()) == NSA_OK                    # n = 0
    z = lib.nsa_adam_table_step_zero_grad
    assert z(p, m, v, 64, 0, lr, b1, b2, eps, st()) == NSA_EBADARG
    for i in range(3):
        a = [p, m, v]
        a[i] += 2
        assert z(*a, 60, 1, lr, b1, b2, eps, st()) == NSA_EBADARG
    assert z(p, m, v, 0, 1, lr, b1, b2, eps, st()) == NSA_OK
    torch.cuda.synchronize()
    for b, w in zip(bufs, before):
        assert torch.equal(b.words, w), "a refused or empty call wrote something"


# ------------------------------------------------------------------------------------------------------------------ non-temporal forms
@pytest.mark.parametrize("form", ["step", "zero_grad"])
def test_non_temporal_forms_at_2_pow_26_plus_5(form, capsys):
    """n >= 2^26 takes k_adam_table_linear_nt / k_adam_table_zero_grad<NT>.  The operands are a 2^16-element case tiled on the device;
    float64 reference and gate are evaluated there; the yardstick is the CPU's for the tile (fp32 with subnormals), tiled alike."""
    t0 = time.perf_counter()
    hyper, t = C.HYPER["project"], 7
    b1, b2, eps, lr = hyper
    n, tile_n = (1 << 26) + 5, 1 << 16
    tile = C.adam_case(tile_n, 77, eps, "BC" if form == "zero_grad" else C.CLASSES, b1=b1)
    up = lambda x: x.cuda().repeat(n // tile_n + 1)[:n].contiguous()
    case = {k: up(tile[k]) for k in ("p0", "g", "m0", "v0", "cls")}
    case["n"] = n
    y_t = tuple(up(x) for x in _refs(tile, t, hyper)[1])
    r64 = R.adam_step(case["p0"], case["g"], case["m0"], case["v0"], t, lr, b1, b2, eps)          # float64 on the device
    p, g, m, v = (Buf(case[k]) for k in ("p0", "g", "m0", "v0"))
    if form == "zero_grad":
        rc = _lib().nsa_adam_table_step_zero_grad(p.ptr, m.ptr, v.ptr, n, t, lr, b1, b2, eps, st())
    else:
        rc = _lib().nsa_adam_table_step(p.ptr, g.ptr, m.ptr, v.ptr, n, t, lr, b1, b2, eps, st())
    assert rc == NSA_OK
    _intact("non-temporal " + form, p, g, m, v)
    assert torch.equal(_bits(g.t), _bits(case["g"]))
    failures = []
    judge = _judge(failures)
    judge.add(f"non-temporal {form} n=2^26+5", case, (m.t, v.t, p.t), r64, y_t, y_t)
    _finish(judge, f"non-temporal {form}", capsys)
    # the plain form on the two halves (each below the threshold): reported, not asserted -- contraction may differ between kernels
    half = 1 << 25
    q = [Buf(case[k]) for k in ("p0", "g", "m0", "v0")]
    for lo, cnt in ((0, half), (half, n - half)):
        a = [b.ptr + 4 * lo for b in q]
        if form == "zero_grad":
            rc = _lib().nsa_adam_table_step_zero_grad(a[0], a[2], a[3], cnt, t, lr, b1, b2, eps, st())
        else:
            rc = _lib().nsa_adam_table_step(*a, cnt, t, lr, b1, b2, eps, st())
        assert rc == NSA_OK
    torch.cuda.synchronize()
    same = [torch.equal(_bits(x.t), _bits(y.t)) for x, y in zip((p, m, v), (q[0], q[2], q[3]))]
    with capsys.disabled():
        print(f"\n  == non-temporal {form}: bit-identical to the plain form on the two halves: p {same[0]}  m {same[1]}  v {same[2]};  "
              f"wall time of this test {time.perf_counter() - t0:.1f} s")
    assert not failures, [f["what"] for f in failures]


# ------------------------------------------------------------------------------------------------------------------ multi
MULTI_N = (1, 255, 256, 257, 65536, 3, 4, 5, 63, 64, 65, 511, 513, 1000, 1023, 1025, 2051, 4097, 7, 31, 33, 127, 129, 12345)


def run_multi(segs, hyper, what):
    """segs: [(case, t, lr, shift)] -> [(m, v, p)]"""
    from nicer_slam_amd._native import AdamSeg
    b1, b2, eps, _lr = hyper
    bufs = [[Buf(case[k], shift=shift) for k in ("p0", "g", "m0", "v0")] for case, _t, _lr, shift in segs]
    arr = (AdamSeg * len(segs))(*[AdamSeg(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, case["n"], t, lr)
                                  for b, (case, t, lr, _s) in zip(bufs, segs)])
    assert _lib().nsa_adam_multi_step(arr, len(segs), b1, b2, eps, st()) == NSA_OK, what
    _intact(what, *[x for b in bufs for x in b])
    for b, (case, _t, _lr, _s) in zip(bufs, segs):
        assert torch.equal(_bits(b[1].cpu()), _bits(case["g"]))
    return [(b[2].cpu(), b[3].cpu(), b[0].cpu()) for b in bufs]


@pytest.mark.parametrize("name", ["project", "tracker"])
def test_multi_step_24_segments_vs_float64(name, capsys):
    from nicer_slam_amd._native import AdamSeg
    hyper = C.HYPER[name]
    b1, b2, eps, _lr = hyper
    failures = []
    judge = _judge(failures)
    segs = [(C.adam_case(n, 7 * i + 1, eps, b1=b1), C.STEPS[i % 5], (0.04, 0.005, 0.0, 1e-3)[i % 4], 1 if i % 3 == 1 else 0)
            for i, n in enumerate(MULTI_N)]
    assert len(segs) == 24
    for count, sub in ((24, segs), (1, segs[3:4]), (1, segs[4:5])):
        for (case, t, lr, shift), got in zip(sub, run_multi(sub, hyper, f"multi {name} x{count}")):
            judge.add(f"multi {name} x{count} n={case['n']} t={t} lr={lr}", case, got, *_refs(case, t, (b1, b2, eps, lr)))
            if lr == 0.0:
                assert torch.equal(_bits(got[2]), _bits(case["p0"]))
    _finish(judge, f"multi {name}", capsys)
    dummy = Buf(n=8, fill=0.0)
    arr = (AdamSeg * 25)(*[AdamSeg(dummy.ptr, dummy.ptr, dummy.ptr, dummy.ptr, 8, 1, 0.0) for _ in range(25)])
    assert _lib().nsa_adam_multi_step(arr, 25, b1, b2, eps, st()) == NSA_EBADARG
    assert not failures, [f["what"] for f in failures]


# ------------------------------------------------------------------------------------------------------------------ optim.Adam
def test_optimizer_class_one_step_from_a_loaded_state(capsys):
    """nicer_slam_amd.optim.Adam: 50 small parameters in two groups (different lr and eps: two flushes of 24 and a key change), 65536 and
    65537 elements (both sides of SMALL), and under none_grad="zeros" a small and a large parameter without a gradient -- against float64
    torch.optim.Adam on CPU copies, torch's fp32 CPU Adam as the yardstick."""
    from nicer_slam_amd.optim import Adam
    t = 7
    # (hyper-parameters that ARE fp32 numbers: the C ABI takes floats, and 1 - fl(0.99) is not fl(1 - 0.99) -- see DESIGN.md section 7)
    groups = [dict(lr=R.f32(0.04), eps=R.f32(1e-15)), dict(lr=R.f32(0.005), eps=R.f32(1e-8))]
    sizes = [[(1, 3, 255, 256, 257, 1000, 4097)[i % 7] + i for i in range(30)] + [65536, 65537],
             [(5, 64, 513, 2051)[i % 4] + i for i in range(20)] + [65537, 300]]
    no_grad = {(0, 31), (1, 20), (1, 21), (0, 4)}        # a large and a small one in either group
    cases = [[C.adam_case(n, 100 * gi + i, groups[gi]["eps"], "BC" if (gi, i) in no_grad else C.CLASSES) for i, n in enumerate(ns)]
             for gi, ns in enumerate(sizes)]

    def build(cls, dtype, device, **kw):
        params = [[c["p0"].to(device, dtype).clone().requires_grad_(True) for c in cs] for cs in cases]
        opt = cls([dict(params=ps, **g) for ps, g in zip(params, groups)], betas=(R.f32(0.9), R.f32(0.99)), **kw)
        sd = opt.state_dict()
        flat = [c for cs in cases for c in cs]
        sd["state"] = {i: dict(step=torch.tensor(float(t - 1)), exp_avg=c["m0"].to(dtype).clone(), exp_avg_sq=c["v0"].to(dtype).clone())
                       for i, c in enumerate(flat)}
        opt.load_state_dict(sd)
        for gi, ps in enumerate(params):
            for i, p in enumerate(ps):
                if (gi, i) in no_grad and cls is Adam:
                    p.grad = None
                else:                              # (torch skips a None gradient: the reference environment's zero tensor instead)
                    p.grad = cases[gi][i]["g"].to(device, dtype).clone()
        opt.step()
        return [(opt.state[p]["exp_avg"].detach().cpu(), opt.state[p]["exp_avg_sq"].detach().cpu(), p.detach().cpu(),
                 int(opt.state[p]["step"])) for ps in params for p in ps]

    got = build(Adam, F32, "cuda", none_grad="zeros")
    torch.cuda.synchronize()
    r64, y32 = build(torch.optim.Adam, F64, "cpu"), build(torch.optim.Adam, F32, "cpu")
    failures = []
    judge = _judge(failures)
    for c, a, r, y in zip([c for cs in cases for c in cs], got, r64, y32):
        assert a[3] == r[3] == t
        judge.add(f"optim.Adam n={c['n']}", c, a[:3], r[:3], y[:3], y[:3])
    _finish(judge, "optim.Adam", capsys)
    assert not failures, [f["what"] for f in failures]


# ------------------------------------------------------------------------------------------------------------------ camera forms
def _camera_step(state, g_raw, t, hyper, lr_step, gamma, div, cls, judge, tag, got):
    """one camera step judged: state = the fp32 (p, m, v) the kernel started from, got = what it left"""
    b1 = hyper[0]
    g32 = g_raw / div if div else g_raw                  # the kernel's own fp32 quotient
    g64 = g_raw.double() / div if div else g_raw.double()
    case = dict(p0=state[0], m0=state[1], v0=state[2], g=g32, cls=cls, n=g_raw.numel())
    judge.add(tag, case, got, *_refs(case, t, hyper, lr_step, gamma, g64=g64, camera=True))


def run_camera_sequence(n, seed, hyper, lr_step, gamma, steps, t0, div, judge, tag, best_losses=None):
    """nsa_adam_step (div None) or nsa_adam_step_scaled, `steps` steps from the kernel's own state, the device step scalar preset to
    t0; judge None: the steps are not judged.  best_losses: the loss of every step -- then the candidate (best[0], best[1..]) must follow keep_best bit for bit."""
    lib = _lib()
    b1, b2, eps, lr = hyper
    case = C.adam_case(n, seed, eps, b1=b1)
    p, m, v, g = Buf(case["p0"]), Buf(case["m0"]), Buf(case["v0"]), Buf(n=n, fill=0.0)
    step = Buf(torch.tensor([float(t0)]))
    dv = Buf(torch.tensor([float(div)])) if div else None
    loss, best = Buf(n=1, fill=0.0), Buf(torch.cat([torch.tensor([1e10]), torch.zeros(n)]))
    state, cams, seen = (case["p0"], case["m0"], case["v0"]), [], []
    for i in range(steps):
        t = t0 + i + 1
        fresh = case if i == 0 else C.adam_case(n, seed + 8 * (1 + 131 * i), eps, b1=b1)
        g_raw = (case["g"] * (div or 1.0)) if i == 0 else C.next_gradient(fresh, state[1], b1, div or 1.0)
        g.t.copy_(g_raw)
        if best_losses is not None:
            loss.t.fill_(best_losses[i])
        if div:
            rc = lib.nsa_adam_step_scaled(p.ptr, g.ptr, dv.ptr, m.ptr, v.ptr, step.ptr, n, lr, b1, b2, eps, lr_step, gamma,
                                          loss.ptr if best_losses is not None else None, best.ptr if best_losses is not None else None, st())
        else:
            rc = lib.nsa_adam_step(p.ptr, g.ptr, m.ptr, v.ptr, step.ptr, n, lr, b1, b2, eps, lr_step, gamma, st())
        assert rc == NSA_OK
        _intact(tag, p, m, v, g, step, loss, best)
        got = (m.cpu(), v.cpu(), p.cpu())
        assert float(step.cpu()[0]) == t
        if judge is not None:
            _camera_step(state, g_raw, t, hyper, lr_step, gamma, div, case["cls"], judge, f"{tag} t={t}", got)
        state = (got[2], got[0], got[1])
        if best_losses is not None:
            cams.append(got[2].numpy().copy())
            seen.append(np.float32(best_losses[i]) / np.float32(div))
            want_l, want_c = R.keep_best(seen, cams)[-1]
            b = best.cpu().numpy()
            assert b[0].tobytes() == np.float32(want_l).tobytes(), (tag, i, b[0], want_l)
            assert b[1:].tobytes() == (np.zeros(n, np.float32) if want_c is None else want_c).tobytes(), (tag, i)


@pytest.mark.parametrize("name", ["tracker", "project"])
def test_camera_adam_step_sizes_schedules_and_scaling(name, capsys):
    hyper = C.HYPER[name]
    failures = []
    judge = _judge(failures)
    for n in (1, 7, 64, 65, 256):                                      # nsa_adam_step, one step, constant lr
        for seed in range(64 if n <= 7 else 4):
            run_camera_sequence(n, 8 * seed + n, hyper, 0, 1.0, 1, (0, 6)[seed % 2], None, judge, f"adam_step n={n}")
    _finish(judge, f"camera {name}: nsa_adam_step n in 1..256", capsys)
    for seed in range(64):                                             # StepLR(3, 0.5) over t = 1..8
        run_camera_sequence(7, 1000 + seed, hyper, 3, 0.5, 8, 0, None, judge, "adam_step StepLR(3,0.5)")
    _finish(judge, f"camera {name}: StepLR(3,0.5) t=1..8", capsys)
    for t0 in (49, 50, 51):                                            # StepLR(50, 0.95), the step scalar preset
        for seed in range(64):
            run_camera_sequence(7, 2000 + 8 * seed + t0, hyper, 50, 0.95, 1, t0, None, judge, f"adam_step StepLR(50,0.95) from {t0}")
    _finish(judge, f"camera {name}: StepLR(50,0.95) from 49, 50, 51", capsys)
    for div in (1024.0, 3.0):                                          # nsa_adam_step_scaled
        for seed in range(64):
            run_camera_sequence(7, 3000 + seed, hyper, 3, 0.5, 4, 0, div, judge, f"adam_step_scaled / {div:g}")
        _finish(judge, f"camera {name}: grad_div {div:g}", capsys)
    assert not failures, [f["what"] for f in failures]


def test_camera_adam_step_beyond_256_and_bad_arguments():
    lib = _lib()
    b = [Buf(n=300, fill=0.5) for _ in range(4)]
    step = Buf(torch.tensor([0.0]))
    before = [x.words.clone() for x in b + [step]]
    a = [x.ptr for x in b] + [step.ptr]
    assert lib.nsa_adam_step(*a, 257, 0.01, 0.9, 0.999, 1e-8, 0, 1.0, st()) == NSA_EBADARG      # documented: n <= 256
    assert lib.nsa_adam_step(*a, 0, 0.01, 0.9, 0.999, 1e-8, 0, 1.0, st()) == NSA_EBADARG
    assert lib.nsa_adam_step_scaled(a[0], a[1], None, a[2], a[3], a[4], 7, 0.01, 0.9, 0.999, 1e-8, 0, 1.0, None, None, st()) == NSA_EBADARG
    torch.cuda.synchronize()
    for x, w in zip(b + [step], before):
        assert torch.equal(x.words, w)


LOSSES = (5.0, 3.0, 3.0, float("nan"), 4.0, 2.0, 2.0)


# ------------------------------------------------------------------------------------------------------------------ tracker
_JAC = {}


def _jacobian_abs(uv, K, cam):
    """[R,7,6] |d (per-ray cam term) / d (g_o, g_d)| in float64"""
    key = (uv.numpy().tobytes(), K.numpy().tobytes(), cam.numpy().tobytes())
    if key not in _JAC:
        _JAC[key] = _jacobian_abs_of(uv, K, cam)
    return _JAC[key]


def _jacobian_abs_of(uv, K, cam):
    R_ = uv.shape[0]
    cols = []
    for k in range(6):
        e = torch.zeros(R_, 6, dtype=F64)
        e[:, k] = 1.0
        cols.append(R.per_ray_cam_terms(uv, K, cam, e[:, :3], e[:, 3:]))
    return torch.stack(cols, -1).abs()


def _tracker_case(Rn, seed, S=None):
    rc = OC.rays_case(1, Rn, seed)
    out = dict(uv=rc["uv"][0].contiguous(), K=rc["K"][0].contiguous(), cam=rc["cam"][0].contiguous(), g_o=rc["g_o"], g_d=rc["g_d"], R=Rn)
    if S:
        rb = OC.rays_backward_case(Rn, S, seed + 1)
        g = torch.Generator().manual_seed(seed + 2)
        out.update(z=rb["z"], g_x=rb["g_x"], g_dir=rb["g_dir"], ray_loss=torch.rand(Rn, generator=g) * 3, S=S)
    return out


def run_track_tail(c, weight, slot7, adam=None):
    """-> g_cam [9] (slot 8 a NaN sentinel of its own when weight = 0)"""
    d = {k: Buf(c[k]) for k in ("uv", "K", "cam", "g_o", "g_d")}
    gc = Buf(torch.tensor([float("nan")] * 7 + [slot7, float("nan")]))
    extra = []
    if adam is None:
        rc = _lib().nsa_track_tail(d["uv"].ptr, d["K"].ptr, d["cam"].ptr, c["R"], d["g_o"].ptr, d["g_d"].ptr, gc.ptr, 0, weight,
                                   None, None, None, 0.0, 0.9, 0.999, 1e-8, 0, 1.0, None, None, st())
    else:
        m, v, step, loss, best, (b1, b2, eps, lr), lr_step, gamma = adam
        extra = [m, v, step, loss, best]
        rc = _lib().nsa_track_tail(d["uv"].ptr, d["K"].ptr, d["cam"].ptr, c["R"], d["g_o"].ptr, d["g_d"].ptr, gc.ptr, 1, weight,
                                   m.ptr, v.ptr, step.ptr, lr, b1, b2, eps, lr_step, gamma, loss.ptr, best.ptr, st())
    assert rc == NSA_OK
    _intact("nsa_track_tail", gc, *d.values(), *extra)
    for k in ("uv", "K", "g_o", "g_d") + (("cam",) if adam is None else ()):
        assert torch.equal(_bits(d[k].cpu()), _bits(c[k].reshape(-1)))
    return gc.cpu(), d["cam"].cpu()


def run_track_finish(c, weight, adam=None):
    """-> (red [9], cam after, ticket word)"""
    Rn, S = c["R"], c["S"]
    d = {k: Buf(c[k]) for k in ("uv", "K", "cam", "z", "g_x", "g_dir", "ray_loss")}
    gc = Buf(torch.tensor([float("nan")] * 9))
    ws = Buf(n=int(_lib().nsa_track_finish_workspace(Rn)), fill=0.0)
    a = [d["uv"].ptr, d["K"].ptr, d["cam"].ptr, Rn, S, d["z"].ptr, d["g_x"].ptr, d["g_dir"].ptr, d["ray_loss"].ptr, gc.ptr]
    extra = []
    if adam is None:
        rc = _lib().nsa_track_finish(*a, 0, weight, None, None, None, 0.0, 0.9, 0.999, 1e-8, 0, 1.0, None, ws.ptr, st())
    else:
        m, v, step, best, (b1, b2, eps, lr), lr_step, gamma = adam
        extra = [m, v, step, best]
        rc = _lib().nsa_track_finish(*a, 1, weight, m.ptr, v.ptr, step.ptr, lr, b1, b2, eps, lr_step, gamma, best.ptr, ws.ptr, st())
    assert rc == NSA_OK
    _intact("nsa_track_finish", gc, ws, *d.values(), *extra)
    return gc.cpu(), d["cam"].cpu(), int(ws.words[ws.lo])


TRACK_R = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def _add_message(pool, what, got, ref, y32, norm7, loss_norm, weight):
    """slots 0..3 (quaternion), 4..6 (translation), 7 (loss) as rows of one value each; slot 8 exactly the weight"""
    w = weight if weight > 0 else 1.0
    for name, sl, nrm in (("quaternion", slice(0, 4), norm7[:4] * w), ("translation", slice(4, 7), norm7[4:] * w),
                          ("loss slot", slice(7, 8), torch.tensor([loss_norm * w], dtype=F64))):
        pool.add(f"{what}: {name}", got[sl, None], ref[sl, None], y32[sl, None], nrm)
    if weight > 0:
        assert float(got[8]) == weight
    else:
        assert bool(torch.isnan(got[8])), "slot 8 was written without a reduce weight"


@pytest.mark.parametrize("weight", [0.0, 3.0])
def test_track_tail_g_cam_vs_float64(weight, capsys):
    pool, failures = Pool(), []
    for Rn in TRACK_R:
        for seed in range(8):
            c = _tracker_case(Rn, 10 * Rn + seed)
            args = (c["uv"], c["K"], c["cam"], c["g_o"], c["g_d"])
            slot7 = 0.375 + seed
            ref, y32 = R.track_tail_g_cam(*args, weight, slot7), R.track_tail_g_cam(*args, weight, slot7, dtype=F32)
            norm7 = (_jacobian_abs(*args[:3]) * torch.cat([c["g_o"], c["g_d"]], 1).double().abs()[:, None, :]).sum((0, 2))
            got, _cam = run_track_tail(c, weight, slot7)
            _add_message(pool, "nsa_track_tail g_cam", got.double(), ref, y32.double(), norm7, slot7, weight)
    with capsys.disabled():
        print()
        pool.judge(f"reduce_weight {weight:g}: ", failures)
    zero = _tracker_case(65, 5)
    zero["g_o"], zero["g_d"] = torch.zeros(65, 3), torch.zeros(65, 3)
    got, _cam = run_track_tail(zero, weight, 0.0)
    assert bool((got[:8] == 0).all()), "all-zero cotangents: the gradient is not exactly zero"
    assert not failures, [f["what"] for f in failures]


@pytest.mark.parametrize("S", [64, 98])
@pytest.mark.parametrize("weight", [0.0, 3.0])
def test_track_finish_red_vs_float64(weight, S, capsys):
    pool, failures = Pool(), []
    for Rn in TRACK_R:
        for seed in range(8):
            c = _tracker_case(Rn, 10 * Rn + seed, S)
            args = (c["uv"], c["K"], c["cam"], c["z"], c["g_x"], c["g_dir"], c["ray_loss"])
            ref, y32 = R.track_finish_red(*args, weight), R.track_finish_red(*args, weight, dtype=F32)
            mag = torch.cat([c["g_x"].double().abs().sum(1),
                             (c["z"].double()[..., None] * c["g_x"].double()).abs().sum(1) + c["g_dir"].double().abs().sum(1)], 1)
            norm7 = (_jacobian_abs(c["uv"], c["K"], c["cam"]) * mag[:, None, :]).sum((0, 2))
            got, _cam, ticket = run_track_finish(c, weight)
            assert ticket == 0, "nsa_track_finish left its ticket word non-zero"
            _add_message(pool, f"nsa_track_finish red S={S}", got.double(), ref, y32.double(), norm7,
                         float(c["ray_loss"].double().sum() / (3 * Rn)), weight)
    with capsys.disabled():
        print()
        pool.judge(f"reduce_weight {weight:g}: ", failures)
    zero = _tracker_case(65, 5, S)
    zero["g_x"], zero["g_dir"] = torch.zeros(65, S, 3), torch.zeros(65, S, 3)
    got, _cam, ticket = run_track_finish(zero, weight)
    assert bool((got[:7] == 0).all()) and ticket == 0
    assert not failures, [f["what"] for f in failures]


@pytest.mark.parametrize("via", ["track_tail", "track_finish"])
def test_adam_step_inside_the_tracker_tails(via, capsys):
    """the camera step of nsa_track_tail / nsa_track_finish, fed the kernel's own fp32 gradient (its g_cam), 64 seeds pooled, StepLR(3,
    0.5) with the step scalar preset to 2, 3 and 4; the candidate follows the loss (nsa_track_tail: the caller's scalar, no loss_div;
    nsa_track_finish: slot 7 of its own message)"""
    hyper = C.HYPER["tracker"]
    b1, b2, eps, lr = hyper
    failures = []
    judge = _judge(failures)
    cls = torch.full((7,), ord("A"), dtype=torch.uint8)
    for seed in range(64):
        c = _tracker_case(65, 400 + seed, 64 if via == "track_finish" else None)
        c["cam"][:4] = torch.nn.functional.normalize(c["cam"][:4], dim=0)             # a camera of unit scale, as the tracker holds it
        dry = run_track_tail(c, 0.0, 0.0)[0][:7] if via == "track_tail" else run_track_finish(c, 0.0)[0][:7]
        rng = np.random.default_rng(seed)
        m0 = (0.5 * dry.double() * torch.from_numpy(rng.standard_normal(7))).float()
        m0 = torch.where((b1 * m0 + (1 - b1) * dry).abs() < torch.maximum(m0.abs(), dry.abs()) / 16, -m0, m0)      # optim_cases' rule
        v0 = (dry.double() ** 2 * torch.from_numpy(rng.uniform(0.2, 2, 7))).float()
        t0 = (2, 3, 4)[seed % 3]
        m, v, step = Buf(m0), Buf(v0), Buf(torch.tensor([float(t0)]))
        loss_value, prior = 0.5, (0.25, 1e10)[seed % 2]                                # a candidate that stays / one that is replaced
        best = Buf(torch.tensor([prior] + [9.0] * 7))
        if via == "track_tail":
            loss = Buf(torch.tensor([loss_value]))
            gc, cam = run_track_tail(c, 0.0, loss_value, (m, v, step, loss, best, hyper, 3, 0.5))
            l = np.float32(loss_value)
        else:
            gc, cam, ticket = run_track_finish(c, 0.0, (m, v, step, best, hyper, 3, 0.5))
            assert ticket == 0
            l = gc[7].numpy()
        assert torch.equal(_bits(gc[:7]), _bits(dry)), "the gradient differs between the run with and without the step"
        assert float(step.cpu()[0]) == t0 + 1
        got = (m.cpu(), v.cpu(), cam)
        _camera_step((c["cam"], m0, v0), gc[:7].clone(), t0 + 1, hyper, 3, 0.5, None, cls, judge, f"{via} step", got)
        b = best.cpu().numpy()
        want = np.concatenate([[l], cam.numpy()]) if l < np.float32(prior) else np.array([prior] + [9.0] * 7)
        assert b.tobytes() == want.astype(np.float32).tobytes(), (via, seed, b, want)
    _finish(judge, f"camera step inside nsa_{via}", capsys)
    assert not failures, [f["what"] for f in failures]


@pytest.mark.parametrize("div", [1024.0, 3.0, None])
def test_candidate_sequence_follows_keep_best(div):
    """losses 5, 3, 3, NaN, 4, 2, 2: strict <, a NaN never wins, the camera AFTER the step -- with loss_div (nsa_adam_step_scaled: the
    loss is divided by the same device scalar as the gradient) and without (nsa_track_tail)"""
    hyper = C.HYPER["tracker"]
    if div:                                        # (the steps themselves are judged by test_camera_adam_step_sizes_schedules_and_scaling)
        run_camera_sequence(7, 42, hyper, 0, 1.0, len(LOSSES), 0, div, None, f"candidate / {div:g}", best_losses=LOSSES)
    else:
        c = _tracker_case(5, 9)
        c["cam"][:4] = torch.nn.functional.normalize(c["cam"][:4], dim=0)
        m, v, step = Buf(torch.zeros(7)), Buf(torch.zeros(7)), Buf(torch.tensor([0.0]))
        best = Buf(torch.tensor([1e10] + [0.0] * 7))
        cams = []
        for i, l in enumerate(LOSSES):
            loss = Buf(torch.tensor([l]))
            _gc, cam = run_track_tail(c, 0.0, l, (m, v, step, loss, best, hyper, 0, 1.0))
            c["cam"] = cam.clone()
            cams.append(cam.numpy().copy())
            want_l, want_c = R.keep_best(LOSSES[:i + 1], cams)[-1]
            b = best.cpu().numpy()
            assert b[0].tobytes() == np.float32(want_l).tobytes() and b[1:].tobytes() == want_c.tobytes(), (i, b, want_l, want_c)
        assert len({x.tobytes() for x in cams}) == len(cams), "the camera did not move between the steps"


# ------------------------------------------------------------------------------------------------------------------ weight norm
def _wn_table(layers):
    from nicer_slam_amd._native import WnLayer
    bufs = [[Buf(x) for x in l] for l in layers]
    arr = (WnLayer * len(layers))(*[WnLayer(b[0].ptr, b[1].ptr, b[2].ptr, l[0].shape[0], l[0].shape[1]) for b, l in zip(bufs, layers)])
    return arr, bufs


def _wn_rows(layers, flat_like, stride_extra):
    """the weight rows of a flat vector laid out per layer as [rows x cols | stride_extra x rows] -> [total rows, max cols], zero padded"""
    width = max(l[0].shape[1] for l in layers)
    out, off = [], 0
    for v, _g, _b in layers:
        rows, cols = v.shape
        out.append(torch.nn.functional.pad(flat_like[off:off + rows * cols].double().reshape(rows, cols), (0, width - cols)))
        off += rows * cols + stride_extra * rows
    return torch.cat(out)


def _wn_tails(layers, flat_like, stride_extra, which):
    out, off = [], 0
    for v, _g, _b in layers:
        rows, cols = v.shape
        lo = off + rows * cols + which * rows
        out.append(flat_like[lo:lo + rows])
        off += rows * cols + stride_extra * rows
    return torch.cat(out)


@pytest.mark.parametrize("n_layers", [1, 3, 8])
def test_weight_norm_flat_and_backward_vs_float64(n_layers, capsys):
    lib = _lib()
    pool, failures = Pool(), []                    # (rows pooled over the seeds: one or two rows are a coin toss)
    for seed in range(6 if n_layers < 8 else 3):
        layers = C.wn_layers(n_layers, seed)
        g_flat, c = C.wn_cotangent(layers, seed)
        n_rows = sum(l[0].shape[0] for l in layers)
        total = g_flat.numel()
        arr, bufs = _wn_table(layers)
        flat, norms = Buf(n=total, fill=float("nan")), Buf(n=n_rows, fill=float("nan"))
        assert lib.nsa_weight_norm_flat(arr, n_layers, flat.ptr, norms.ptr, st()) == NSA_OK
        _intact("nsa_weight_norm_flat", flat, norms, *[x for b in bufs for x in b])
        got = flat.cpu()
        ref, n64 = R.weight_norm_flat(layers)
        y32 = R.weight_norm_flat(layers, F32)[0]
        g_abs = torch.cat([l[1] for l in layers]).double().abs()
        pool.add("forward rows / |g|", *(_wn_rows(layers, x, 1) for x in (got, ref, y32)), g_abs)
        assert torch.equal(_bits(_wn_tails(layers, got, 1, 0)), _bits(torch.cat([l[2] for l in layers]))), "bias not copied bit for bit"
        assert float(got[-1]) == 0.0
        assert bool(torch.isfinite(norms.cpu()).all())
        # backward, from the kernel's own fp32 norms
        gf, gp = Buf(g_flat), Buf(n=total - 1 + n_rows, fill=float("nan"))
        assert lib.nsa_weight_norm_flat_backward(arr, n_layers, norms.ptr, gf.ptr, gp.ptr, st()) == NSA_OK
        _intact("nsa_weight_norm_flat_backward", gp, gf, norms, *[x for b in bufs for x in b])
        got = gp.cpu()
        ref = R.weight_norm_flat_backward(layers, g_flat)
        y32 = R.weight_norm_flat_backward(layers, g_flat, F32)
        gw_norm = _wn_rows(layers, g_flat, 1).norm(dim=1)
        pool.add("backward g_v rows / (|g| |gW| / |v|)", *(_wn_rows(layers, x, 2) for x in (got, ref, y32)), g_abs * gw_norm / n64)
        # g_g missed the gate against the header's order s / |v| on MI355X at 8 layers (1.58 x rms), traced in k_weight_norm_flat_bwd:
        # out = s * rnorm with rnorm = 1.0f / norm -- a reciprocal and a product, two roundings where the quotient has one; it shows on
        # the cols = 1 rows (65 of them at 8 layers), whose s is a single product and whose |v| is exact.  A different but valid fp32
        # order: this quantity alone has a second yardstick in that order.
        y_ker = R.weight_norm_flat_backward(layers, g_flat, F32, kernel_order=True)
        rows = [_wn_tails(layers, x, 2, 0).double()[:, None] for x in (got, ref, y32, y_ker)]
        pool.add("backward g_g / |gW|", *rows[:3], gw_norm, kernel_order=rows[3])
        assert torch.equal(_bits(_wn_tails(layers, got, 2, 1)), _bits(_wn_tails(layers, g_flat, 1, 0))), "g_bias is not the cotangent's slice"
        zero = c == 0
        assert n_rows <= 2 or bool(zero.any())
        assert bool((_wn_rows(layers, got, 2)[zero] == 0).all()) and bool((_wn_tails(layers, got, 2, 0)[zero] == 0).all()) and \
            bool((_wn_tails(layers, got, 2, 1)[zero] == 0).all()), "a row with a zero cotangent has a non-zero gradient"
    with capsys.disabled():
        print()
        pool.judge(f"weight norm, {n_layers} layers: ", failures)
    assert not failures, [f["what"] for f in failures]


def test_weight_norm_nine_layers_is_refused():
    layers = C.wn_layers(8, 0) + C.wn_layers(1, 1)
    arr, bufs = _wn_table(layers)
    out = Buf(n=8, fill=0.0)
    assert _lib().nsa_weight_norm_flat(arr, 9, out.ptr, out.ptr, st()) == NSA_EBADARG
    assert _lib().nsa_weight_norm_flat_backward(arr, 9, out.ptr, out.ptr, out.ptr, st()) == NSA_EBADARG
    _intact("nine layers", out)


# ------------------------------------------------------------------------------------------------------------------ voxels and keys
def _points_desc(x):
    from nicer_slam_amd._native import PointsDesc
    b = Buf(torch.from_numpy(x))
    return PointsDesc(None, None, None, b.ptr, x.shape[0], 0, None), b


def _voxel_sets():
    for P in C.VOXEL_P:
        yield f"crafted P={P}", C.crafted_points(P, 7 * P)
    for kind in ("same", "straddle", "alternate"):
        yield kind, C.run_points(kind)


@pytest.mark.parametrize("res", C.VOXEL_RES)
def test_update_voxels_on_crafted_points_exactly(res):
    lib = _lib()
    vox = Buf(n=res ** 3, fill=0.0)
    want = torch.zeros(res ** 3, device="cuda")
    for what, x in _voxel_sets():
        desc, b = _points_desc(x)
        assert lib.nsa_update_voxels(ctypes.byref(desc), vox.ptr, res, st()) == NSA_OK
        _intact(f"nsa_update_voxels res={res} {what}", vox, b)
        idx = R.voxel_index(x, res)
        idx = torch.from_numpy(idx[idx >= 0]).cuda()
        assert idx.numel() > 0
        want.index_add_(0, idx, torch.ones(idx.numel(), device="cuda"))
        assert torch.equal(vox.t, want), f"res={res} {what}: the counts differ from the fp32 statement"        # (accumulated over the sets)


def test_morton_keys_on_crafted_points_exactly():
    lib = _lib()
    sets = [(w, x) for w, x in _voxel_sets()] + [(f"with NaN and clamps P={P}", C.crafted_points(P, 3 * P, nan=True)) for P in C.VOXEL_P]
    for what, x in sets:
        desc, b = _points_desc(x)
        keys = Buf(n=x.shape[0], dtype=torch.int32)
        assert lib.nsa_morton_keys(ctypes.byref(desc), keys.ptr, st()) == NSA_OK
        _intact(f"nsa_morton_keys {what}", keys, b)
        assert np.array_equal(keys.cpu().numpy(), R.morton_key(x)), what
    nan = np.array([[np.nan, -1.0, -1.0], [np.nan, np.nan, np.nan], [-5.0, 7.0, np.nan]], dtype=np.float32)
    desc, b = _points_desc(nan)
    keys = Buf(n=3, dtype=torch.int32)
    assert lib.nsa_morton_keys(ctypes.byref(desc), keys.ptr, st()) == NSA_OK
    torch.cuda.synchronize()
    assert keys.cpu().tolist() == [0, 0, int(R.morton_key(np.array([[-1.0, 1.0, -1.0]], dtype=np.float32))[0])]      # NaN -> cell 0
