"""The per-ray importance sampler k_sample_rays against float64 (tests/sampler_ref64.py), sample by sample, through the C ABI
(nsa_sample_rays called directly: no network, no model).

The method is tests/test_objective_float64_gpu.py's (the gate and its Pool are tests/gate64.py), in TWO classes,
because the reference's own algorithm is discontinuous in z where a chosen bin sits on the 1e-5 floor (its normalised mass is a hair
under the den < 1e-5 switch, so an fp32 and a float64 evaluation legitimately take different branches there) and at u = 1 (the last cdf
entry rounds to 1 or to 1 + 2^-23); it is continuous in u everywhere:
  * u-space, EVERY sample: e = |cdf64(z) - cdf64(z_64)| with the float64 bins and cdf on both sides;
  * z-space, the determinate samples -- float64 mass of the chosen bin >= 2e-5 and j < N - 1 --: e = |z - z_64| / max(far, 1);
    tests/test_sampler_ref64_cpu.py asserts that these are at least 90 % of every case with N >= 94 (1 - 1 / N - 10 % below);
  * the samples that remain must lie inside the float64 sample's bin or an adjacent one.
e_k is the kernel's error, e_32 that of the fp32 mode of the same restatement (reference order) and of a second fp32 evaluation in the
kernel's documented order; gate: rms(e_k) <= 1.5 rms(e_32) and max(e_k) <= 3 max(e_32) against the larger of the two yardsticks,
pooled over the cases and judged once per (family, E class).  No fixed tolerance.

Exact, on every case: NSA_OK; every output finite, the guard words around the outputs untouched; rows non-decreasing and inside
[min(near, z_0), max(far, z_{E-1})]; every row holds near, far[ray] and z[ray, clamp(extra_idx)] bit for bit and with multiplicity (they
are removed from the row as a multiset; what remains, in order, is sample j = 0 ... N - 1: the inverse cdf is monotone in u);
z_eik[ray] == z_vals[ray, clamp(eik_idx[ray])]; the call without z_eik, a second call, the ray alone (R = 1) and the ray in a permuted
batch give the same bits.

Inputs: tests/sampler_cases.py.  Measured on MI355X: DESIGN.md section 7 holds the printed table."""
import bisect

import pytest
import torch

import sampler_cases as C
import sampler_ref64 as S
from devcall import dev, ptr, st
from gate64 import Pool

pytestmark = pytest.mark.gpu
GUARD, GUARD_WORD, NAN_WORD = 64, 0x5A5A5A5A, 0x7FC00000
NSA_OK, NSA_EBADARG = 0, 4


def _guarded(n):
    """n floats pre-filled with NaN between two runs of guard words -> (whole int32 buffer, the float32 view of the middle)"""
    buf = torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device="cuda")
    buf[GUARD:GUARD + n] = NAN_WORD
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_ok(buf):
    return bool((buf[:GUARD] == GUARD_WORD).all()) and bool((buf[-GUARD:] == GUARD_WORD).all())


class DevCase:
    def __init__(self, cs, rays=None):
        take = (lambda t: t) if rays is None else (lambda t: t[rays].contiguous())
        self.cs = cs
        self.R = cs["R"] if rays is None else len(rays)
        self.t = {k: dev(take(cs[k])) for k in ("rays_o", "rays_d", "z", "sdf", "far")}
        self.voxels, self.u = dev(cs["voxels"]), dev(S.u_lin(cs["N"]))
        self.extra = None if cs["extra_idx"] is None else cs["extra_idx"].cuda()
        self.eik = take(cs["eik_idx"]).cuda()

    def call(self, with_eik=True, **over):
        """-> rc, z_vals [R,S] (CPU), z_eik [R] or None, guards untouched"""
        from nicer_slam_amd._native import lib
        cs, t, R = self.cs, self.t, self.R
        a = dict(voxel_res=cs["voxel_res"], E=cs["E"], N=cs["N"], n_extra=cs["n_extra"])
        a.update(over)
        S_ = cs["S"]
        zb, zv = _guarded(R * S_)
        eb, ze = _guarded(R)
        rc = lib.nsa_sample_rays(ptr(t["rays_o"]), ptr(t["rays_d"]), ptr(t["z"]), ptr(t["sdf"]), ptr(t["far"]), ptr(self.voxels), a["voxel_res"],
                                 R, a["E"], a["N"], ptr(self.u), ptr(self.extra), a["n_extra"], cs["near"],
                                 ptr(self.eik) if with_eik else None, ptr(zv), ptr(ze) if with_eik else None, st())
        torch.cuda.synchronize()
        return rc, zv.cpu().reshape(R, S_), (ze.cpu() if with_eik else None), _guards_ok(zb) and _guards_ok(eb)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _recover(cs, zv):
    """remove near, far[ray] and the picked coarse samples from every sorted row, bit-exactly and as a multiset -> [R,N], sample
    j = 0 ... N - 1 in order.  (Where a sample equals an extra bit for bit either removal leaves the same remainder.)"""
    ex = S.extras(cs["z"], cs["far"], cs["near"], cs["extra_idx"])
    out = torch.empty(cs["R"], cs["N"])
    for r in range(cs["R"]):
        row = zv[r].tolist()
        for v in ex[r].tolist():
            i = bisect.bisect_left(row, v)
            assert i < len(row) and row[i] == v, f"{cs['name']} ray {r}: the row does not hold the extra {v!r} (again)"
            del row[i]
        out[r] = torch.tensor(row)
    return out


def _exact(cs, dc):
    """the conditions without a tolerance -> z_vals [R,S]"""
    name, R, S_, E = cs["name"], cs["R"], cs["S"], cs["E"]
    rc, zv, ze, guards = dc.call()
    assert rc == NSA_OK, (name, rc)
    assert guards, f"{name}: a guard word was written"
    assert bool(torch.isfinite(zv).all()) and bool(torch.isfinite(ze).all()), f"{name}: an output is not finite"
    assert bool((zv[:, 1:] >= zv[:, :-1]).all()), f"{name}: a row is not sorted"
    lo = torch.minimum(torch.full((R,), cs["near"]), cs["z"][:, 0])
    hi = torch.maximum(cs["far"], cs["z"][:, E - 1])
    assert bool((zv >= lo[:, None]).all()) and bool((zv <= hi[:, None]).all()), f"{name}: a sample outside the ray's range"
    pick = S.clamp_idx(cs["eik_idx"], S_)
    assert _same(ze, zv[torch.arange(R), pick]), f"{name}: z_eik is not z_vals[ray, clamp(eik_idx)]"
    rc2, zv2, ze2, g2 = dc.call(with_eik=False)
    assert rc2 == NSA_OK and g2 and _same(zv2, zv), f"{name}: the call without z_eik differs"
    rc3, zv3, ze3, g3 = dc.call()
    assert rc3 == NSA_OK and g3 and _same(zv3, zv) and _same(ze3, ze), f"{name}: two calls differ"
    if R > 1:
        # a permuted batch, and rays alone (the first, one carrying an edge, the last)
        perm = torch.randperm(R, generator=torch.Generator().manual_seed(R + E))
        _rc, zvp, zep, gp = DevCase(cs, perm).call()
        assert gp and _same(zvp, zv[perm]) and _same(zep, ze[perm]), f"{name}: a permuted batch changes a ray's row"
        for r in sorted({0, R - 1, *list(cs["edges"])[:3]}):
            _rc, zv1, ze1, g1 = DevCase(cs, torch.tensor([r])).call()
            assert g1 and _same(zv1[0], zv[r]) and _same(ze1, ze[r:r + 1]), f"{name}: ray {r} alone differs from the batch"
    return zv


@pytest.mark.parametrize("cls", [c for c, _ in C.E_CLASSES])
def test_sample_rays_vs_float64(cls, capsys):
    fails, pools, lines, share = [], {f: Pool() for f in range(5)}, [], {f: [0, 0] for f in range(5)}
    for E in dict(C.E_CLASSES)[cls]:
        for cs, s64, s32, sko in C.evaluated(E):
            zv = _exact(cs, DevCase(cs))
            z_got = _recover(cs, zv)
            keep = C.determinate(cs, s64)
            # the samples outside the z-space gate: inside the float64 sample's bin or an adjacent one
            b = s64.below
            lo = torch.gather(s64.bins, 1, (b - 1).clamp(min=0))
            hi = torch.gather(s64.bins, 1, (b + 2).clamp(max=E - 1))
            inside = (z_got.double() >= lo) & (z_got.double() <= hi)
            assert bool(inside[~keep].all()), f"{cs['name']}: a sample outside the z-space gate left its bin's neighbourhood"
            lines.append(f"  {cs['name']:<44s} left out of the z-space gate {1.0 - float(keep.double().mean()):.4f}")
            for f in cs["family"].unique().tolist():
                share[f][0] += int((~keep[cs["family"] == f]).sum())
                share[f][1] += int((cs["family"] == f).sum()) * cs["N"]
            C.add_rows(pools, cs, s64, s32, sko, z_got)
    with capsys.disabled():
        print(f"\n  nsa_sample_rays, {cls}: {len(lines)} cases pooled per family\n" + "\n".join(lines))
        for f, pool in pools.items():
            pool.judge(f"{cls}, {C.FAMILIES[f]}: ", fails)
            print(f"  {cls}, {C.FAMILIES[f]}: {share[f][0]} of {share[f][1]} samples ({share[f][0] / share[f][1]:.4f}) left out of the z-space gate")
    assert not fails, [f["what"] for f in fails]


def test_entry_point_limits():
    """at their exact values: S = 256 accepted, 257 refused; E = 3328 accepted, 3329 and 1 refused; voxel_res 0 and 1025 refused; a
    refused call writes nothing"""
    def refused(dc, **over):
        rc, zv, ze, guards = dc.call(**over)
        return rc == NSA_EBADARG and guards and bool(torch.isnan(zv).all()) and bool(torch.isnan(ze).all())

    def accepted(dc, **over):
        rc, zv, ze, guards = dc.call(**over)
        return rc == NSA_OK and guards and bool(torch.isfinite(zv).all()) and bool(torch.isfinite(ze).all())

    top = C.case(3328, 250, 4, 3, 7, 0.0, seed=1)                   # E and S at their maxima
    dc = DevCase(top)
    assert accepted(dc)
    assert refused(dc, N=251) and refused(dc, n_extra=5)            # S = 257 (the output buffers are sized for 256: nothing may be written)
    assert refused(dc, voxel_res=0) and refused(dc, voxel_res=1025)
    assert refused(dc, E=1)
    big = dict(top)                                                 # E = 3329: one more coarse sample per ray than the limit
    for k in ("z", "sdf"):
        big[k] = torch.cat([top[k], top[k][:, -1:] + (1.0 if k == "z" else 0.0)], 1).contiguous()
    big["E"] = 3329
    assert refused(DevCase(big))
    small = C.case(2, 1, 0, 1, 1, 0.0, seed=2)                      # the minima: E = 2, N = 1, no extras, one ray, one voxel
    assert accepted(DevCase(small))
