"""tests/sampler_ref64.py and tests/sampler_cases.py held without a GPU: what tests/test_sampler_float64_gpu.py relies on.

  * the fp32 mode of the restatement, fed the oracle's own coarse samples and SDF values, reproduces oracle/render_ref.py::importance_z
    bit for bit on the eight goldens of tests/test_sampler_gpu.py (eval-mode linspace extras and training-mode drawn extras);
  * the second fp32 yardstick (kernel order) stays within the gate factors of the first against float64, on the GPU test's inputs;
  * hand cases with known answers;
  * the conditions the GPU gates rest on, from the float64 restatement alone: the share of determinate samples, the paths that are
    taken (den = 1 branch, u = 0 and u = 1, heavy bins, ties, weight in the tail thread's bins)."""
import pytest
import torch

import sampler_cases as C
import sampler_ref64 as S
from helpers import load, tt, params_of, oracle_config, draws_of
from gate64 import Pool

F32 = torch.float32
GOLDENS = ["full_tracking", "full_tracking_poisson", "full_mapping", "full_vis_eval", "full_tracking_rw", "full_mapping_rw",
           "full_tracking_7scenes", "full_mapping_7scenes"]


@pytest.mark.parametrize("name", GOLDENS)
def test_fp32_mode_is_the_oracle_bit_for_bit(name):
    from oracle import render_ref as R
    fx = load(name)
    cfg, params, draws = oracle_config(fx), params_of(fx), draws_of(fx)
    training = bool(fx["meta_training"])
    pose = R.camera_from_tensor(tt(fx["in_cam"]))
    d, o = R.camera_rays(tt(fx["in_uv"]), pose if pose.dim() == 3 else pose.unsqueeze(0), tt(fx["in_K"]))
    n = d.shape[1]
    d, o = d.reshape(-1, 3).contiguous(), o.unsqueeze(1).repeat(1, n, 1).reshape(-1, 3).contiguous()
    voxels = tt(fx["in_voxels"])
    aux = {}
    z_all, z_eik = R.importance_z(params, cfg, d, o, voxels, training, draws, aux=aux)
    z, near, far = R.uniform_z(cfg, d, o, training, draws.get("t_rand"))
    pts = (o.unsqueeze(1) + z.unsqueeze(2) * d.unsqueeze(1)).reshape(-1, 3)
    with torch.no_grad():
        sdf = R.sdf_vals(params, cfg, pts).reshape(z.shape)
    E = z.shape[1]
    extra = None
    if cfg.n_samples_extra > 0:
        extra = draws["extra_idx"] if training else torch.linspace(0, E - 1, cfg.n_samples_extra).long()
    got = S.sample(z.contiguous(), sdf.contiguous(), far.reshape(-1).contiguous(), o, d, voxels.reshape(-1).contiguous(), cfg.voxel_res,
                   cfg.n_samples, extra, draws["eik_idx"], float(cfg.near), dtype=F32)
    assert torch.equal(got.bins, aux["bins"]) and torch.equal(got.cdf, aux["cdf"])
    assert torch.equal(got.z_all, z_all) and torch.equal(got.z_eik, z_eik.reshape(-1))
    assert got.z_all.dtype == F32 and got.z_imp.shape == (z.shape[0], cfg.n_samples)


def _rows(cs, s64, z_imp):
    u, u64, z, z64, norm = C.sample_rows(cs, s64, z_imp)
    return u, u64, z, z64, norm


@pytest.mark.parametrize("cls", [c for c, _ in C.E_CLASSES])
def test_kernel_order_within_the_gate_factors_of_the_reference_order(cls, capsys):
    """per (family, E class), pooled over the cases: the kernel-order fp32 evaluation judged as if it were a kernel, against the
    reference-order one -- rms <= 1.5 x, max <= 3 x -- in u-space on every sample and in z-space on the determinate ones"""
    fails, pools = [], {f: Pool() for f in range(5)}
    for E in dict(C.E_CLASSES)[cls]:
        for cs, s64, s32, sko in C.evaluated(E):
            u_o, u_64, z_o, z_64, norm = _rows(cs, s64, sko.z_imp)
            u_r, _, z_r, _, _ = _rows(cs, s64, s32.z_imp)
            keep = C.determinate(cs, s64).reshape(-1)
            fam = cs["family"][:, None].expand(-1, cs["N"]).reshape(-1)
            for f in fam.unique().tolist():
                m = fam == f
                pools[f].add("u-space, every sample", u_o[m], u_64[m], u_r[m], torch.ones_like(norm[m]))
                if bool((m & keep).any()):
                    pools[f].add("z-space, determinate samples", z_o[m], z_64[m], z_r[m], norm[m], keep[m])
    with capsys.disabled():
        print(f"\n  kernel order (as e_k) against reference order (as e_32), {cls}")
        for f, pool in pools.items():
            pool.judge(f"{cls}, {C.FAMILIES[f]}: ", fails)
    assert not fails, [f["what"] for f in fails]


def _hand(z, sdf, far, N, extra=None, eik=None, near=0.0, dtype=torch.float64):
    R = z.shape[0]
    o, d = torch.zeros(R, 3), torch.tensor([[0.0, 0.0, 0.1]]).repeat(R, 1)
    return S.sample(z, sdf, far, o, d, torch.zeros(1), 1, N, extra, eik, near, dtype=dtype)


def test_hand_cases():
    # E = 2: one bin of mass 1; the samples are z0 + u (z1 - z0)
    z, far = torch.tensor([[0.25, 1.75]]), torch.tensor([2.0])
    for sdf in (torch.tensor([[0.3, 0.3]]), torch.tensor([[-0.01, 0.2]])):
        for dtype in (torch.float64, F32):
            s = _hand(z, sdf, far, 5, dtype=dtype)
            assert torch.equal(s.cdf, torch.tensor([[0.0, 1.0]], dtype=dtype))
            assert torch.equal(s.z_imp, (0.25 + S.u_lin(5).to(dtype) * 1.5)[None])           # (exact: 0.25 + k 0.375)
            assert s.z_all[0].tolist() == [0.0, 0.25, 0.625, 1.0, 1.375, 1.75, 2.0]
            k = S.kernel_order(z, sdf, far, torch.zeros(1, 3), torch.tensor([[0.0, 0.0, 0.1]]), torch.zeros(1), 1, 5, None, None, 0.0)
            assert torch.equal(k.z_imp, s.z_imp.float()) and torch.equal(k.z_all, s.z_all.float())
    # N = 1: u = [0], the sample is z0 whatever the density; with the extras and a clamped eikonal pick
    z = torch.tensor([[0.5, 1.0, 1.5, 2.0]])
    s = _hand(z, torch.tensor([[0.2, 0.01, -0.2, -0.4]]), far, 1, extra=torch.tensor([3, 7, -1, 1]), eik=torch.tensor([99]), near=0.125)
    assert s.z_imp.tolist() == [[0.5]] and s.z_all[0].tolist() == [0.125, 0.5, 1.0, 2.0, 2.0, 2.0, 2.0] and s.z_eik.tolist() == [2.0]
    assert _hand(z, torch.tensor([[0.2, 0.01, -0.2, -0.4]]), far, 1, eik=torch.tensor([-5])).z_eik.tolist() == [2.0]
    # a cdf that saturates: a wall between samples 1 and 2 takes all the weight in bin 2, every other bin sits on the floor
    z, far = torch.linspace(0.0, 4.0, 12)[None].contiguous(), torch.tensor([4.0])
    sdf = (0.5 - z) * 5.0
    s = _hand(z, sdf, far, 18)
    mass = s.cdf[0, 1:] - s.cdf[0, :-1]
    assert float(mass[2]) > 0.999 and bool((mass[:2] < 1e-5).all()) and bool((mass[3:] < 1e-5).all())
    assert float(s.cdf[0, -1]) == pytest.approx(1.0, abs=1e-12)
    assert bool(((s.z_imp[0, 1:-1] >= z[0, 2]) & (s.z_imp[0, 1:-1] <= z[0, 3])).all())       # every interior sample inside bin 2
    # u = 1: the last cdf entry is 1 or 1 + an ulp; the sample is the last coarse z or within the floor bins just below it, the same
    # point in u-space (1e-5 of mass a bin)
    assert float(s.z_imp[0, -1]) == 4.0 or float(S.cdf_at64(s.z_imp, s.bins, s.cdf)[0, -1]) > 1 - 1e-5
    s32 = _hand(z, sdf, far, 18, dtype=F32)
    du = (S.cdf_at64(s32.z_imp, s.bins, s.cdf) - S.cdf_at64(s.z_imp, s.bins, s.cdf)).abs()
    assert float(du.max()) <= 1.01e-5
    # the float64 cdf inverts the float64 samples: u-space error of the algorithm itself is at most the floor
    u = S.u_lin(18).double()[None]
    assert float((S.cdf_at64(s.z_imp, s.bins, s.cdf) - u).abs().max()) <= 1.0e-5


def test_index_rules():
    assert S.clamp_idx(torch.tensor([0, 4, 5, -1, -2 ** 31, 2 ** 31 - 1], dtype=torch.int32), 5).tolist() == [0, 4, 4, 4, 4, 4]
    z = torch.tensor([[1.0, 2.0, 3.0]])
    assert S.extras(z, torch.tensor([9.0]), 0.5, None).tolist() == [[0.5, 9.0]]
    assert S.extras(z, torch.tensor([9.0]), 0.5, torch.tensor([1, 1, 3, -7])).tolist() == [[0.5, 9.0, 2.0, 2.0, 3.0, 3.0]]


@pytest.mark.parametrize("E", C.E_ALL)
def test_cases_take_every_path_and_leave_out_little(E, capsys):
    """from the float64 restatement alone, case by case: everything finite; the share of (ray, j) outside the z-space gate is at most
    10 % (N >= 94; below that 1 / N + 10 %, the u = 1 column being 1 / N on its own); samples on the den = 1 branch; u = 0 and, for
    N >= 2, u = 1; at E > 256 a ray with more than half of its weight in the bins of the thread that owns the last bin; bit-equal keys
    in the rows of the tie cases"""
    lines, on_floor = [], False
    for cs, s64, s32, sko in C.evaluated(E):
        N, R = cs["N"], cs["R"]
        for t in (cs["z"], cs["sdf"], cs["far"], cs["rays_o"], cs["rays_d"], cs["voxels"], s64.z_all, s64.cdf, s32.z_all, sko.z_all):
            assert bool(torch.isfinite(t).all()), cs["name"]
        assert bool((cs["z"][:, 1:] >= cs["z"][:, :-1]).all())
        left = 1.0 - float(C.determinate(cs, s64).double().mean())
        lines.append(f"  {cs['name']:<44s} left out of the z-space gate {left:.4f} (cap {C.left_out_cap(N):.4f})")
        assert left <= C.left_out_cap(N), (cs["name"], left)
        on_floor = on_floor or bool((s64.den < S.DEN_MIN).any())
        # (N = 1 is the single sample u = 0, and with E <= 5 a ray may have no bin on the floor at all: there the E's cases together)
        assert N == 1 or E <= 5 or bool((s64.den < S.DEN_MIN).any()), f"{cs['name']}: no sample on the den = 1 branch"
        u = S.u_lin(N)
        assert float(u[0]) == 0.0 and (N == 1 or float(u[-1]) == 1.0)
        # ties: near, far and the picked coarse samples hold bit-equal keys whenever a pick repeats (n_extra >= 4) or z[0] == near
        ex = S.extras(cs["z"], cs["far"], cs["near"], cs["extra_idx"])
        if cs["n_extra"] >= 4:
            assert all(len(set(row.tolist())) < ex.shape[1] for row in ex), f"{cs['name']}: no two bit-equal keys"
        if E > 256 and R == 67:
            lo, hi = C.tail_bins(E)
            w, _cdf = S.pdf_cdf(*C.args(cs)[:2], *C.args(cs)[3:7])
            share = w[:, lo:hi].sum(1) / w.sum(1)
            prefix = 1.0 - w[:, lo:hi].sum(1) / w.sum(1)
            assert float(share.max()) > 0.5, f"{cs['name']}: no ray with half of its weight in bins {lo} .. {hi - 1}"
            r = int(share.argmax())
            assert cs["edges"].get(r) == "tail" and 0.05 < float(prefix[r]) < 0.5      # (behind a prefix that is not negligible)
    assert on_floor, f"E = {E}: no sample on the den = 1 branch"
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_every_family_is_met_at_every_class_and_surfaces_have_heavy_bins():
    for cls, es in C.E_CLASSES:
        heavy, seen, near_tie, res_seen, r_seen = set(), set(), 0, set(), set()
        for E in es:
            for cs, s64, _s32, _sko in C.evaluated(E):
                mass = (s64.cdf[:, 1:] - s64.cdf[:, :-1]).amax(1)
                for f in range(5):
                    m = cs["family"] == f
                    if bool(m.any()):
                        seen.add(f)
                        if float(mass[m].max()) > 0.1:
                            heavy.add(f)
                near_tie += int((cs["z"][:, 0] == cs["near"]).sum())
                res_seen.add(cs["voxel_res"])
                r_seen.add(cs["R"])
        assert seen == set(range(5)), (cls, seen)
        if es[0] < 3328:                    # (at E = 3328 a crossing spreads over a hundred bins: the heaviest holds a few per cent)
            assert set(C.SURFACE) <= heavy, (cls, heavy)
        assert near_tie > 0 and res_seen == set(C.RES_ALL) and r_seen == set(C.R_ALL), (cls, near_tie, res_seen, r_seen)
    shapes = {(N, x) for N, x in C.SHAPES}
    assert {N + 2 + x for N, x in shapes} >= {3, 4, 5, 98, 127, 128, 129, 192, 255, 256}
    assert {(N + 2 + x) % 4 for N, x in shapes} == {0, 1, 2, 3} and any(N == 1 for N, _ in shapes)
