"""The operands of the MLP suites (tests/test_gemm_float64_gpu.py, tests/bf16_cases.py and, for single builders,
tests/test_grid_float64_gpu.py), built on the CPU from seeds (test infrastructure).

Cotangent scales c_p = 2^U(-60, 40), neighbours alternating between 2^40 and 2^-60, some points all zero (exactly 0 out); each cotangent
alone and all three at independent scales; g_sdf alone at 2^20..2^40 (the accumulator of the feature GEMM then holds sbar ws while its
operand vector is zero).  Points are explicit fp32 (colour kernels: one sample per ray at z = 0, so x = o exactly), identical for
kernel and references."""
import torch

N_BIG = 16411                                   # ragged (16411 = 512 x 32 + 27)
SMALL_P = (1, 15, 17, 31, 33, 4097)
KINK = 2e-6                                     # colour ReLU margin left out on both sides (as tests/test_configs_gpu.py)


def cube_points(n, seed):
    """uniform in the cube, an eighth of them within 1e-3 of a face (some exactly on it)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.999
    m = n // 8
    i, face = torch.arange(m), torch.randint(3, (m,), generator=g)
    x[i, face] = torch.sign(x[i, face]) * (1 - torch.rand(m, generator=g) * 1e-3)
    x[i[::17], face[::17]] = torch.sign(x[i[::17], face[::17]])
    return x[torch.randperm(n, generator=g)].contiguous()


def scales(n, seed, alternate=True, zeros=True):
    """c_p = 2^U(-60, 40); within the first half neighbours alternate 2^40 / 2^-60; every 97th point 0"""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-60, 41, (n,), generator=g).double()
    if alternate:
        h = torch.arange(n // 2)
        e[h] = torch.where(h % 2 == 0, 40.0, -60.0).double()
    c = torch.exp2(e)
    if zeros:
        c[torch.arange(n) % 97 == 5] = 0.0
    return c


def cot(n, seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n,) + shape, generator=g)


def scaled(base, c):
    return (base.double() * c.reshape((-1,) + (1,) * (base.dim() - 1))).float()


def sdf_families(n):
    """name -> (g_sdf, g_feat, g_grad, c_p): cotangents of O(1) random base values times per-point scales"""
    base = (cot(n, 10, ()), cot(n, 11, (64,)), cot(n, 12, (3,)))
    c = scales(n, 13)
    fam = {"all three x c_p": tuple(scaled(b, c) for b in base) + (c,)}
    for i, name in enumerate(("g_sdf", "g_feat", "g_grad")):
        fam[name + " alone x c_p"] = tuple(scaled(b, c) if j == i else None for j, b in enumerate(base)) + (c,)
    cs = [scales(n, 20 + i, alternate=(i == 1)) for i in range(3)]
    fam["independent scales per input"] = tuple(scaled(b, ci) for b, ci in zip(base, cs)) + (torch.stack(cs).amax(0),)
    g = torch.Generator().manual_seed(30)
    ca = torch.exp2(torch.randint(20, 41, (n,), generator=g).double())
    fam["g_sdf alone at 2^20..2^40 (features, normals NULL)"] = (scaled(base[0], ca), None, None, ca)
    return fam


def colour_inputs(net, n, seed):
    """points, view directions and the fine network's fp32 normals and features there (net: anything with .params and .cfg)"""
    from oracle import render_ref as R
    x = cube_points(n, seed)
    g = torch.Generator().manual_seed(seed + 1)
    _s, feat, grad = R.sdf_outputs(net.params, net.cfg, x.clone(), "fine")
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * (0.6 + 0.8 * torch.rand(n, 1, generator=g))
    return x, d.contiguous(), grad.detach().contiguous(), feat.detach().contiguous()
