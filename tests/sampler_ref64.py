"""A float64 restatement of the per-ray importance sampler k_sample_rays (csrc/render_sampler.hip, entry point nsa_sample_rays) -- test
infrastructure.  Plain torch with a ``dtype`` argument: float64 is the reference, float32 evaluates the same graph in fp32 (the
reference-order yardstick of tests/test_sampler_float64_gpu.py; tests/test_sampler_ref64_cpu.py holds that mode bit for bit to
oracle/render_ref.py::importance_z).  ``kernel_order`` is a second fp32 evaluation in the kernel's documented operation order.

The inputs are the kernel's own: z [R,E] ascending, sdf [R,E], far [R], rays_o / rays_d [R,3], the visit counter voxels [res^3], N,
extra_idx [n_extra] or None, eik_idx [R] or None, near.  There is no network in it.

What is DISCRETE is taken from the fp32 inputs and enters as data (as tests/grid_ref64.py and tests/objective_ref64.py do): the point
x = o + z d in fp32 with a separate multiply and add, the out-of-range test |x| > 0.99 on it and the truncated voxel index.  The
u_j = linspace(0, 1, N) are the fp32 ones.  Everything else is promoted to ``dtype``.

Index rules (the kernel's): an extra index e with (uint32) e >= E reads sample E - 1 -- so does a negative one --; an eikonal index
with (uint32) e >= S reads the last sample of the sorted row."""
from collections import namedtuple

import torch

import objective_ref64 as O

F64, F32 = torch.float64, torch.float32
FLOOR = 1e-5                  # added to every weight but the last: ray_sampler.py:116
DEN_MIN = 1e-5                # a chosen bin below this mass is sampled with den = 1: ray_sampler.py:136
EXPM1_FROM_E = 1024           # k_sample_rays: beyond this many coarse samples alpha = -expm1f(-en), up to it 1 - expf(-en)

Samples = namedtuple("Samples", "z_imp z_all z_eik bins cdf den below")


def u_lin(N):
    return torch.linspace(0.0, 1.0, steps=N)


def clamp_idx(idx, n):
    """(uint32) i < n ? i : n - 1"""
    idx = idx.long()
    return torch.where((idx >= 0) & (idx < n), idx, torch.full_like(idx, n - 1))


def extras(z, far, near, extra_idx):
    """[R, 2 + n_extra] fp32: near, far[ray], z[ray, clamp(extra_idx)] -- the keys the kernel merges with the N samples"""
    R, E = z.shape
    cols = [torch.full((R, 1), float(near), dtype=F32), far.reshape(R, 1)]
    if extra_idx is not None and len(extra_idx):
        cols.append(z[:, clamp_idx(extra_idx, E)])
    return torch.cat(cols, -1)


def pdf_cdf(z, sdf, rays_o, rays_d, voxels, voxel_res, dtype=F64):
    """-> w [R,E-1] (the weights before the floor), cdf [R,E]; oracle/render_ref.py::volume_weights and importance_z lines 437-440"""
    assert all(t.dtype == F32 for t in (z, sdf, rays_o, rays_d, voxels))
    R, E = z.shape
    res = int(voxel_res)
    beta = O.beta_of(O.visit_counts(O.sample_points(z, rays_o, rays_d), voxels.reshape(res, res, res), res), dtype)
    zz = z.to(dtype)
    sigma = O.density(sdf.to(dtype), beta)
    dists = torch.cat([zz[:, 1:] - zz[:, :-1], torch.full((R, 1), 1e10, dtype=dtype)], -1)
    energy = dists * sigma
    shifted = torch.cat([torch.zeros(R, 1, dtype=dtype), energy[:, :-1]], dim=-1)
    alpha = -torch.exp(-energy) + 1
    w = (alpha * torch.exp(-torch.cumsum(shifted, dim=-1)))[:, :-1]
    pdf = w + FLOOR
    pdf = pdf / torch.sum(pdf, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    return w, torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)


def _invert(zz, cdf, u):
    """importance_z lines 442-451 -> z_imp [R,N], den [R,N] (the chosen bin's mass, before the den < 1e-5 switch), below [R,N]"""
    inds = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cdf_b, cdf_a = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bin_b, bin_a = torch.gather(zz, 1, below), torch.gather(zz, 1, above)
    den = cdf_a - cdf_b
    denom = torch.where(den < DEN_MIN, torch.ones_like(den), den)
    t = (u - cdf_b) / denom
    return bin_b + t * (bin_a - bin_b), den, below


def _merge(z_imp, z, far, near, extra_idx, eik_idx):
    z_all, _ = torch.sort(torch.cat([z_imp, extras(z, far, near, extra_idx).to(z_imp.dtype)], -1), -1)
    z_eik = None
    if eik_idx is not None:
        z_eik = torch.gather(z_all, 1, clamp_idx(eik_idx, z_all.shape[1]).unsqueeze(-1))[:, 0]
    return z_all, z_eik


def sample(z, sdf, far, rays_o, rays_d, voxels, voxel_res, N, extra_idx, eik_idx, near, dtype=F64):
    """-> Samples(z_imp [R,N] in j order, z_all [R,S] sorted, z_eik [R] or None, bins [R,E], cdf [R,E], den [R,N], below [R,N])"""
    R, E = z.shape
    _w, cdf = pdf_cdf(z, sdf, rays_o, rays_d, voxels, voxel_res, dtype)
    zz = z.to(dtype)
    u = u_lin(N).to(dtype).unsqueeze(0).repeat(R, 1).contiguous()
    z_imp, den, below = _invert(zz, cdf, u)
    z_all, z_eik = _merge(z_imp, z, far, near, extra_idx, eik_idx)
    return Samples(z_imp, z_all, z_eik, zz, cdf, den, below)


def cdf_at64(z, bins, cdf):
    """The float64 piecewise-linear cdf at z (oracle/render_ref.py::cdf_at in float64): sample sets are compared in u-space"""
    z, bins, cdf = z.to(F64).contiguous(), bins.to(F64).contiguous(), cdf.to(F64)
    idx = torch.clamp(torch.searchsorted(bins, z, right=True) - 1, 0, bins.shape[1] - 2)
    b0, b1 = torch.gather(bins, 1, idx), torch.gather(bins, 1, idx + 1)
    c0, c1 = torch.gather(cdf, 1, idx), torch.gather(cdf, 1, idx + 1)
    t = torch.clamp((z - b0) / torch.clamp(b1 - b0, min=1e-20), 0, 1)
    return c0 + t * (c1 - c0)


# ------------------------------------------------------------------------------------------------------------------ kernel order
def _block_excl_scan(v):
    """block_excl_scan of the kernel on v [R,256] fp32 -> exclusive prefix [R,256], total [R]: the shuffle-up inclusive scan of each
    wave (off = 1, 2, ... 32, lanes >= off add), exclusive = the previous lane's inclusive, the wave totals added in wave order,
    total = ((r0 + r1) + r2) + r3"""
    R = v.shape[0]
    incl = v.reshape(R, 4, 64).clone()
    lane = torch.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        up = torch.cat([torch.zeros(R, 4, off, dtype=F32), incl[:, :, :-off]], -1)
        incl = torch.where(lane >= off, incl + up, incl)
    red = incl[:, :, 63]
    prev = torch.cat([torch.zeros(R, 4, 1, dtype=F32), incl[:, :, :-1]], -1)
    base = torch.zeros(R, 4, dtype=F32)
    for w in range(1, 4):
        base[:, w] = base[:, w - 1] + red[:, w - 1]
    excl = torch.where(lane == 0, base[:, :, None].expand(-1, -1, 64), base[:, :, None] + prev)
    total = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    return excl.reshape(R, 256), total


def kernel_order(z, sdf, far, rays_o, rays_d, voxels, voxel_res, N, extra_idx, eik_idx, near):
    """A second fp32 evaluation, in the order k_sample_rays documents, statement by statement: thread-blocked partial sums with
    per = ceil(E / 256), block_excl_scan, ``run`` / ``nrun`` continued sequentially inside a thread, q = pdf / ptot, cdf[i + 1] = nrun,
    the kernel's binary search.  expf / expm1f are torch's fp32 ones and the compiler may contract a multiply and an add that stand
    apart here: a yardstick, not a bit-exact trace.  -> Samples (den as the kernel sees it)"""
    assert all(t.dtype == F32 for t in (z, sdf, far, rays_o, rays_d, voxels))
    R, E = z.shape
    res = int(voxel_res)
    f = lambda v: torch.tensor(v, dtype=F32)
    count = O.visit_counts(O.sample_points(z, rays_o, rays_d), voxels.reshape(res, res, res), res)
    beta = f(O.BETA_A) * torch.exp((f(-O.BETA_B) * f(0.0001)) * count * f(O.BETA_D)) + f(O.BETA_C)
    sigma = (1.0 / beta) * (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() / beta))
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, dtype=F32)], -1)
    per = (E + 255) // 256
    pad = 256 * per - E
    blocked = lambda t: torch.nn.functional.pad(t, (0, pad)).reshape(R, 256, per)
    en = blocked(delta * sigma)                                        # pdf[i] after the first phase; 0 beyond E
    idx = torch.arange(256 * per).reshape(256, per)
    is_bin = (idx + 1 < E)[None]                                       # i + 1 < E: a bin of the pdf
    esum = torch.zeros(R, 256, dtype=F32)
    for k in range(per):
        esum = esum + en[:, :, k]
    run, _tot = _block_excl_scan(esum)
    p = torch.zeros(R, 256, per, dtype=F32)
    psum = torch.zeros(R, 256, dtype=F32)
    for k in range(per):
        alpha = -torch.expm1(-en[:, :, k]) if E > EXPM1_FROM_E else 1.0 - torch.exp(-en[:, :, k])
        w = alpha * torch.exp(-run)
        run = run + en[:, :, k]
        p[:, :, k] = torch.where(is_bin[:, :, k], w + f(FLOOR), torch.zeros_like(w))
        psum = psum + p[:, :, k]
    _excl, ptot = _block_excl_scan(psum)
    q = torch.where(is_bin, p / ptot[:, None, None], torch.zeros_like(p))
    nsum = torch.zeros(R, 256, dtype=F32)
    for k in range(per):
        nsum = nsum + q[:, :, k]
    nrun, _ntot = _block_excl_scan(nsum)
    upper = torch.zeros(R, 256, per, dtype=F32)                        # cdf[i + 1]
    for k in range(per):
        nrun = nrun + q[:, :, k]
        upper[:, :, k] = nrun
    cdf = torch.cat([torch.zeros(R, 1, dtype=F32), upper.reshape(R, -1)[:, :E - 1]], -1)
    # the kernel's search: first index in [0, E] with cdf > u
    u = u_lin(N).unsqueeze(0).repeat(R, 1)
    lo, hi = torch.zeros(R, N, dtype=torch.long), torch.full((R, N), E, dtype=torch.long)
    while bool((lo < hi).any()):
        active = lo < hi
        mid = (lo + hi) >> 1
        right = torch.gather(cdf, 1, mid.clamp(max=E - 1)) <= u
        lo = torch.where(active & right, mid + 1, lo)
        hi = torch.where(active & ~right, mid, hi)
    below = torch.clamp(lo - 1, min=0)
    above = torch.clamp(lo, max=E - 1)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(z, 1, below), torch.gather(z, 1, above)
    den = c1 - c0
    denom = torch.where(den < DEN_MIN, torch.ones_like(den), den)
    z_imp = b0 + ((u - c0) / denom) * (b1 - b0)
    z_all, z_eik = _merge(z_imp, z, far, near, extra_idx, eik_idx)
    return Samples(z_imp, z_all, z_eik, z, cdf, den, below)
