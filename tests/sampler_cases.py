"""The inputs of tests/test_sampler_float64_gpu.py (test infrastructure), built on the CPU from seeds so that
tests/test_sampler_ref64_cpu.py can check on the very same tensors what the GPU gates rely on: the share of determinate samples, the
paths that are taken, the ties.  Everything is finite.

Five ray families, interleaved ray by ray (family = (ray + offset) mod 5; the offset of a case with one or three rays is chosen so
that the case holds a crossing ray): a plane crossed at 0.3 - 0.8 of the ray at incidence cos 0.2 - 1; a miss (sdf 0.3 - 0.4); a grazing
ray (least sdf about 0.5 beta); a broad, fuzzy density (0.05 |s| + 3 beta U); a crossing inside voxels visited up to 30 000 times.
Edges sit on known rays (``edge_rays``).  The visit counter is not symmetric under any permutation of its three indices."""

import torch

import objective_ref64 as O

FAMILIES = ("crossing", "miss", "grazing", "broad", "crossing, visited voxels")
SURFACE = (0, 4)                                # the families whose rays cross a surface
EDGES = ("zero_sdf", "neg_run", "equal_z", "beyond", "exact099", "last_inside", "tail")
# per = ceil(E / 256) changes at 256 / 257, 512 / 513, 1024 / 1025; at 1024 / 1025 the kernel's alpha changes form as well
E_ALL = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513, 640, 1023, 1024, 1025, 3328)
E_CLASSES = (("E 2-5", (2, 3, 4, 5)), ("E 63-65", (63, 64, 65)), ("E 255-257", (255, 256, 257)),
             ("E 511-1025", (511, 513, 640, 1023, 1024, 1025)), ("E 3328", (3328,)))
# (N, n_extra) -> S = N + 2 + n_extra: 3, 4, 5, 7, 96, 98 (the shipped one), 127, 128 | 129 (the sort changes form), 192, 255, 256;
# S mod 4 = 1, 2, 3 occur; n_extra = 0 is called with extra_idx = NULL; N = 1 is u = [0]
SHAPES = ((1, 0), (2, 0), (2, 1), (5, 0), (94, 0), (94, 2), (120, 5), (94, 32), (94, 33), (158, 32), (250, 3), (250, 4))
R_ALL = (1, 3, 67)
RES_ALL = (1, 7, 64)
NEARS = (0.0, 0.05)
BETA0 = O.BETA_A + O.BETA_C                    # beta of an unvisited voxel
DETERMINATE = 2e-5                             # float64 bin mass from which fp32 and float64 take the same branch


def voxel_table(res):
    """[res^3] counts 0 .. 30 000 on the half ix < res / 2 (where the rays of family 4 live), 0 elsewhere.  20000 f(ix) + 7000 g(iy) +
    3000 h(iz) with three different f, g, h: a wrong index order changes the count of most points"""
    i = torch.arange(res, dtype=torch.float64)
    fx = (i + 1) / res
    gy = ((i * 7 + 3) % res) / res if res > 1 else torch.tensor([0.5], dtype=torch.float64)
    hz = (((i * 3 + 1) % res) / res) ** 2 if res > 1 else torch.tensor([0.25], dtype=torch.float64)
    v = (20000.0 * fx[:, None, None] + 7000.0 * gy[None, :, None] + 3000.0 * hz[None, None, :]).floor()
    v = v * (i[:, None, None] < res / 2)
    return v.float().reshape(-1).contiguous()


def edge_rays(R, E, calm=False):
    """{ray: edge}: R >= 32: rays 8 .. 14 and 40 .. 46 carry one edge each; smaller R: ray r >= 1 carries edge (r + E) mod 7 (ray 0 is
    the plain crossing ray every case holds)"""
    if R >= 32:
        out = {8 + k: e for k, e in enumerate(EDGES)}
        if not calm:
            out.update({40 + k: e for k, e in enumerate(EDGES)})
        return out
    return {r: EDGES[(r + E) % len(EDGES)] for r in range(1, R)}


def tail_bins(E):
    """the bins owned by the thread that owns the LAST bin E - 2 (thread-blocked, per = ceil(E / 256)).  At E = 513, 1023, 1024, 1025, 3328 this is
    the thread that also owns sample E - 1 -- whose free energy carries the 1e10 interval --; at E = 257, 511, 640 that sample sits alone
    in the thread after it, which owns no bin."""
    per = (E + 255) // 256
    t = (E - 2) // per
    return t * per, min(t * per + per, E - 1)


def family_offset(R, k):
    """ray 0 of a case with one or three rays is a crossing ray"""
    return (0, 4)[k % 2] if R <= 3 else k % 5


def extra_pattern(E, n_extra, g):
    """duplicates, 0 and E - 1, values >= E and negative ones first, then random picks"""
    fixed = [0, E - 1, E // 2, E // 2, E, -1, E + 5, 1 % E, -2 ** 31, 2 ** 31 - 1]
    more = torch.randint(0, E, (max(n_extra - len(fixed), 0),), generator=g).tolist()
    return torch.tensor((fixed + more)[:n_extra], dtype=torch.int32)


def eik_pattern(R, S, g):
    fixed = [0, S - 1, S, -1, S + 7, S // 2, -2 ** 31, 2 ** 31 - 1]
    more = torch.randint(0, S, (max(R - len(fixed), 0),), generator=g).tolist()
    return torch.tensor((fixed + more)[:R], dtype=torch.int32)


def case(E, N, n_extra, R, res, near, seed, offset=0, jitter=False, calm=False):
    """-> dict of CPU tensors (fp32 / int32): rays_o, rays_d [R,3], z [R,E] ascending, sdf [R,E], far [R], voxels [res^3], extra_idx
    [n_extra] or None, eik_idx [R], and family [R], edges {ray: name}.  z = near + (far - near) t with t = linspace (z[0] == near and, at
    near = 0, z[E - 1] == far bit for bit: ties with the extras) or, with ``jitter``, sorted uniform draws.  ``calm``: every ray but ray 0
    is of a family without a surface, a grazing one -- whose floor bins carry 1.0 - 1.4e-5 -- only every ninth (at N = 2 and 5 the u = 0 column is a half resp. a fifth of the samples, and on a crossing ray it
    sits in a floor bin -- outside the z-space gate; see ``left_out_cap``)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    fam = (torch.arange(R) + offset) % 5
    if calm:
        fam = torch.where(torch.arange(R) == 0, fam, torch.tensor((1, 3, 1, 3, 1, 3, 1, 3, 2))[torch.arange(R) % 9])
    o = (rnd(R, 3) - 0.5) * 0.4
    d = torch.nn.functional.normalize(rnd(R, 3) - 0.5, dim=-1) * 0.2
    side = torch.where(fam == 4, -1.0, 1.0).double()
    o[:, 0] = side * (0.5 + o[:, 0] * 0.5)                         # x_0 = +-(0.4 .. 0.6) + z d_0, |z d_0| <= 0.14
    d[:, 0] *= 0.2
    far = 1.0 + 2.5 * rnd(R)
    t = torch.sort(rnd(R, E), dim=-1)[0] if jitter else torch.linspace(0.0, 1.0, E, dtype=torch.float64).expand(R, E)
    edges = edge_rays(R, E, calm)
    for r, e in edges.items():
        if e == "tail" and jitter:                                 # (evenly spaced: the tail thread's bins must be able to hold the weight)
            t[r] = torch.linspace(0.0, 1.0, E, dtype=torch.float64)
        if e == "beyond":                                          # leaves |x| <= 0.99 along the ray (x_0 = 0.9 + 0.1 z)
            o[r] = torch.tensor([0.9, 0.2, 0.1], dtype=torch.float64)
            d[r] = torch.tensor([0.1, 0.02, -0.03], dtype=torch.float64)
        elif e == "exact099":                                      # x_0 = fp32(0.99), x_1 = -fp32(0.99) at every sample: inside, voxel
            o[r] = torch.tensor([0.99, -0.99, 0.3], dtype=torch.float64)       # indices res - 1 and 0
            d[r] = torch.tensor([0.0, 0.0, 0.1], dtype=torch.float64)
        elif e in ("neg_run", "tail"):
            far[r] = 3.5
    far = far.float()
    z = (near + (far.double()[:, None] - near) * t).float()
    zd, span = z.double(), (far.double() - near)[:, None]
    zc = near + (0.3 + 0.5 * rnd(R, 1)) * span
    slope = 0.2 * (0.2 + 0.8 * rnd(R, 1))                          # |d| cos
    cross = slope * (zc - zd)
    zg = near + (0.2 + 0.6 * rnd(R, 1)) * span
    graze = 0.5 * BETA0 + slope * (zd - zg).abs()
    broad = 0.05 * (zd - zc).abs() + 3.0 * BETA0 * rnd(R, E)
    miss = 0.3 + 0.1 * rnd(R, E)
    f = fam[:, None]
    sdf = torch.where((f == 0) | (f == 4), cross, torch.where(f == 1, miss, torch.where(f == 2, graze, broad)))
    lo, hi = tail_bins(E)
    for r, e in edges.items():
        if e == "zero_sdf":
            sdf[r, E // 2] = 0.0
        elif e == "neg_run":                                       # surface at 0.1 of the ray, then a run of sigma = 1 / beta: the free
            sdf[r] = 0.2 * (near + 0.1 * span[r] - zd[r])         # energy passes 104 and exp(-run) underflows in fp32
        elif e == "equal_z":
            z[r, min(E // 3 + 1, E - 1)] = z[r, E // 3]            # a bin of width 0
        elif e == "last_inside":                                   # empty space, the last sample inside: the 1e10 interval has the mass
            sdf[r] = miss[r]
            sdf[r, E - 1] = -0.05
        elif e == "tail":                                          # a thin haze (free energy about 0.2 over the ray), then the bins of the
            sdf[r] = 6.4 * BETA0                                   # last bin's thread deep inside: more than half of the weight is theirs,
            sdf[r, lo:] = -1.0                                     # behind a prefix that is not negligible
    S = N + 2 + n_extra
    c = lambda x: x.float().contiguous()
    return dict(rays_o=c(o), rays_d=c(d), z=z.contiguous(), sdf=c(sdf), far=far.contiguous(), voxels=voxel_table(res), voxel_res=res,
                N=N, n_extra=n_extra, extra_idx=extra_pattern(E, n_extra, g) if n_extra else None, eik_idx=eik_pattern(R, S, g),
                near=float(near), family=fam, edges=edges, R=R, E=E, S=S, name=f"E{E} N{N} x{n_extra} R{R} res{res} near{near:g}"
                + (" jitter" if jitter else ""))


def args(cs):
    """the arguments of sampler_ref64.sample / kernel_order"""
    return (cs["z"], cs["sdf"], cs["far"], cs["rays_o"], cs["rays_d"], cs["voxels"], cs["voxel_res"], cs["N"], cs["extra_idx"],
            cs["eik_idx"], cs["near"])


def cases_of(E):
    """every (N, n_extra) of SHAPES at this E; R, the counter's resolution, near, jitter and the family offset rotate with the case's
    number so that every value meets every E and every shape somewhere"""
    out = []
    e_no = E_ALL.index(E)
    for s_no, (N, n_extra) in enumerate(SHAPES):
        k = e_no * len(SHAPES) + s_no
        calm = N in (2, 5)
        R = 67 if calm else R_ALL[(e_no + s_no) % 3]
        out.append(case(E, N, n_extra, R, RES_ALL[(e_no + s_no // 3) % 3], NEARS[(e_no + s_no // 2) % 2], seed=1000 + k,
                        offset=0 if calm else family_offset(R, k), jitter=(k % 4 == 3), calm=calm))
    return out


def e_class(E):
    return next(name for name, es in E_CLASSES if E in es)


_EVALUATED = {}


def evaluated(E):
    """[(case, float64 Samples, fp32 reference-order Samples, fp32 kernel-order Samples)] of cases_of(E), computed once and shared"""
    import sampler_ref64 as S
    if E not in _EVALUATED:
        _EVALUATED[E] = [(cs, S.sample(*args(cs)), S.sample(*args(cs), dtype=torch.float32), S.kernel_order(*args(cs)))
                         for cs in cases_of(E)]
    return _EVALUATED[E]


def determinate(cs, s64):
    """[R,N] bool: the (ray, j) of the z-space gate -- float64 mass of the chosen bin >= 2e-5 and j < N - 1"""
    keep = s64.den >= DETERMINATE
    keep[:, cs["N"] - 1] = False
    return keep


def left_out_cap(N):
    """the share of (ray, j) a case may leave out of the z-space gate: 10 %; below N = 94 the u = 1 column alone is 1 / N more"""
    return 0.10 if N >= 94 else 1.0 / N + 0.10


def sample_rows(cs, s64, z_imp):
    """one set of N samples per ray against float64, sample by sample -> (u [R N, 1], u64, z [R N, 1], z64, norm [R N]): the float64 cdf
    at the samples and at the float64 samples, the samples themselves, and max(far, 1) per row"""
    import sampler_ref64 as S
    flat = lambda t: t.double().reshape(-1, 1)
    norm = cs["far"].double().clamp_min(1.0)[:, None].expand(-1, cs["N"]).reshape(-1)
    return (flat(S.cdf_at64(z_imp, s64.bins, s64.cdf)), flat(S.cdf_at64(s64.z_imp, s64.bins, s64.cdf)), flat(z_imp), flat(s64.z_imp),
            norm)


def add_rows(pools, cs, s64, s32, sko, z_got):
    """the rows of one case into pools[family]: every sample in u-space; the determinate ones in z-space"""
    u_k, u_64, z_k, z_64, norm = sample_rows(cs, s64, z_got)
    u_r, _, z_r, _, _ = sample_rows(cs, s64, s32.z_imp)
    u_o, _, z_o, _, _ = sample_rows(cs, s64, sko.z_imp)
    keep = determinate(cs, s64).reshape(-1)
    fam = cs["family"][:, None].expand(-1, cs["N"]).reshape(-1)
    one = torch.ones_like(norm)
    for f in fam.unique().tolist():
        m = fam == f
        pools[f].add("u-space, every sample", u_k[m], u_64[m], u_r[m], one[m], None, kernel_order=u_o[m])
        if bool((m & keep).any()):
            pools[f].add("z-space, determinate samples", z_k[m], z_64[m], z_r[m], norm[m], keep[m], kernel_order=z_o[m])
