"""The inputs of tests/test_objective_float64_gpu.py (test infrastructure), built on the CPU from seeds so that
tests/test_objective_ref64_cpu.py can check on the very same tensors what the GPU gate relies on: the 0/1 last alpha, the size of the
yardstick's own error, the left-out shares."""
import math

import torch

RES = 64
COMPOSITE_S = (1, 2, 63, 64, 65, 98, 128, 129, 160, 192, 193, 255, 256)      # lane ownership changes at 64/65, 128/129, 192/193
COMPOSITE_R_SMALL = (1, 3, 5)
COMPOSITE_R_BIG = 1027
COMPOSITE_S_BIG = (98, 128, 160, 256)
EDGES = ("zero_sdf", "equal_z", "zero_grad", "beyond", "exact099", "decade1", "decade10", "decade100")
GROUPS = ("crossing", "crossing, visited voxels", "grazing", "miss")
KINK = 2e-6                                    # as tests/test_gemm_float64_gpu.py
SUM_W_MIN = 1e-3                               # depth = sum w z / (sum w + 1e-8) is ill-conditioned below


def composite_shapes():
    return [(R, S) for S in COMPOSITE_S for R in COMPOSITE_R_SMALL] + [(COMPOSITE_R_BIG, S) for S in COMPOSITE_S_BIG]


def scales(n, g, lo=-30, hi=30):
    """c_r = 2^U(lo, hi); within the first half neighbours alternate 2^hi / 2^lo; every 97th ray 0"""
    e = torch.randint(lo, hi + 1, (n,), generator=g).double()
    h = torch.arange(n // 2)
    e[h] = torch.where(h % 2 == 0, float(hi), float(lo)).double()
    c = torch.exp2(e)
    c[torch.arange(n) % 97 == 5] = 0.0
    return c


def scaled(base, c):
    return (base.double() * c.reshape((-1,) + (1,) * (base.dim() - 1))).float()


def voxel_table(g):
    """visit counts 0 .. 30 000 on some 70 % of the voxels of the half space x < 0 (where the rays of group 2 live); two known voxels
    at the ends of the index range for the rays that sit exactly on +-0.99"""
    v = torch.zeros(RES, RES, RES)
    half = torch.rand(RES // 2, RES, RES, generator=g) * 30000.0 * (torch.rand(RES // 2, RES, RES, generator=g) < 0.7)
    v[: RES // 2] = half.floor()
    v[RES - 1, 0, :] = 12345.0
    return v


def _edge_rays(R, S):
    """{ray: edge}: R >= 32: rays 8.. and 500.. carry one edge each; smaller R: ray r carries edge (r + S) mod 8"""
    if R >= 32:
        out = {8 + k: e for k, e in enumerate(EDGES)}
        if R >= 540:
            out.update({500 + 3 * k: e for k, e in enumerate(EDGES)})
        return out
    return {r: EDGES[(r + S) % len(EDGES)] for r in range(R)}


def composite_case(R, S, seed):
    """-> dict of fp32 CPU tensors: rays_o, rays_d [R,3], z [R,S] ascending, sdf [R,S], rgb, grad [R,S,3], voxels, group [R] (0..3),
    edges {ray: name}"""
    import objective_ref64 as O
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    group = torch.arange(R) % 4                                    # interleaved ray by ray
    o = (rnd(R, 3) - 0.5) * 0.4
    d = torch.nn.functional.normalize(rnd(R, 3) - 0.5, dim=-1) * 0.35
    side = torch.where(group == 1, -1.0, 1.0)
    o[:, 0] = side * (0.5 + o[:, 0] * 0.5)                         # x_0 = +-(0.4 .. 0.6) + z d_0, |z d_0| <= 0.14
    d[:, 0] *= 0.2
    z = torch.sort(rnd(R, S) * 1.95 + 0.05, dim=-1)[0]
    slope = 0.3 + 0.7 * rnd(R, 1)
    zc_cross = z[:, :1] * 0.5 if S == 1 else z[:, :1] + (0.1 + 0.8 * rnd(R, 1)) * (z[:, -1:] - z[:, :1])
    k = torch.randint(0, max(S // 2, 1), (R, 1), generator=g)
    zc_graze = torch.gather(z, 1, k)
    sdf = torch.where((group <= 1)[:, None], slope * (zc_cross - z),
                      torch.where((group == 2)[:, None], 0.002 * rnd(R, 1) + slope * (z - zc_graze).abs(), 0.3 + rnd(R, S)))
    rgb = rnd(R, S, 3)
    grad = torch.randn(R, S, 3, generator=g) * torch.exp2(torch.rand(R, S, 1, generator=g) * 6 - 3)
    voxels = voxel_table(g)
    edges = _edge_rays(R, S)
    for r, e in edges.items():
        m = S // 2
        if e == "zero_sdf":
            sdf[r, m] = 0.0
        elif e == "equal_z" and S >= 2:
            z[r, S // 3 + 1] = z[r, S // 3]                        # an interval of length 0
        elif e == "zero_grad":
            grad[r, m] = 0.0
        elif e == "beyond":                                        # leaves |x| <= 0.99 along the ray (x_0 = 0.9 + 0.1 z)
            o[r] = torch.tensor([0.9, 0.2, 0.1])
            d[r] = torch.tensor([0.1, 0.02, -0.03])
        elif e == "exact099":                                      # x_0 = fp32(0.99), x_1 = -fp32(0.99) at every sample: inside, voxel
            o[r] = torch.tensor([0.99, -0.99, 0.3])                # indices RES - 1 and 0 (the ends of the range)
            d[r] = torch.tensor([0.0, 0.0, 0.1])
    zero_grad = [r for r, e in edges.items() if e == "zero_grad"]
    if R >= 32:                                                    # (enough zero rows for a statistic: every 16th ray, a grazing one,
        more = [r for r in range(10, R, 16) if r not in edges]    # at the sample that meets the surface)
        grad[more, k[more, 0]] = 0.0
        zero_grad += more
    for r, e in edges.items():                                     # the last sample at sdf / beta = 1, 10, 100
        if e.startswith("decade"):                                 # (on a grazing profile that meets the surface at sample 0, so that
            if S >= 2:                                             # the ray keeps some weight whatever the last sample does)
                sdf[r] = 0.001 + slope[r] * (z[r] - z[r, 0]).abs()
                group[r] = 2
            elif e == "decade100":                                 # S = 1: the only sample is in empty space -- a miss
                group[r] = 3
            count = O.visit_counts(O.sample_points(z[r:r + 1, -1:], o[r:r + 1], d[r:r + 1]), voxels, RES)
            sdf[r, -1] = float(e[6:]) * float(O.beta_of(count, torch.float64))
    c = lambda t: t.float().contiguous()
    return dict(rays_o=c(o), rays_d=c(d), z=c(z), sdf=c(sdf), rgb=c(rgb), grad=c(grad), voxels=c(voxels), group=group, edges=edges,
                zero_grad_rays=zero_grad, R=R, S=S)


COTANGENTS = ("g_rgb_values", "g_depth", "g_nmap", "g_entropy", "g_weights")


def composite_cotangents(case, seed):
    """-> c_r [R] float64 and the five unit cotangents times c_r (fp32)"""
    R, S = case["R"], case["S"]
    g = torch.Generator().manual_seed(seed)
    c = scales(R, g)
    shapes = dict(g_rgb_values=(R, 3), g_depth=(R,), g_nmap=(R, 3), g_entropy=(R,), g_weights=(R, S))
    return c, {k: scaled(torch.randn(shapes[k], generator=g), c) for k in COTANGENTS}


def composite_args(case):
    return (case["z"], case["sdf"], case["rgb"], case["grad"], case["rays_o"], case["rays_d"], case["voxels"], RES)


def track_gt(case, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(case["R"], 3, generator=g)


# ------------------------------------------------------------------------------------------------------------------ rays and pose
RAYS_B = (1, 3, 8)
RAYS_N = (1, 63, 1024, 1025, 8192 + 7)          # the 1024-thread stride of k_rays_pose_bwd crossed and ragged
IMG_W, IMG_H = 1200, 680


def rays_case(b, n, seed):
    """-> uv [b,n,2], cam [b,7], K [b,4,4], c_r [b*n] float64, g_o, g_d [b*n,3]; image 1 (b >= 3) has all-zero cotangents"""
    g = torch.Generator().manual_seed(seed)
    cam = torch.zeros(b, 7)
    K = torch.zeros(b, 4, 4)
    uv = torch.stack([torch.rand(b, n, generator=g) * (IMG_W - 1), torch.rand(b, n, generator=g) * (IMG_H - 1)], -1)
    for i in range(b):
        j = i + seed
        q = torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0)
        if j % 4 == 1:                                              # within 1e-3 of a half turn
            axis = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0)
            th = math.pi - 1e-3 * float(torch.rand((), generator=g))
            q = torch.cat([torch.tensor([math.cos(th / 2)]), math.sin(th / 2) * axis])
        cam[i, :4] = q * (2.0 ** (-10, 0, 10)[j % 3])
        cam[i, 4:] = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=0) * (0.0, 1.0, 100.0)[(j + j // 3) % 3]
        fx, fy = 600.0 + 7 * i, 590.0 - 5 * i
        K[i] = torch.eye(4)
        K[i, 0, 0], K[i, 1, 1], K[i, 0, 1], K[i, 0, 2], K[i, 1, 2] = fx, fy, 2.5 + 0.5 * i, 610.25 + 3 * i, 330.75 - 2 * i
        special = torch.tensor([[0.0, 0.0], [IMG_W - 1.0, 0.0], [0.0, IMG_H - 1.0], [IMG_W - 1.0, IMG_H - 1.0],
                                [float(K[i, 0, 2]), float(K[i, 1, 2])]])
        m = min(n, 5)
        uv[i, :m] = special.roll(-i, 0)[:m]                        # the four corners and the principal point
    c = scales(b * n, g)
    if b >= 3:
        c[n:2 * n] = 0.0
    g_o, g_d = (scaled(torch.randn(b * n, 3, generator=g), c) for _ in range(2))
    return dict(uv=uv.contiguous(), cam=cam.contiguous(), K=K.contiguous(), c=c, g_o=g_o, g_d=g_d, b=b, n=n)


def rays_backward_case(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    c = scales(R, g)
    z = torch.sort(torch.rand(R, S, generator=g) * 3.5, dim=-1)[0]
    g_x, g_dir = (scaled(torch.randn(R, S, 3, generator=g), c) for _ in range(2))
    return dict(z=z.contiguous(), g_x=g_x, g_dir=g_dir, c=c)


L1_N = (3, 255, 3 * 1024, 3 * 8192 + 3)


def l1_case(n, seed):
    """pred, target [n] in [0,1); every 7th element an exact tie (gradient exactly 0)"""
    g = torch.Generator().manual_seed(seed)
    pred, target = torch.rand(n, generator=g), torch.rand(n, generator=g)
    target[::7] = pred[::7]
    return pred, target


# ------------------------------------------------------------------------------------------------------------------ loss
LOSS_SHAPES = ((1, 1, 3, 0), (1, 255, 40, 7), (3, 257, 40, 4400), (8, 1024, 98, 22 * 8192), (2, 5000, 16, 100))
LOSS_WEIGHTS = dict(rgb=1.0, eikonal=0.1, smooth=0.005, depth=0.1, gt_depth=0.0, normal_l1=0.05, normal_cos=0.05)
LOSS_VARIANTS = ("plain", "whole_image", "first_frame", "no_foreground", "no_smooth_no_eikonal", "null_nei", "one_empty_image",
                 "near_singular", "edge_foreground", "zero_rows", "one_gt_depth")


def loss_case(shape, variant, seed):
    """-> out, gt (fp32 CPU tensors, the arguments of objective_ref64.slam_terms), weights (7), whole_image, note
    (tests/test_loss_gpu.py::_random_case plus the edges of the variant)"""
    bs, n, S, E = shape
    g = torch.Generator().manual_seed(seed)
    R = bs * n
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    sdf = rn(R, S).abs() + 0.01
    cross = ru(R) < (0.0 if variant == "no_foreground" else 0.7)          # rays whose sdf changes sign
    sdf[cross, S // 2:] *= -1
    mask = (ru(bs, n, 1) > 0.1).float()
    depth = ru(bs, n, 1) * 3 + 0.5
    out = dict(rgb_values=ru(bs, n, 3), depth_values=depth, normal_map=rn(bs, n, 3), grad_theta=rn(E, 3) if E else None,
               grad_theta_nei=rn(E, 3) if E else None, sdf=sdf)
    gt_depth = ru(bs, n, 1) * 3 * (ru(bs, n, 1) > 0.2)
    gt = dict(rgb=ru(bs, n, 3), depth=ru(bs, n, 1) * 0.05, normal=rn(bs, n, 3), gt_depth=gt_depth, gt_depth_mask=gt_depth.clone(),
              mask=mask)
    w = dict(LOSS_WEIGHTS)
    whole = variant == "whole_image"
    sd = sdf.view(bs, n, S)
    if variant == "first_frame":                                           # loss.py: supervise with the scaled monocular depth
        gt["gt_depth"] = gt["depth"] * 20.0
        w["gt_depth"] = 10.0
    elif variant == "no_smooth_no_eikonal":
        w["eikonal"] = w["smooth"] = 0.0
    elif variant == "null_nei":
        out["grad_theta_nei"] = None
    elif variant == "one_empty_image":                                     # one image of the batch without foreground
        sd[bs // 2] = sd[bs // 2].abs()
    elif variant == "near_singular":                                       # masked depths of image 0 constant to 1e-6 relative
        depth[0] = 1.7 * (1.0 + 1e-6 * (2 * ru(n, 1) - 1))
    elif variant == "edge_foreground":                                     # a foreground ray first / last in its image, background next
        for b_ in range(bs):
            for i, fg in ((0, True), (1, False), (n - 1, True), (n - 2, False)):
                if 0 <= i < n and (fg or n > 2):
                    sd[b_, i] = sd[b_, i].abs()
                    if fg:
                        sd[b_, i, S // 2:] *= -1
                        mask[b_, i] = 1.0
    elif variant == "zero_rows":                                           # a grad_theta row and a masked normal_map row of zeros
        if E:
            out["grad_theta"][E // 2:E // 2 + (48 if E >= 96 else 1):3] = 0.0
        for i in range(n // 2, min(n // 2 + 48, n), 3):                   # (16 rays, foreground, every third)
            sd[0, i] = sd[0, i].abs()
            sd[0, i, S // 2:] *= -1
            mask[0, i] = 1.0
            out["normal_map"][0, i] = 0.0
    elif variant == "one_gt_depth":                                        # a depth_real_mask with one set element
        w["gt_depth"] = 0.5
        gt["gt_depth_mask"] = torch.zeros(bs, n, 1)
        gt["gt_depth_mask"][bs - 1, n // 3] = 1.0
    weights = tuple(w[k] for k in ("rgb", "eikonal", "smooth", "depth", "gt_depth", "normal_l1", "normal_cos"))
    return out, gt, weights, whole


def loss_cases():
    """(shape, variant): every variant at (3, 257, 40, 4400), the plain objective at every shape, the edges again at the smallest and
    at the mapping shape"""
    cases = [(s, "plain") for s in LOSS_SHAPES] + [(LOSS_SHAPES[2], v) for v in LOSS_VARIANTS[1:]]
    cases += [(LOSS_SHAPES[1], v) for v in ("null_nei", "edge_foreground", "zero_rows", "one_gt_depth", "near_singular")]
    cases += [(LOSS_SHAPES[0], v) for v in ("edge_foreground", "one_gt_depth")]
    cases += [(LOSS_SHAPES[4], v) for v in ("one_empty_image", "near_singular", "whole_image")]
    cases += [(LOSS_SHAPES[3], v) for v in ("edge_foreground", "null_nei")]
    return cases


def loss_kinks(aux, shape):
    """bool [R] depth-kink rays, bool [R] normal-kink rays: a float64 magnitude of the quantity under a `sign` below the fp32 rounding
    bound of that quantity -- 8 * 2^-24 * (|scale p| + |shift| + |t|) for a depth residual (both rays of a pair), 8 * 2^-24 for a
    component of the difference of unit normals.  Left out on both sides of the kink."""
    bs, n = shape[0], shape[1]
    eps = 8 * 2.0 ** -24
    dk = torch.zeros(bs, n, dtype=torch.bool)
    if "resid" in aux:
        d, m, bound = aux["resid"], aux["depth_mask"], eps * aux["resid_bound"]
        pair = (m[:, 1:] * m[:, :-1]) > 0
        close = pair & ((d[:, 1:] - d[:, :-1]).abs() < bound[:, 1:] + bound[:, :-1])
        dk[:, 1:] |= close
        dk[:, :-1] |= close
    nk = torch.zeros(bs * n, dtype=torch.bool)
    if "unit_diff" in aux:
        nk = aux["fg"].reshape(-1) & (aux["unit_diff"].abs().amin(-1) < eps)
    return dk.reshape(-1), nk
