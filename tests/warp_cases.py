"""Inputs of tests/test_warp_float64_gpu.py and tests/test_warp_ref64_cpu.py, built on the CPU from a seed (fp32 tensors, as the
kernels of csrc/warp_terms.hip see them).

  * images H x W in {2 x 2, 24 x 40, 48 x 33}: smooth plus 2 % noise (kinks of the bilinear sample stay rare), the ground-truth depth
    frames with a half of variance 0.12 and a half of variance 2e-4 (patch variances well above and well below 0.01);
  * a different K per frame: focal lengths +-20 %, principal points off centre, skew non-zero on the even frames and exactly 0 on the odd;
  * poses: small rigid motions around a common view; w2c in three kinds -- "inv64" (float64 inverse rounded to fp32), "inv_ex32"
    (torch.linalg.inv_ex in fp32, as fused/warp.py forms it), "perturbed" (a NON-inverse: inv64 with a relative perturbation of 1e-3,
    for the independent-leaf check);
  * pixels on KNOWN rows of source 0 (``case["known"]``: name -> row), as far as n and the image size allow: the corners, a depth
    behind the camera, (near_plane) a depth that puts the point within 1e-6 of the last frame's camera plane -- that frame stands
    0.6 behind the others, so that no OTHER point comes near its plane --, pixels found by search whose projection lands in each of
    the four zero-padded border strips of a target, pixels whose patch leaves the image on each side, and (patch > 1) rows whose
    ground-truth depth patch is rescaled to a variance of 0.01 (1 + eps);
  * cotangent scales per (source, pixel) row 2^U(-30, 30), in the first half neighbours alternate 2^30 / 2^-30, every 17th row zero."""
import torch

import warp_ref64 as R

F32, F64 = torch.float32, torch.float64
SIZES = ((2, 2), (24, 40), (48, 33))
VAR_EPS = (0.0, 1e-5, -1e-5, 1e-3, -1e-3, 1e-7)          # rows placed at variance 0.01 (1 + eps); +-1e-3 lies outside the fp32 bound

SHIPPED_36 = [(a, b) for a in range(8) for b in range(8) if a != b and abs(a - b) <= 3]          # keyframes at most 3 apart, both ways
# a self edge (0,0); sources 3, 6, 7 without an outgoing edge; targets 4, 6, 7 without an incoming one; target 3 with three
SPECIAL_8 = [(0, 0), (0, 3), (1, 3), (2, 3), (4, 1), (2, 5), (5, 2)]
# ne > b at b = 3: a self edge, source 2 without an outgoing edge, target 1 without an incoming one, target 2 with three (one edge twice)
SPECIAL_3 = [(0, 0), (0, 2), (1, 2), (0, 2), (1, 0)]


def quat_to_rot(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                        torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                        torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def cameras(b, H, W, g, w2c_kind, near_plane):
    K = torch.eye(4, dtype=F64).repeat(b, 1, 1)
    f0 = 0.9 * W
    K[:, 0, 0] = f0 * (1 + 0.2 * (2 * torch.rand(b, generator=g, dtype=F64) - 1))
    K[:, 1, 1] = f0 * (1 + 0.2 * (2 * torch.rand(b, generator=g, dtype=F64) - 1))
    K[:, 0, 2] = (W - 1) / 2 + 0.1 * W * (2 * torch.rand(b, generator=g, dtype=F64) - 1)
    K[:, 1, 2] = (H - 1) / 2 + 0.1 * H * (2 * torch.rand(b, generator=g, dtype=F64) - 1)
    sk = (0.5 + 1.5 * torch.rand(b, generator=g, dtype=F64)) * torch.where(torch.rand(b, generator=g) < 0.5, -1.0, 1.0).double()
    K[:, 0, 1] = torch.where(torch.arange(b) % 2 == 0, sk, torch.zeros_like(sk))
    q = torch.tensor([1.0, 0, 0, 0], dtype=F64) + 0.02 * torch.randn(b, 4, generator=g, dtype=F64)
    t = torch.tensor([0.1, 0.0, -0.2], dtype=F64) + 0.02 * torch.randn(b, 3, generator=g, dtype=F64)
    if near_plane:
        t[b - 1, 2] -= 0.6
    pose = torch.eye(4, dtype=F64).repeat(b, 1, 1)
    pose[:, :3, :3], pose[:, :3, 3] = quat_to_rot(q), t
    pose = pose.to(F32)
    inv64 = torch.linalg.inv(pose.double())
    if w2c_kind == "inv64":
        w2c = inv64.to(F32)
    elif w2c_kind == "inv_ex32":
        w2c = torch.linalg.inv_ex(pose).inverse
    else:
        assert w2c_kind == "perturbed"
        w2c = inv64.clone()
        w2c[:, :3] *= 1 + 1e-3 * (2 * torch.rand(b, 3, 4, generator=g, dtype=F64) - 1)
        w2c = w2c.to(F32)
    return K.to(F32), pose, w2c.contiguous()


def frames(count, H, W, g):
    i = torch.arange(H * W)
    uu, vv = (i % W).float(), (i // W).float()
    ph = torch.rand(count, 1, 3, generator=g) * 6.28
    rgb = 0.5 + 0.35 * torch.sin(uu[None, :, None] * (8.2 / W) + ph) * torch.cos(vv[None, :, None] * (5.7 / H) + 0.5 * ph)
    rgb = rgb + 0.02 * torch.rand(count, H * W, 3, generator=g)
    dep = 1.0 + 0.05 * torch.rand(count, H * W, 1, generator=g)
    left = (uu < W // 2)[None, :, None]
    dep = dep + torch.where(left, 1.2 * torch.rand(count, H * W, 1, generator=g), torch.zeros(1))
    return rgb.contiguous(), dep.contiguous()


def scales(b, n, g):
    e = torch.randint(-30, 31, (b * n,), generator=g).double()
    h = torch.arange(b * n // 2)
    e[h] = torch.where(h % 2 == 0, 30.0, -30.0).double()
    c = torch.exp2(e)
    c[torch.arange(b * n) % 17 == 5] = 0.0
    return c.reshape(b, n)


def _strip_search(c, s, taken, half):
    """pixels of source s (integer, not yet used) and depths whose float64 projection into some other frame lands in the middle of a
    zero-padded border strip: ix in (-1, 0), (W-1, W) or iy in (-1, 0), (H-1, H), the other coordinate well inside -> {name: (u, v, depth)} for the strips
    that some pixel reaches (tests/test_warp_ref64_cpu.py asserts that the cases together reach all four)"""
    H, W, b = c["H"], c["W"], c["b"]
    others = torch.tensor([t for t in range(b) if t != s])
    i = torch.arange(H * W)
    depths = torch.linspace(0.5, 2.5, 41, dtype=F64)
    u = (i % W).double().repeat_interleave(len(depths))[None]
    v = (i // W).double().repeat_interleave(len(depths))[None]
    d = depths.repeat(H * W)[None]
    g = R.geometry(u.expand(b, -1), v.expand(b, -1), c["pose"].double(), c["w2c"].double(), c["K"].double(), d.expand(b, -1),
                   targets=others, sources=torch.full_like(others, s))
    ix, iy = (g.tu / W * 2 - 1 + 1) / 2 * (W - 1), (g.tv / H * 2 - 1 + 1) / 2 * (H - 1)
    mid = lambda a: ((a - a.floor()) - 0.5).abs() < 0.3
    in_x, in_y = (ix > 1.2) & (ix < W - 2.2), (iy > 1.2) & (iy < H - 2.2)
    want = {"strip_left": (ix > -1) & (ix < 0) & mid(ix) & in_y, "strip_right": (ix > W - 1) & (ix < W) & mid(ix) & in_y,
            "strip_top": (iy > -1) & (iy < 0) & mid(iy) & in_x, "strip_bottom": (iy > H - 1) & (iy < H) & mid(iy) & in_x}
    found = {}
    for name, hit in want.items():
        hit = hit & (g.tz > 0.2)
        for k in hit.any(0).nonzero()[:, 0].tolist():
            px = (int(u[0, k]), int(v[0, k]))
            interior = half + 1 <= px[0] < W - half and half + 1 <= px[1] < H - half       # (off the self-projection kinks, see warp_case)
            if interior and px not in taken:
                taken.add(px)
                found[name] = (px[0], px[1], float(d[0, k]))
                break
    return found


def warp_case(b, n, H, W, patch, seed, w2c_kind="inv64", index="none", frac_uv=False, near_plane=False, corners=True):
    """-> dict: b, n, H, W, patch; uv [b,n,2], pose, w2c, K [b,4,4], depth [b,n], images [frames,H*W,3], depths [frames,H*W,1],
    frame_index (int32 [b] or None), scale [b,n] float64, known {name: row of source 0}, var_rows {row: eps}"""
    assert (H, W) in SIZES and index in ("none", "perm", "shared")
    g = torch.Generator().manual_seed(seed)
    near_plane = near_plane and b >= 2
    K, pose, w2c = cameras(b, H, W, g, w2c_kind, near_plane)
    count = b if index == "none" else b + 2
    images, depths = frames(count, H, W, g)
    frame_index = None
    if index != "none":
        frame_index = torch.randperm(count, generator=g)[:b].to(torch.int32)
        if index == "shared" and b >= 2:
            frame_index[b - 1] = frame_index[0]                       # one frame used by two batch entries
    # random pixels whose patch stays clear of the columns u = 0, W and the rows v = 0, H: a frame's own pixel re-projects onto
    # ix = u (W - 1) / W, an INTEGER there, i.e. exactly onto a kink of the bilinear sample, and its row leaves the g_depth gate
    # (the known rows on the border do, and are counted); the 2 x 2 image has no such pixel and gets fractional coordinates instead
    half = patch // 2
    frac_uv = frac_uv or H < 8
    if H >= 8:
        uv = torch.stack([torch.randint(half + 1, W - half, (b, n), generator=g).float(),
                          torch.randint(half + 1, H - half, (b, n), generator=g).float()], -1)
    else:
        uv = torch.stack([torch.randint(W, (b, n), generator=g).float(), torch.randint(H, (b, n), generator=g).float()], -1)
    depth = (0.5 + 2.0 * torch.rand(b, n, generator=g)).float()
    if near_plane:
        depth[b - 1] += 1.0                                            # (the frame that stands behind: its points stay in front of the others)
    c = dict(b=b, n=n, H=H, W=W, patch=patch, pose=pose, w2c=w2c, K=K, images=images, depths=depths, frame_index=frame_index,
             w2c_kind=w2c_kind, seed=seed)
    rows = [("corner_00", (0, 0, None)), ("corner_WH", (W - 1, H - 1, None))] if corners and n >= 16 else []
    taken = {(0, 0), (W - 1, H - 1)}
    centres = []
    if patch > 1 and H >= 2 * patch + 2:                               # a lattice of disjoint patches, for the rows placed at variance 0.01
        centres = [(cu, cv) for cv in range(half + 1, H - half, patch + 1) for cu in range(half + 1, W - half, patch + 1)]
        taken |= set(centres)
    if H < 8:
        rows = []                                                      # (2 x 2: every pixel is a corner; all rows fractional)
    else:
        if patch == 1:                                                 # (coordinates of size 1e2 .. 1e3: they would set delta for a whole patch case)
            rows.append(("behind", (W // 2 - 3, H // 2 + 2, -0.3)))
        if near_plane:
            rows.append(("near_plane", (W // 2 + 9, H // 2 - 5, "plane")))
        if b >= 2 and n >= 16:
            rows += list(_strip_search(c, 0, taken, half).items())
        if n >= 128:                                                   # (on the border: out of the g_depth gate, see above; 4 of >= 255 rows)
            rows += [("leaves_left", (0, H // 2, None)), ("leaves_right", (W - 1, H // 2 - 1, None)), ("leaves_top", (W // 2, 0, None)),
                     ("leaves_bottom", (W // 2 + 1, H - 1, None))]
    known, var_rows = {}, {}
    for r, (name, (pu, pv, pd)) in enumerate(rows[:n]):
        known[name] = r
        uv[0, r] = torch.tensor([float(pu), float(pv)])
        if pd == "plane":                                              # q.z of the last frame is linear in the depth: solve q.z = 0
            best = None
            for du, dv in ((9, -5), (-9, 5), (9, 5), (-9, -5), (12, -7), (-12, 7)):     # the pixel with the largest |pr.x|, |pr.y| there
                pu_, pv_ = torch.full((2, 1), float(W // 2 + du), dtype=F64), torch.full((2, 1), float(H // 2 + dv), dtype=F64)
                two = torch.tensor([0, b - 1])
                one = lambda z: R.geometry(pu_, pv_, pose[two].double(), w2c[two].double(), K[two].double(), torch.full((2, 1), z, dtype=F64),
                                           targets=torch.tensor([1]), sources=torch.tensor([0]))
                z0, z1 = one(0.0).q[0, 0, 2], one(1.0).q[0, 0, 2]
                at = float(-z0 / (z1 - z0))
                g_ = one(at)
                size = float(torch.minimum((g_.tu * g_.tz).abs(), (g_.tv * g_.tz).abs()))     # min(|pr.x|, |pr.y|) up to 1e-8 / tz
                if (W // 2 + du, H // 2 + dv) not in taken and (best is None or size > best[0]):
                    best = (size, W // 2 + du, H // 2 + dv, at)
            uv[0, r] = torch.tensor([float(best[1]), float(best[2])])
            depth[0, r] = best[3]
        elif pd is not None:
            depth[0, r] = pd
    if frac_uv:                                                        # the .long() truncation on fractional coordinates
        free = torch.arange(n) >= len(rows)
        uv[:, free] += torch.tensor([0.25, 0.75])
        uv[b - 1, free] += torch.tensor([0.5, -0.5])                  # (+0.75, +0.25 on the last source)
    if centres:
        # rows whose ground-truth depth patch has the variance 0.01 (1 + eps): centres on the lattice, in source 0's frame
        f0 = 0 if frame_index is None else int(frame_index[0])
        dimg = depths[f0].reshape(H, W).double()
        r = len(rows)
        # (patch 11 on 24 x 40: four of the six disjoint patches, so that the half of low variance keeps patches well below 0.01)
        for eps, (cu, cv) in zip(VAR_EPS[:4] if patch == 11 else VAR_EPS, centres):
            if r >= n:
                break
            z = torch.randn(patch, patch, generator=g, dtype=F64)
            z = z - z.mean()
            s = (R.FLAT_LIMIT * (1 + eps) / (z * z).mean()).sqrt()
            dimg[cv - half:cv + half + 1, cu - half:cu + half + 1] = 1.0 + s * z
            uv[0, r] = torch.tensor([float(cu), float(cv)])
            var_rows[r] = eps
            r += 1
        depths[f0] = dimg.reshape(H * W, 1).float()
    c.update(uv=uv.contiguous(), depth=depth.contiguous(), scale=scales(b, n, g), known=known, var_rows=var_rows)
    return c


def cot_rows(scale, shape, seed):
    """U(-1,1) times the row's scale, fp32.  scale [rows...] float64, shape = the trailing dimensions of a row"""
    g = torch.Generator().manual_seed(seed)
    base = 2 * torch.rand(tuple(scale.shape) + tuple(shape), generator=g, dtype=F64) - 1
    return (base * scale.reshape(tuple(scale.shape) + (1,) * len(shape))).float()


def g_sampled_of(c, scale=None):
    """[b_t, b_s, n, p2, 3]: the row (s, i) carries its scale in every target, cell and channel"""
    b, n, p2 = c["b"], c["n"], c["patch"] ** 2
    scale = c["scale"] if scale is None else scale
    return cot_rows(scale, (b, p2, 3), c["seed"] + 7).permute(2, 0, 1, 3, 4).contiguous()


def g_flow_of(c, edges, scale=None):
    """[ne, n, 2]: the row (edge e, pixel i) carries the scale of (source of e, i)"""
    scale = c["scale"] if scale is None else scale
    ii = torch.tensor([a for a, _ in edges], dtype=torch.long)
    return cot_rows(scale[ii], (2,), c["seed"] + 11)


# (b, n, (H, W), patch, w2c kind, frame index, fractional uv, near plane); per image n p2 threads = ceil(n p2 / 256) * 4 waves
PATCH_CASES = {
    # (b = 1 with the perturbed w2c: against its exact inverse a frame's own re-projection does not depend on the depth at all, and
    #  g_depth would be rounding noise on both sides)
    "b1 n1 2x2 p1": (1, 1, (2, 2), 1, "perturbed", "none", False, False),
    "b2 n1 24x40 p5": (2, 1, (24, 40), 5, "inv64", "none", False, False),
    "b2 n4 2x2 p3": (2, 4, (2, 2), 3, "inv_ex32", "shared", False, False),
    "b1 n64 24x40 p3": (1, 64, (24, 40), 3, "perturbed", "none", False, False),
    "b2 n63 24x40 p11": (2, 63, (24, 40), 11, "inv64", "shared", False, False),          # 120 waves per image; no corner rows
    "b3 n65 48x33 p5": (3, 65, (48, 33), 5, "perturbed", "perm", False, False),           # 28 waves per image: past the 21 groups
    "b8 n257 24x40 p1": (8, 257, (24, 40), 1, "inv_ex32", "none", False, True),           # 8 waves per image, 64 in all
    "b8 n255 48x33 p1": (8, 255, (48, 33), 1, "perturbed", "perm", True, False),
    "b3 n256 48x33 p3": (3, 256, (48, 33), 3, "inv64", "shared", False, False),
    "b8 n64 24x40 p3": (8, 64, (24, 40), 3, "perturbed", "perm", False, False),
    # fractional uv under a patch on a real image: the .long() truncation of the multi-cell patch read and of k_warp_flat
    "b3 n63 24x40 p3 frac": (3, 63, (24, 40), 3, "inv_ex32", "perm", True, False),
}
SEEDS = {"b3 n63 24x40 p3 frac": 1010}                 # seeds set by hand; every other case: 1000 + its rank among the rest
POOLED_PATCH = ("b1 n1 2x2 p1", "b2 n1 24x40 p5", "b2 n4 2x2 p3", "b1 n64 24x40 p3")   # n = 1, b = 1, the 2 x 2 image: judged once

# (b, n, edges, w2c kind); the flow reads no image: H, W only size the known rows
FLOW_CASES = {
    "b8 n257 shipped 36": (8, 257, SHIPPED_36, "inv_ex32"),           # 64 waves, ne > b
    "b8 n65 special 7": (8, 65, SPECIAL_8, "perturbed"),
    "b3 n255 special 5": (3, 255, SPECIAL_3, "inv64"),
    "b2 n256 one edge": (2, 256, [(1, 0)], "perturbed"),
    "b1 n64 self": (1, 64, [(0, 0)], "perturbed"),                    # (against the exact inverse a self edge is all rounding noise)
    "b1 n1 self": (1, 1, [(0, 0)], "perturbed"),
    "b2 n63 pair": (2, 63, [(0, 1), (1, 0)], "perturbed"),
    "b3 n1 special 5": (3, 1, SPECIAL_3, "inv64"),
}
POOLED_FLOW = ("b1 n64 self", "b1 n1 self", "b2 n63 pair", "b3 n1 special 5")


def patch_case(name):
    b, n, (H, W), patch, kind, index, frac, near = PATCH_CASES[name]
    # (the corners' own re-projection sits on a kink, which takes their rows out of the g_depth gate: with 242 samples a row, patch 11
    #  has no room for them under the 5 % cap; the corners of patch 3 and 5 leave the image on two sides each)
    seed = SEEDS[name] if name in SEEDS else 1000 + sorted(k for k in PATCH_CASES if k not in SEEDS).index(name)
    return warp_case(b, n, H, W, patch, seed, kind, index, frac, near, corners=patch != 11)


def flow_case(name):
    b, n, edges, kind = FLOW_CASES[name]
    c = warp_case(b, n, 24, 40, 1, 2000 + sorted(FLOW_CASES).index(name), kind)
    c["edges"] = edges
    c["idii"] = torch.tensor([a for a, _ in edges], dtype=torch.int64)
    c["idjj"] = torch.tensor([t for _, t in edges], dtype=torch.int64)
    return c


def evaluate(c, dtype):
    return R.patch_warp(c["uv"], c["pose"], c["w2c"], c["K"], c["depth"], c["images"], c["depths"], c["frame_index"], c["H"], c["W"],
                        c["patch"], dtype=dtype)


def evaluate_flow(c, dtype):
    return R.flow(c["uv"], c["pose"], c["w2c"], c["K"], c["depth"], c["idii"], c["idjj"], dtype=dtype)


def _near_integer(a, delta):
    return (a - a.round()).abs() < delta


def exclusions(c, o64, o32):
    """What the kernel gates leave out of a patch-warp case, from the restatement ALONE (its float64 and fp32 evaluations):
    delta = 8 x the largest |fp32 - float64|, one for each of ix, iy, gx, gy and tz, over the samples whose coordinates are usable
    (b.ok) in both; the factor 8 is the margin for the kernel's different operation order.
      * g_depth row (s, i): one of its usable samples has a float64 ix or iy within delta of an integer (the bilinear slope jumps there);
      * mask entry: gx or gy lies within delta of +-1 or tz within delta of 0, and NO other factor of the entry is false by more
        than delta -- an entry with one factor robustly false is false on both sides whatever the close comparison says;
      * flat row: float64 variance within R.flat_bound of 0.01.  Such a row takes NO mask entry out: its entries are held to the
        flat bit that the side under test produced itself (expected_mask).
    -> dict(delta {ix, iy, gx, gy, tz}, rows [b,n] bool, mask [b,b,n,p2] bool, flat [b,n] bool or None)"""
    both = o64.ok & o32.ok
    worst = lambda a, b_: float((a.double() - b_)[both].abs().max()) if bool(both.any()) else 0.0
    d_ix, d_iy, d_gx, d_gy, d_tz = (8 * worst(getattr(o32, k), getattr(o64, k)) for k in ("ix", "iy", "gx", "gy", "tz"))
    # (a kink between two cells that both read nothing but zero padding is none: the integer k = round(ix) separates the cells k - 1
    #  and k, which read the columns k - 1 .. k + 1 and the rows y0, y0 + 1)
    H, W = c["H"], c["W"]
    kx, ky = o64.ix.round(), o64.iy.round()
    reach_x = (kx >= -1) & (kx <= W) & (o64.y0 >= -1) & (o64.y0 <= H - 1)
    reach_y = (ky >= -1) & (ky <= H) & (o64.x0 >= -1) & (o64.x0 <= W - 1)
    kink = o64.ok & ((_near_integer(o64.ix, d_ix) & reach_x) | (_near_integer(o64.iy, d_iy) & reach_y))
    rows = kink.any(dim=3).any(dim=0)
    # per comparison: close (within delta of the limit) / robustly false
    close, false = torch.zeros_like(o64.ok), torch.zeros_like(o64.ok)
    for val, lim, sign, d in ((o64.gx, -1.0, 1, d_gx), (o64.gx, 1.0, -1, d_gx), (o64.gy, -1.0, 1, d_gy), (o64.gy, 1.0, -1, d_gy),
                              (o64.tz, 0.0, 1, d_tz)):
        margin = sign * (val - lim)                        # the comparison holds where margin > 0
        near = ~(margin.abs() > d)                         # (a NaN counts as close)
        close, false = close | near, false | (~near & (margin < 0))
    false = false | ~o64.inside[None]
    flat = None
    if o64.flat is not None:
        flat = (o64.var - R.FLAT_LIMIT).abs() <= R.flat_bound(o64.var, float(c["depths"].abs().max()), c["patch"] ** 2)
        false = false | (~flat & ~o64.flat)[None, :, :, None]
    return dict(delta=dict(ix=d_ix, iy=d_iy, gx=d_gx, gy=d_gy, tz=d_tz), rows=rows, mask=close & ~false, flat=flat)


def expected_mask(o64, ex, flat_seen):
    """The mask a side under test must produce bit for bit outside ex["mask"]: the float64 comparisons on gx, gy and tz, the
    ``inside`` test, and the flat bit of the row -- the float64 one, except on the rows of ex["flat"] (variance within the fp32
    rounding bound of 0.01), where it is the bit ``flat_seen`` [b,n] that the same side returned for the row."""
    m = (o64.gx > -1) & (o64.gx < 1) & (o64.gy > -1) & (o64.gy < 1) & (o64.tz > 0) & o64.inside[None]
    if o64.flat is not None:
        m = m & torch.where(ex["flat"], flat_seen.bool(), o64.flat)[None, :, :, None]
    return m


def known_rows(c, with_var=False):
    """[b,n] bool: the rows of the known-edge pixels (all of them in source 0); with_var: the rows placed near variance 0.01 as well"""
    k = torch.zeros(c["b"], c["n"], dtype=torch.bool)
    k[0, list(c["known"].values())] = True
    if with_var and c["var_rows"]:                 # (and every row that reads the same patch of the same frame)
        frame = lambda s: s if c["frame_index"] is None else int(c["frame_index"][s])
        for r in c["var_rows"]:
            for s in range(c["b"]):
                if frame(s) == frame(0):
                    k[s] |= (c["uv"][s] == c["uv"][0, r]).all(-1)
    return k


def check_caps(c, ex):
    """the caps on what is left out, conditions of the tests -> a line for the log"""
    b, n = c["b"], c["n"]
    rows, entries = int(ex["rows"].sum()), int(ex["mask"].sum())
    d = ex["delta"]
    line = (f"delta ix {d['ix']:.2e} iy {d['iy']:.2e} gx {d['gx']:.2e} gy {d['gy']:.2e} tz {d['tz']:.2e}; left out: g_depth rows {rows} of {b * n}, "
            f"mask entries {entries} of {ex['mask'].numel()}")
    assert rows <= 0.05 * b * n, f"{line}: more than 5 % of the g_depth rows"
    assert entries <= 0.01 * ex["mask"].numel(), f"{line}: more than 1 % of the mask entries"
    placed = known_rows(c, with_var=True) & ~known_rows(c)
    # No known-edge row is left out, with one kind of entry held to "either value": against the exact inverse a frame's own pixel
    # on column 0 or row 0 re-projects onto gx = -1 or gy = -1 up to rounding, and that comparison is a coin toss in the reference
    # itself (tests/test_warp_cpu.py: "a projection within an ulp of the image border may flip").  Only the entry t = s of such a
    # row may be left out, only by its gx / gy comparison against -1, and never under the perturbed w2c, which moves the
    # re-projection off the border; every other entry of a known-edge row is asserted (here that none is left out, in the tests
    # that each equals the reference).
    own = torch.eye(b, dtype=torch.bool)[:, :, None, None]
    known = known_rows(c)
    assert not bool((ex["mask"] & ~own).any(dim=3).any(dim=0)[known].any()), f"{line}: a known-edge row is left out of the mask"
    own_out = (ex["mask"] & own).any(dim=0)[known]                                    # [known rows, p2]
    on_border = ((c["uv"][known][:, None, 0] + R.cell_offsets(c["patch"])[None, :, 0] == 0)
                 | (c["uv"][known][:, None, 1] + R.cell_offsets(c["patch"])[None, :, 1] == 0))
    assert bool((own_out <= on_border).all()), f"{line}: a known-edge row is left out of the mask off column 0 and row 0"
    assert c["w2c_kind"] != "perturbed" or not bool(own_out.any()), f"{line}: a known-edge row is left out of the mask"
    line += f" ({int(own_out.any(dim=1).sum())} known rows with their own frame's entry on gx, gy = -1 held to either value)"
    if ex["flat"] is not None:
        other = int((ex["flat"] & ~placed).sum())
        line += f", flat rows {int(ex['flat'].sum())} of {b * n} ({int((ex['flat'] & placed).sum())} of them placed there)"
        assert other <= 0.01 * b * n, f"{line}: more than 1 % of the flat rows"
        assert not bool(ex["flat"][known].any()), f"{line}: a known-edge row is left out of flat"
    return line


def known_mask_entries(c, ex):
    """[b_t, b_s, n, p2] bool: the mask entries of the known-edge rows that the tests assert explicitly -- all of them but those that
    check_caps holds to either value"""
    return known_rows(c)[None, :, :, None] & ~ex["mask"]


def pose_norms(scale, feeds):
    """[b] the largest cotangent scale among the rows that feed image s as a source / image t as a target (feeds [b_t, b_s] bool)"""
    per_source = scale.amax(dim=1)
    as_target = torch.stack([per_source[feeds[t]].max() if bool(feeds[t].any()) else torch.zeros((), dtype=F64) for t in range(scale.shape[0])])
    return per_source, as_target


L1_ITEMS = (0, 1, 255, 256, 257, 65536, 65537, 3 * 65536 + 5)
L1_CH = (1, 2, 3)
L1_MASKS = ("none", "all", "empty", "random")


def l1_case(items, ch, mask, seed):
    """pred, target [items, ch] fp32 with every 17th entry an exact tie, mask [items] bool or None"""
    g = torch.Generator().manual_seed(seed)
    pred, target = torch.rand(items, ch, generator=g), torch.rand(items, ch, generator=g)
    target.view(-1)[::17] = pred.view(-1)[::17]
    m = {"none": None, "all": torch.ones(items, dtype=torch.bool), "empty": torch.zeros(items, dtype=torch.bool),
         "random": torch.rand(items, generator=g) > 0.4}[mask]
    return pred, target, m
