"""Self-intersections of a triangle mesh on the device, decided exactly (include/nicer_slam_amd.h Section 25,
csrc/mesh_intersect.hip): which pairs of faces meet in more than the vertices or the edge they share, as sets of real points -- the
fp32 coordinates are rationals and so is the answer; there is no tolerance anywhere.

* ``self_intersections(mesh, kinds=("proper", "touch"), between=None, brute=False, return_report=False)``: (pairs int64 [n, 2] with
  i < j sorted by (i, j), code uint8 [n], flags uint8 [F]).  A code holds the kind in its two low bits (PROPER 1: the relative
  interiors meet -- a transversal crossing, a coplanar overlap with area, a fold-over, a duplicate; TOUCH 2: reported, not proper --
  a vertex on a face, an edge lying in a face, a T-junction, two edges crossing at a point), COPLANAR 4, and s, the number of vertex
  positions the two faces share, in bits 4 and 5.  flags: bit 0 the face is in a returned proper pair, bit 1 in a returned touch
  pair.  ``between`` (bool per face) keeps only the pairs with one face on each side of the mask: a patch against the rest, or mesh
  A against mesh B after concatenation.  ``brute=True`` tests all pairs on the device (the cross-check of the tree).
* ``is_embedded(mesh)``: no proper pair.
* ``python -m nicer_slam_amd.mesh_intersect MESH.ply [--kinds proper|touch|all] [--brute] [--out FLAGGED.ply] [--pairs PAIRS.npy]
  [--json]``; the exit status is 0 whatever is found.

A float64 filter decides the generic pairs, 256-bit integers on the device the rest; a pair whose exponents span more than 59 binades
(and a face whose own span more than 102) is decided here with Python integers -- slow, and never wrong.  numpy in, numpy out; torch
in, torch out.  There is no CPU path for the search: a missing GPU is an error.
"""
import argparse
import json
import sys

import numpy as np
import torch

from ._native import check, lib
from .mesh_args import as_tensor, mesh_dict_tensors, need_gpu, stream, workspace
from .mesh_eval import TriIndex
from .ply import read_ply, write_mesh_ply

PROPER, TOUCH, UNRESOLVED, COPLANAR = 1, 2, 3, 4
BRUTE = 1
KINDS = ("proper", "touch")
CAUSES = ("index", "non_finite", "zero_area", "collinear")
STATE_UNRESOLVED = 5             # a face whose collinearity the device could not decide (exponent span above 102)


# ---- the decision in Python integers: the same sign logic as csrc/intersect_passes.hpp, on numbers of any size ----------------------

def _sgn(x):
    return (x > 0) - (x < 0)


def _ints(*faces):
    """the coordinates of fp32 faces [3, 3] as integers over one common power of two"""
    ratios = [[float(x).as_integer_ratio() for x in np.asarray(t, np.float32).reshape(-1)] for t in faces]
    den = max(d for r in ratios for _, d in r)
    return [[tuple(n * (den // d) for n, d in r[3 * k:3 * k + 3]) for k in range(3)] for r in ratios]


def _o3(a, b, c, d):
    ax, ay, az = a[0] - d[0], a[1] - d[1], a[2] - d[2]
    bx, by, bz = b[0] - d[0], b[1] - d[1], b[2] - d[2]
    cx, cy, cz = c[0] - d[0], c[1] - d[1], c[2] - d[2]
    return ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)


def _normal(t):
    u = [t[1][k] - t[0][k] for k in range(3)]
    w = [t[2][k] - t[0][k] for k in range(3)]
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def exactly_collinear(face):
    """whether the fp32 face [3, 3] has three collinear (or coincident) vertices, over the rationals"""
    return _normal(_ints(face)[0]) == (0, 0, 0)


def _apex(s):
    """the vertex whose two edges carry the ends of the face's cut with the other plane: alone on its side, or on the plane with the
    two others strictly on one side"""
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        if s[i] != 0 and s[j] * s[i] <= 0 and s[k] * s[i] <= 0:
            return i
        if s[i] == 0 and s[j] * s[k] > 0:
            return i
    raise AssertionError("no apex: the caller rejects faces on one side")


def _code(kind, coplanar, s):
    return kind | (COPLANAR if coplanar else 0) | (s << 4)


def _coplanar(A, B, shared_a, shared_b, s):
    n = _normal(A)
    drop = 0 if n[0] != 0 else (1 if n[1] != 0 else 2)
    u, v = (drop + 1) % 3, (drop + 2) % 3

    def o2(p, q, r):
        return _sgn((q[u] - p[u]) * (r[v] - p[v]) - (q[v] - p[v]) * (r[u] - p[u]))
    oa, ob = o2(*A), o2(*B)
    ea = [[o2(A[i], A[(i + 1) % 3], B[k]) * oa for k in range(3)] for i in range(3)]     # >= 0: B_k on the inner side of A's edge i
    eb = [[o2(B[i], B[(i + 1) % 3], A[k]) * ob for k in range(3)] for i in range(3)]
    proper = (not any(all(ea[i][k] <= 0 for k in range(3)) for i in range(3))
              and not any(all(eb[i][k] <= 0 for k in range(3)) for i in range(3)))
    reported = (any(not shared_b[k] and all(ea[i][k] >= 0 for i in range(3)) for k in range(3))
                or any(not shared_a[k] and all(eb[i][k] >= 0 for i in range(3)) for k in range(3))
                or any(ea[i][j] * ea[i][(j + 1) % 3] < 0 and eb[j][i] * eb[j][(i + 1) % 3] < 0 for i in range(3) for j in range(3)))
    return _code(PROPER if proper else TOUCH, True, s) if reported else 0


def pair_code(a, b):
    """the code of the pair of usable fp32 faces a, b [3, 3], 0 when it is not reported -- with Python integers"""
    a, b = np.asarray(a, np.float32).reshape(3, 3), np.asarray(b, np.float32).reshape(3, 3)
    shared_a = [any(bool((p == q).all()) for q in b) for p in a]
    shared_b = [any(bool((p == q).all()) for q in a) for p in b]
    s = sum(shared_a)
    if s == 3:
        return _code(PROPER, True, 3)
    A, B = _ints(a, b)
    sb = [_sgn(_o3(A[0], A[1], A[2], p)) for p in B]
    sa = [_sgn(_o3(B[0], B[1], B[2], p)) for p in A]
    if sb == [0, 0, 0]:
        return _coplanar(A, B, shared_a, shared_b, s)
    if min(sb) > 0 or max(sb) < 0 or min(sa) > 0 or max(sa) < 0:
        return 0
    if s == 2:                                           # both cuts are the shared edge
        return 0
    ia, ib = _apex(sa), _apex(sb)
    pa, pb = A[ia], B[ib]
    c = []
    for x in (1, 2):
        ja = (ia + x) % 3
        for y in (1, 2):
            jb = (ib + y) % 3
            c.append(_sgn(_o3(pa, A[ja], pb, B[jb])) * _sgn(sa[ja] - sa[ia]) * _sgn(sb[jb] - sb[ib]))
    pos, neg = any(x > 0 for x in c), any(x < 0 for x in c)
    if (pos and not neg and 0 not in c) or (neg and not pos and 0 not in c):
        return 0
    both = pos and neg
    segment = both and sa[ia] != 0 and sb[ib] != 0
    if s == 1 and not segment:
        return 0
    proper = both and min(sa) < 0 < max(sa) and min(sb) < 0 < max(sb)
    return _code(PROPER if proper else TOUCH, False, s)


# ---- the device ------------------------------------------------------------------------------------------------------------------

def _kinds(kinds):
    if isinstance(kinds, str):
        kinds = KINDS if kinds == "all" else (kinds,)
    kinds = tuple(kinds)
    if not kinds or any(k not in KINDS for k in kinds):
        raise ValueError(f"kinds: a non-empty selection of {KINDS}, got {kinds!r}")
    return kinds


def _host_faces(ix, idx):
    """fp32 [len(idx), 3, 3] on the host: the vertices of the faces ``idx`` (all with valid indices)"""
    f = ix.faces[torch.as_tensor(idx, dtype=torch.long, device=ix.device)].long()
    return ix.verts[f].cpu().numpy()


def _late_faces(ix, state, side):
    """The faces the device left undecided (state 5): their collinearity, and the pairs of the usable ones with every other usable face,
    all with Python integers.  Returns (list of (i, j, code, s) over the candidates, collinear count)."""
    late = torch.nonzero(state == STATE_UNRESOLVED).reshape(-1).tolist()
    tri = _host_faces(ix, late)
    usable_late = [g for g, t in zip(late, tri) if not exactly_collinear(t)]
    n_collinear = len(late) - len(usable_late)
    if not usable_late:
        return [], n_collinear
    st = state.cpu().numpy()
    ok = np.nonzero(st == 0)[0].tolist() + usable_late
    faces = _host_faces(ix, ok)
    lo, hi = faces.min(1), faces.max(1)
    where = {g: n for n, g in enumerate(ok)}
    side = None if side is None else side.cpu().numpy()
    seen, out = set(), []
    for g in usable_late:
        n = where[g]
        hit = np.nonzero(((lo[n] <= hi) & (lo <= hi[n])).all(1))[0]
        for m in hit:
            h = ok[m]
            key = (min(g, h), max(g, h))
            if h == g or key in seen or (side is not None and side[g] == side[h]):
                continue
            seen.add(key)
            a, b = faces[where[key[0]]], faces[where[key[1]]]
            c = pair_code(a, b)
            out.append((key[0], key[1], c, sum(any(bool((p == q).all()) for q in b) for p in a)))
    return out, n_collinear


@torch.no_grad()
def _search(ix, kinds=KINDS, between=None, brute=False):
    """(pairs, code, flags, report) on the index's device"""
    kinds = _kinds(kinds)
    F, dev = ix.F, ix.device
    side = None
    if between is not None:
        side = as_tensor(between)
        if side.dim() != 1 or side.shape[0] != F or side.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"between: a bool mask of {F} faces, got {tuple(side.shape)} {side.dtype}")
        side = (side.to(dev) != 0).to(torch.uint8).contiguous()
    st = stream(dev)
    buf, _ = ix._ray_tree()
    ws = workspace(lib.nsa_tri_isect_workspace(F), dev)
    state = torch.empty(F, dtype=torch.uint8, device=dev)
    totals = torch.zeros(16, dtype=torch.int64, device=dev)
    flags = BRUTE if brute else 0
    mesh = (buf.data_ptr(), ix.verts.data_ptr(), ix.V, ix.faces.data_ptr(), F, side.data_ptr() if side is not None else None, flags)
    check(lib.nsa_tri_isect_count(*mesh, ws.data_ptr(), state.data_ptr(), totals.data_ptr(), st))
    t = [int(x) for x in totals.cpu()]
    n = t[0]
    pairs = torch.empty(n, 2, dtype=torch.int64, device=dev)
    code = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        check(lib.nsa_tri_isect_emit(*mesh, ws.data_ptr(), state.data_ptr(), n, pairs.data_ptr(), code.data_ptr(), st))
    by_s, n_host, n_collinear = list(t[1:5]), 0, t[11]
    late = (code & 3) == UNRESOLVED
    if bool(late.any()):                                  # pairs beyond the device's width
        where = torch.nonzero(late).reshape(-1)
        lp = pairs[where].cpu().numpy()
        fa, fb = _host_faces(ix, lp[:, 0]), _host_faces(ix, lp[:, 1])
        new = torch.tensor([pair_code(a, b) for a, b in zip(fa, fb)], dtype=torch.uint8, device=dev)
        code[where] = new
        n_host += len(lp)
        keep = code != 0
        pairs, code = pairs[keep], code[keep]
    if t[12]:                                             # faces beyond it
        extra, more = _late_faces(ix, state, side)
        n_collinear += more
        n_host += len(extra)
        for _, _, _, s in extra:
            by_s[s] += 1
        extra = [e for e in extra if e[2]]
        if extra:
            pairs = torch.cat([pairs, torch.tensor([e[:2] for e in extra], dtype=torch.int64, device=dev).reshape(-1, 2)])
            code = torch.cat([code, torch.tensor([e[2] for e in extra], dtype=torch.uint8, device=dev)])
    order = torch.argsort(pairs[:, 0] * F + pairs[:, 1])
    pairs, code = pairs[order], code[order]
    kind = code & 3
    report = {"n_faces": F, "n_candidates": sum(by_s), "n_candidates_s": by_s, "n_stage1": t[5], "n_exact": t[6], "n_host": n_host,
              "n_skipped": dict(zip(CAUSES, t[8:11] + [n_collinear])), "n_proper": int((kind == PROPER).sum()),
              "n_touch": int((kind == TOUCH).sum())}
    if len(kinds) < 2:
        keep = kind == (PROPER if kinds[0] == "proper" else TOUCH)
        pairs, code = pairs[keep], code[keep]
    face_flags = torch.zeros(F, dtype=torch.uint8, device=dev)
    for bit, k in ((1, PROPER), (2, TOUCH)):
        hit = torch.zeros(F, dtype=torch.bool, device=dev)
        hit[pairs[(code & 3) == k].reshape(-1)] = True
        face_flags |= hit.to(torch.uint8) * bit
    return pairs, code, face_flags, report


def _index(mesh, device="cuda"):
    if isinstance(mesh, TriIndex):
        return mesh, False, mesh.device
    need_gpu("mesh_intersect")
    m, was_numpy, orig = mesh_dict_tensors(mesh, device)
    if m["verts"].shape[0] == 0 or m["faces"].shape[0] == 0:
        return None, was_numpy, orig
    return TriIndex(m["verts"], m["faces"]), was_numpy, orig


def self_intersections(mesh, kinds=KINDS, between=None, brute=False, return_report=False, device="cuda"):
    """(pairs, code, flags) of ``mesh`` (a dict with ``verts`` [V, 3] and ``faces`` [F, 3], numpy or torch, or a ``mesh_eval.TriIndex``),
    as the module's head describes them; ``return_report=True`` appends a dict: n_faces, n_candidates (pairs of usable faces whose
    exact boxes overlap) and its split n_candidates_s by shared positions, n_stage1 / n_exact / n_host (candidates decided by the
    float64 filter, by the device's integers, by Python's), n_skipped by cause, n_proper and n_touch (of all kinds, whatever
    ``kinds`` selects)."""
    kinds = _kinds(kinds)
    ix, was_numpy, orig = _index(mesh, device)
    if ix is None:
        F = int(mesh["faces"].shape[0])
        out = (torch.zeros(0, 2, dtype=torch.int64), torch.zeros(0, dtype=torch.uint8), torch.zeros(F, dtype=torch.uint8))
        report = {"n_faces": F, "n_candidates": 0, "n_candidates_s": [0, 0, 0, 0], "n_stage1": 0, "n_exact": 0, "n_host": 0,
                  "n_skipped": dict.fromkeys(CAUSES, 0), "n_proper": 0, "n_touch": 0}
    else:
        *out, report = _search(ix, kinds, between, brute)
    out = tuple(x.cpu().numpy() if was_numpy else (x.to(orig) if orig is not None else x) for x in out)
    return out + (report,) if return_report else out


def is_embedded(mesh, device="cuda"):
    """whether no two faces of ``mesh`` meet properly (touching pairs are allowed)"""
    return self_intersections(mesh, kinds=("proper",), device=device)[0].shape[0] == 0


def format_report(r):
    sk = r["n_skipped"]
    return [f"faces {r['n_faces']}, skipped {sum(sk.values())} (" + ", ".join(f"{k} {v}" for k, v in sk.items()) + ")",
            f"candidate pairs {r['n_candidates']} (sharing 0 / 1 / 2 / 3 positions: " + " / ".join(map(str, r["n_candidates_s"])) + ")",
            f"decided by the float64 filter {r['n_stage1']}, by 256-bit integers {r['n_exact']}, on the host {r['n_host']}",
            f"proper pairs {r['n_proper']}, touching pairs {r['n_touch']}: " + ("embedded" if r["n_proper"] == 0 else "NOT embedded")]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nicer_slam_amd.mesh_intersect", description=__doc__.splitlines()[0])
    ap.add_argument("mesh")
    ap.add_argument("--kinds", choices=("proper", "touch", "all"), default="all")
    ap.add_argument("--brute", action="store_true", help="test all pairs on the device instead of walking the tree")
    ap.add_argument("--out", metavar="FLAGGED.ply", help="the input with the vertices of flagged faces coloured: red proper, yellow touch")
    ap.add_argument("--pairs", metavar="PAIRS.npy", help="int64 [n, 3]: i, j, code")
    ap.add_argument("--json", action="store_true", help="print the report as one JSON object")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("mesh_intersect: needs a GPU", file=sys.stderr)
        raise SystemExit(2)
    try:
        mesh = read_ply(a.mesh)
        pairs, code, flags, r = self_intersections(mesh, kinds=a.kinds, brute=a.brute, return_report=True)
        if a.pairs:
            np.save(a.pairs, np.concatenate([pairs, code[:, None].astype(np.int64)], 1))
        if a.out:
            col = np.full(mesh["verts"].shape, 0.7, np.float32)
            f = np.asarray(mesh["faces"]).reshape(-1, 3)
            col[f[(flags & 2) != 0].reshape(-1)] = (1.0, 1.0, 0.0)
            col[f[(flags & 1) != 0].reshape(-1)] = (1.0, 0.0, 0.0)
            write_mesh_ply(a.out, dict(mesh, colors=col))
    except (ValueError, OSError) as e:
        print(f"mesh_intersect: {e}", file=sys.stderr)
        raise SystemExit(2)
    r = dict(r, embedded=r["n_proper"] == 0, n_returned=int(len(pairs)))
    print(json.dumps(r) if a.json else "\n".join(format_report(r) + ([f"-> {a.out}"] if a.out else [])))
    return r


if __name__ == "__main__":
    main()
