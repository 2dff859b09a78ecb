"""Vectorised numpy restatement of csrc/mesh_extract.hip (the oracle of tests/test_mesh_*.py): the same generated case table
(nicer_slam_amd/mesh_table.py), the fp32 vertex expression, the interpolated gradient normals and the canonical order
(vertices by (lower sample, axis), faces by (cell, table order)).  DESIGN 4f states the rules."""
import numpy as np

from nicer_slam_amd import mesh_table as MT

COUNT = np.array([len(t) for t in MT.TABLE], np.int64)
EDGES = np.zeros((256, MT.MAX_TRIS, 3), np.int64)
for _c, _tris in enumerate(MT.TABLE):
    for _j, _t in enumerate(_tris):
        EDGES[_c, _j] = _t
# start-corner offset (dx, dy, dz) and axis of each of the 12 edges
EDGE_OFF = np.array([MT.CORNERS[c0] for _, c0, _ in MT.EDGES], np.int64)
EDGE_AXIS = np.array([a for a, _, _ in MT.EDGES], np.int64)


def empty():
    return dict(verts=np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32))


def gradient(vol, spacing):
    """[nx, ny, nz, 3] fp32: central differences inside, one-sided on the border, divided by the spacing."""
    g = np.empty(vol.shape + (3,), np.float32)
    for k in range(3):
        f = np.moveaxis(vol, k, 0)
        out = np.moveaxis(g[..., k], k, 0)
        sp = np.float32(spacing[k])
        out[1:-1] = (f[2:] - f[:-2]) / (np.float32(2) * sp)
        out[0] = (f[1] - f[0]) / sp
        out[-1] = (f[-1] - f[-2]) / sp
    return g


def marching_cubes(vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    vol = np.ascontiguousarray(vol, np.float32)
    nx, ny, nz = vol.shape
    if min(vol.shape) < 2:
        return empty()
    lv = np.float32(level)
    sp = np.asarray(spacing, np.float32)
    org = np.asarray(origin, np.float32)
    fin = np.isfinite(vol)
    ins = vol < lv
    N = vol.size
    strides = (ny * nz, nz, 1)
    with np.errstate(all="ignore"):
        cross = np.zeros(vol.shape + (3,), bool)
        for a in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[a], hi[a] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            cross[lo + (a,)] = fin[lo] & fin[hi] & (ins[lo] != ins[hi])
        flat = cross.reshape(-1)
        ids = np.nonzero(flat)[0]                                    # ascending = (sample, axis) order
        V = ids.size
        vid = np.full(N * 3, -1, np.int64)
        vid[ids] = np.arange(V)
        s, a = ids // 3, ids % 3
        idx = np.stack(np.unravel_index(s, vol.shape), -1)
        stride = np.array(strides, np.int64)[a]
        f0 = vol.reshape(-1)[s]
        f1 = vol.reshape(-1)[s + stride]
        t = (lv - f0) / (f1 - f0)
        c = idx.astype(np.float32)
        c[np.arange(V), a] = c[np.arange(V), a] + t
        verts = org + sp * c
        g = gradient(vol, sp).reshape(-1, 3)
        m = (np.float32(1) - t)[:, None] * g[s] + t[:, None] * g[s + stride]
        ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        unit = (ln > 0) & np.isfinite(ln)
        normals = np.where(unit[:, None], m / np.where(unit, ln, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
    # cells
    cx = np.arange(nx - 1)[:, None, None]
    cy = np.arange(ny - 1)[None, :, None]
    cz = np.arange(nz - 1)[None, None, :]
    cell_s = ((cx * ny + cy) * nz + cz).reshape(-1)
    case = np.zeros(cell_s.shape, np.int64)
    ok = np.ones(cell_s.shape, bool)
    for i, (dx, dy, dz) in enumerate(MT.CORNERS):
        q = cell_s + dx * strides[0] + dy * strides[1] + dz
        case |= ins.reshape(-1)[q].astype(np.int64) << i
        ok &= fin.reshape(-1)[q]
    ntri = np.where(ok, COUNT[case], 0)
    cell = np.repeat(np.arange(cell_s.size), ntri)                    # cells are in ascending s already
    j = np.arange(cell.size) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    e = EDGES[case[cell], j]                                          # [F, 3] cell edges
    owner = cell_s[cell][:, None] + (EDGE_OFF[e] * np.array(strides)).sum(-1)
    faces = vid[owner * 3 + EDGE_AXIS[e]]
    assert (faces >= 0).all()
    return dict(verts=verts.astype(np.float32).reshape(-1, 3), normals=normals.reshape(-1, 3),
                faces=faces.astype(np.int32).reshape(-1, 3))


def edge_counts(faces):
    """{(i, j): uses} over directed mesh edges."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    keys, n = np.unique(d, axis=0, return_counts=True)
    return {tuple(k): int(c) for k, c in zip(keys, n)}


def is_closed(faces):
    """Every directed edge used once and its reverse once: a closed, consistently oriented surface."""
    cnt = edge_counts(faces)
    return all(c == 1 and cnt.get((k[1], k[0])) == 1 for k, c in cnt.items())


def euler(faces):
    f = np.asarray(faces, np.int64)
    V = np.unique(f).size
    und = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    E = np.unique(und, axis=0).shape[0]
    return V - E + f.shape[0]
