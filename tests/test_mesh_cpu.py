"""Mesh extraction without a GPU: the generated case table, its watertightness over every pair of neighbouring cells, the numpy
oracle (tests/mc_ref.py) on analytic volumes, the C-ABI argument checks and the PLY writer."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import mc_ref
from nicer_slam_amd import mesh_table as MT


def test_committed_table_equals_generator_output():
    with open(MT.HEADER, "rb") as f:
        assert f.read() == MT.header_text().encode()
    assert MT.MAX_TRIS == 5
    assert len(MT.TABLE[0]) == 0 and len(MT.TABLE[255]) == 0


def _cell_tris(case):
    """Triangles of one case as tuples of cube edges, each edge named by its two corner offsets (frozenset)."""
    out = []
    for t in MT.TABLE[case]:
        out.append(tuple(frozenset((MT.CORNERS[MT.EDGES[e][1]], MT.CORNERS[MT.EDGES[e][2]])) for e in t))
    return out


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_neighbouring_cells_are_watertight_for_every_sign_pattern(axis):
    """Two cells sharing the face at axis = 1: all 2^12 sign patterns of their 12 samples.  Every mesh edge on the shared face is
    used exactly twice, in opposite directions, and every triangle uses only crossing edges of its own cell."""
    samples = [p for p in itertools.product(*[range(3 if k == axis else 2) for k in range(3)])]
    assert len(samples) == 12
    for bits in range(1 << 12):
        inside = {p: (bits >> i) & 1 for i, p in enumerate(samples)}
        directed = {}
        for shift in (0, 1):
            base = tuple(shift if k == axis else 0 for k in range(3))
            case = sum(inside[tuple(base[k] + c[k] for k in range(3))] << i for i, c in enumerate(MT.CORNERS))
            for tri in _cell_tris(case):
                glob = []
                for e in tri:
                    a, b = (tuple(base[k] + c[k] for k in range(3)) for c in e)
                    assert inside[a] != inside[b], "triangle on a non-crossing edge"
                    glob.append(frozenset((a, b)))
                for i in range(3):
                    p, q = glob[i], glob[(i + 1) % 3]
                    # an edge between two vertices on the shared face (both grid edges lie in the plane axis == 1)
                    if all(all(c[axis] == 1 for c in g) for g in (p, q)):
                        directed[(p, q)] = directed.get((p, q), 0) + 1
        for (p, q), n in directed.items():
            assert n == 1 and directed.get((q, p)) == 1, (axis, bits)


def _sphere(n, r, centre=(0.0, 0.0, 0.0), lo=-1.0, hi=1.0):
    ax = np.linspace(lo, hi, n, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - np.float32(r), ax


def test_oracle_sphere_closed_outward_euler_2():
    vol, ax = _sphere(40, 0.6)
    step = float(ax[1] - ax[0])
    m = mc_ref.marching_cubes(vol, 0.0, (step,) * 3, (float(ax[0]),) * 3)
    assert m["faces"].shape[0] > 1000
    assert mc_ref.is_closed(m["faces"])
    assert mc_ref.euler(m["faces"]) == 2
    v = m["verts"].astype(np.float64)
    f = m["faces"]
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    c = v[f].mean(1)
    assert ((n * c).sum(1) > 0).all()                                        # away from the centre
    assert (np.abs(np.linalg.norm(v, axis=1) - 0.6) < step).all()
    assert ((m["normals"] * v).sum(1) > 0).all()                             # vertex normals outward too
    np.testing.assert_allclose(np.linalg.norm(m["normals"], axis=1), 1, atol=1e-6)


def test_oracle_torus_and_two_spheres():
    ax = np.linspace(-1, 1, 48, dtype=np.float32)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    torus = np.sqrt((np.sqrt(x ** 2 + y ** 2) - 0.55) ** 2 + z ** 2) - 0.2
    m = mc_ref.marching_cubes(torus.astype(np.float32), 0.0)
    assert mc_ref.is_closed(m["faces"]) and mc_ref.euler(m["faces"]) == 0
    a, _ = _sphere(48, 0.3, (-0.45, 0, 0))
    b, _ = _sphere(48, 0.3, (0.45, 0.1, 0))
    m = mc_ref.marching_cubes(np.minimum(a, b), 0.0)
    assert mc_ref.is_closed(m["faces"]) and mc_ref.euler(m["faces"]) == 4


def test_oracle_vertex_expression_and_order():
    """The fp32 vertex of the header (origin + spacing * (index + t * axis)) and the (sample, axis) order on a tiny volume."""
    vol = np.array([[[1.0, -1.0], [1.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]]], np.float32)      # sample (0,0,1) inside
    m = mc_ref.marching_cubes(vol, 0.25, (0.5, 2.0, 3.0), (1.0, -1.0, 0.5))
    # edges of sample (0,0,0) axis z (t = 0.75 / -2), then sample (0,0,1) axes x, y
    t = np.float32(0.25 - 1.0) / np.float32(-1.0 - 1.0)
    t2 = np.float32(0.25 + 1.0) / np.float32(1.0 + 1.0)
    exp = np.array([[1.0, -1.0, 0.5 + 3.0 * t], [1.0 + 0.5 * t2, -1.0, 3.5], [1.0, -1.0 + 2.0 * t2, 3.5]], np.float32)
    np.testing.assert_array_equal(m["verts"], exp)
    assert m["faces"].shape == (1, 3) and sorted(m["faces"][0].tolist()) == [0, 1, 2]
    n = np.cross(m["verts"][m["faces"][0, 1]] - m["verts"][m["faces"][0, 0]], m["verts"][m["faces"][0, 2]] - m["verts"][m["faces"][0, 0]])
    assert n @ np.array([1, 1, -1]) > 0                                       # away from the inside corner (0, 0, 1)


def test_oracle_nonfinite_cells_emit_no_faces():
    vol, _ = _sphere(12, 0.5)
    vol[8, 5, 5] = np.nan                                                 # next to the surface
    vol[0, 0, 0] = np.inf
    m = mc_ref.marching_cubes(vol, 0.0)
    full = mc_ref.marching_cubes(_sphere(12, 0.5)[0], 0.0)
    assert m["faces"].shape[0] < full["faces"].shape[0]


def test_marching_cubes_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib
    NSA_EBADARG, NSA_EMESH_TOO_LARGE = 4, 6
    assert b"int32" in lib.nsa_strerror(NSA_EMESH_TOO_LARGE)
    fake = ctypes.c_void_p(4096)                                             # never dereferenced: rejected before any launch
    tot = ctypes.c_void_p(8192)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)                                  # noqa: E731
    one, zero = f3(1, 1, 1), f3(0, 0, 0)
    assert lib.nsa_marching_cubes_workspace(64, 64, 64) > 0
    assert lib.nsa_marching_cubes_workspace(2048, 2048, 2048) == 0          # more than 2^31 samples
    count, emit = lib.nsa_marching_cubes_count, lib.nsa_marching_cubes_emit
    assert count(None, 8, 8, 8, 0.0, fake, tot, None) == NSA_EBADARG
    assert count(fake, 8, 8, 8, 0.0, None, tot, None) == NSA_EBADARG
    assert count(fake, 8, 8, 8, 0.0, fake, None, None) == NSA_EBADARG
    assert count(fake, 8, 8, 8, float("nan"), fake, tot, None) == NSA_EBADARG
    assert count(fake, 8, 8, 8, float("inf"), fake, tot, None) == NSA_EBADARG
    assert count(fake, 2048, 2048, 2048, 0.0, fake, tot, None) == NSA_EBADARG
    ok = (fake, 8, 8, 8, 0.0)
    assert emit(None, 8, 8, 8, 0.0, zero, one, fake, 10, 10, fake, fake, fake, None) == NSA_EBADARG
    assert emit(*ok, None, one, fake, 10, 10, fake, fake, fake, None) == NSA_EBADARG
    assert emit(*ok, zero, None, fake, 10, 10, fake, fake, fake, None) == NSA_EBADARG
    assert emit(*ok, zero, one, None, 10, 10, fake, fake, fake, None) == NSA_EBADARG
    assert emit(fake, 8, 8, 8, float("nan"), zero, one, fake, 10, 10, fake, fake, fake, None) == NSA_EBADARG
    for bad in (f3(1, 0, 1), f3(1, -1, 1), f3(1, float("inf"), 1), f3(float("nan"), 1, 1)):
        assert emit(*ok, zero, bad, fake, 10, 10, fake, fake, fake, None) == NSA_EBADARG
    assert emit(*ok, f3(0, float("nan"), 0), one, fake, 10, 10, fake, fake, fake, None) == NSA_EBADARG
    assert emit(*ok, zero, one, fake, 10, 10, None, fake, fake, None) == NSA_EBADARG
    assert emit(*ok, zero, one, fake, 10, 10, fake, None, fake, None) == NSA_EBADARG
    assert emit(*ok, zero, one, fake, 10, 10, fake, fake, None, None) == NSA_EBADARG
    assert emit(*ok, zero, one, fake, 1 << 31, 10, fake, fake, fake, None) == NSA_EMESH_TOO_LARGE
    assert emit(*ok, zero, one, fake, 10, 1 << 31, fake, fake, fake, None) == NSA_EMESH_TOO_LARGE
    # nothing to write: no launch, no error
    assert emit(*ok, zero, one, fake, 0, 0, None, None, None, None) == 0
    assert emit(fake, 1, 8, 8, 0.0, zero, one, fake, 10, 10, fake, fake, fake, None) == 0


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    props = [h.split() for h in head if h.startswith("property ") and "list" not in h]
    dt = np.dtype([(p[2], {"float": "<f4", "uchar": "u1"}[p[1]]) for p in props])
    v = np.frombuffer(data, dt, nv, end)
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    f = np.frombuffer(data, fdt, nf, end + nv * dt.itemsize)
    assert end + nv * dt.itemsize + nf * fdt.itemsize == len(data)
    assert (f["n"] == 3).all()
    return v, f["v"]


@pytest.mark.parametrize("colours", [False, True])
def test_write_ply_round_trip(tmp_path, colours):
    from nicer_slam_amd.inference import write_ply
    vol, _ = _sphere(10, 0.5)
    m = {k: torch.from_numpy(v) for k, v in mc_ref.marching_cubes(vol, 0.0).items()}
    if colours:
        m["colors"] = torch.rand(m["verts"].shape[0], 3)
    p = tmp_path / "m.ply"
    write_ply(str(p), m)
    v, f = _read_ply(str(p))
    np.testing.assert_array_equal(np.stack([v["x"], v["y"], v["z"]], 1), m["verts"].numpy())
    np.testing.assert_array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), m["normals"].numpy())
    np.testing.assert_array_equal(f, m["faces"].numpy())
    if colours:
        rgb = np.stack([v["red"], v["green"], v["blue"]], 1)
        np.testing.assert_array_equal(rgb, np.rint(m["colors"].numpy() * 255).astype(np.uint8))
    else:
        assert "red" not in v.dtype.names


def test_write_ply_without_faces(tmp_path):
    from nicer_slam_amd.inference import write_ply
    m = dict(verts=torch.rand(4, 3), normals=torch.rand(4, 3), faces=torch.zeros(0, 3, dtype=torch.int32))
    write_ply(str(tmp_path / "e.ply"), m)
    v, f = _read_ply(str(tmp_path / "e.ply"))
    assert v.shape == (4,) and f.shape == (0, 3)
    empty = dict(verts=torch.zeros(0, 3), normals=torch.zeros(0, 3), faces=torch.zeros(0, 3, dtype=torch.int32),
                 colors=torch.zeros(0, 3))
    write_ply(str(tmp_path / "z.ply"), empty)
    v, f = _read_ply(str(tmp_path / "z.ply"))
    assert v.shape == (0,) and f.shape == (0, 3)
