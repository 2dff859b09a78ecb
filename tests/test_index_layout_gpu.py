"""The mesh indexes are laid out as they were before their builds were shared (csrc/octree_build.hpp, csrc/bulk_grid.hpp): the
closest-point grid, the two octrees and the nearest-neighbour grid of a handful of small meshes and clouds, compared exactly --
integers, and fp32 and fp64 bit patterns -- with tests/golden/index_layout.npz, which tests/golden/make_index_layout_fixture.py
recorded from the commit named in tests/golden/index_layout.md.  The float64 oracles of the query tests do not pin the grid (another
grid still gives exact answers); this does.

The cases are the smallest that reach every branch of the two builds: L = 0 and L > 0, an empty grid, one cell, the thin-axis floor,
the large list, skipped faces, a cloud below and one above a wave."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import p2m_ref as P
import winding_ref as W
from test_mesh_closest_cpu import invalid_mesh

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_layout.npz")
GRID_BYTES, NN_GRID_BYTES = 96, 80               # sizeof(tri::Grid), sizeof(bulk::Grid): what the build writes of the first 256 bytes
MESHES = ("box8", "box", "sphere", "mixed", "coincident", "invalid")
CLOUDS = ("one", "seven", "thousand")


def mesh_case(name):
    if name == "box8":                               # 8 usable faces: L = 0, one node
        v, f = P.box_mesh()
        return v, f[:8]
    if name == "box":                                # 12: L = 1
        return P.box_mesh()
    if name == "sphere":
        return P.latlong_sphere(24, 48)[:2]
    if name == "mixed":                              # mixed scales (the large list, a stray component) and faces of every skipped kind
        from test_mesh_closest_gpu import _mixed_mesh
        return _mixed_mesh()[:2]
    if name == "coincident":                         # one leaf, one cell
        return W.coincident_copies(40)
    v, f, _, good = invalid_mesh()                   # no usable face: an empty grid and an empty tree
    return v, np.delete(f, good, 0)


def cloud_case(name):
    rng = np.random.default_rng(20261019)
    if name == "one":
        return np.array([[0.5, -1.0, 2.0]], np.float32)
    if name == "seven":                              # planar: z is the thin axis
        t = rng.uniform(-1, 1, (7, 3))
        t[:, 2] = 0.25
        return t.astype(np.float32)
    t = rng.standard_normal((1000, 3)) * [1.0, 0.5, 2.0]
    t[17] = [np.nan, 0, 0]
    t[500] = [0, np.inf, 0]
    t[999] = [0, 0, -np.inf]
    t[321] = [1e4, -3.0, 2.0]                        # a far outlier: clamped into a border cell
    return t.astype(np.float32)


def queries():
    return np.random.default_rng(257).uniform(-2.0, 2.0, (257, 3)).astype(np.float32)


def record_mesh(name):
    """{key: array} of everything the fixture holds for one mesh"""
    from nicer_slam_amd.mesh_eval import TriIndex
    v, f = mesh_case(name)
    ix = TriIndex(torch.as_tensor(v).cuda(), torch.as_tensor(np.ascontiguousarray(f), dtype=torch.int32).cuda())
    lay, q = ix.layout(), torch.as_tensor(queries()).cuda()
    out = {"grid": ix.buf[:GRID_BYTES].cpu().numpy(),
           "cells": np.array(lay["cells"], np.int64), "cell_size": np.array(lay["cell size"], np.float32),
           "faces": np.array([lay["grid faces"], lay["large faces"], lay["skipped faces"]], np.int64),
           "skipped": np.array(ix.skipped, np.int64)}
    for key, tree in (("winding", ix.winding_layout()), ("ray", ix.ray_layout())):
        out[key] = np.array([tree["L"], tree["nodes"], tree["usable faces"], tree["bytes"]], np.int64)
    out["evaluated"] = ix.query(q, counts=True)[3].cpu().numpy()
    d2, _, _, n_eval, n_cells = ix.query(q, counts=True, squared=True, max_dist=math.inf)
    out.update(bounded_d2=d2.cpu().numpy(), bounded_evaluated=n_eval.cpu().numpy(), bounded_cells=n_cells.cpu().numpy())
    return out


def record_cloud(name):
    from nicer_slam_amd.mesh_eval import NNIndex
    ix = NNIndex(torch.as_tensor(cloud_case(name)).cuda())
    lo, h, R, counts = ix.grid()
    return {"grid": ix.buf[:NN_GRID_BYTES].cpu().numpy(), "lo": lo, "h": h, "R": R, "counts": counts.cpu().numpy()}


def record():
    """the whole fixture but its provenance"""
    out = {}
    for kind, names, one in (("mesh", MESHES, record_mesh), ("cloud", CLOUDS, record_cloud)):
        for name in names:
            out.update({f"{kind}__{name}__{k}": x for k, x in one(name).items()})
    return out


@functools.lru_cache(maxsize=None)
def _fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _compare(kind, name, got):
    want = {k: x for k, x in _fixture().items() if k.startswith(f"{kind}__{name}__")}
    assert sorted(want) == sorted(f"{kind}__{name}__{k}" for k in got)
    for k, x in got.items():
        w = want[f"{kind}__{name}__{k}"]
        assert x.dtype == w.dtype and x.shape == w.shape, (name, k, x.dtype, w.dtype, x.shape, w.shape)
        assert x.tobytes() == w.tobytes(), (name, k, x.reshape(-1)[:8], w.reshape(-1)[:8])     # bit patterns, NaN included


@pytest.mark.parametrize("name", MESHES)
def test_mesh_indexes_are_laid_out_as_recorded(name):
    got = record_mesh(name)
    print(name, "cells", got["cells"].tolist(), "faces", got["faces"].tolist(), "winding", got["winding"].tolist(), "ray",
          got["ray"].tolist(), "evaluated", int(got["evaluated"].sum()), "cells visited", int(got["bounded_cells"].sum()))
    _compare("mesh", name, got)


@pytest.mark.parametrize("name", CLOUDS)
def test_nearest_neighbour_grid_is_laid_out_as_recorded(name):
    got = record_cloud(name)
    print(name, "R", got["R"].tolist(), "h", got["h"].tolist(), "points in cells", int(got["counts"].sum()))
    _compare("cloud", name, got)


def test_the_fixture_reaches_every_branch_and_names_its_commit():
    z = _fixture()
    assert len(str(z["commit"])) == 40
    L = {name: int(z[f"mesh__{name}__winding"][0]) for name in MESHES}
    assert L["box8"] == 0 and z["mesh__box8__ray"][1] == 1 and L["box"] == 1 and L["sphere"] > 1
    assert z["mesh__coincident__winding"][1] == L["coincident"] + 1 and z["mesh__coincident__cells"].tolist() == [1, 1, 1]
    assert z["mesh__invalid__winding"][1:3].tolist() == [0, 0] and z["mesh__invalid__faces"][:2].tolist() == [0, 0]
    assert z["mesh__mixed__faces"][1] >= 12 and z["mesh__mixed__skipped"].sum() == 7
    assert z["cloud__one__R"].tolist() == [1, 1, 1] and z["cloud__seven__R"][2] == 1 and z["cloud__thousand__counts"].sum() == 997
