"""The bodies the k-nearest-neighbour and normal kernels call (csrc/normals_passes.hpp: a query's candidate list and its final order, a
neighbourhood's mean and scatter, the cyclic Jacobi, the normal's orientation and validity), compiled by the host compiler with
-ffp-contract=off into tests/cloud_normals_host_check.cpp and held to tests/normals_ref.py bit for bit; once plain and once under the
address and undefined-behaviour sanitizers where the host compiler has them."""
import numpy as np
import pytest

import host_program
from host_program import bits32, words
import normals_ref as N


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("cloud_normals_host_check.cpp", tmp_path_factory.mktemp("cloud_normals_host"),
                             sanitize, flags=("-ffp-contract=off",))

    def call(mode, path, lines):
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        out = host_program.run(exe, [mode, str(path)], 300, sanitize)
        assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr
        return out.stdout.split("\n")
    return call


def _knn(run, path, q, t, k, max_dist, order):
    strict = max_dist < np.inf
    r2 = np.float32(max_dist * max_dist) if strict else np.float32(np.inf)
    rows = run("knn", path, [words([len(q), len(t), k, int(strict), int(np.array([r2]).view(np.uint32)[0])]), bits32(t), bits32(q),
                             words(order)])
    return (np.array(rows[1].split(), np.uint32).reshape(len(q), k), np.array(rows[0].split(), np.int64).reshape(len(q), k),
            np.array(rows[2].split(), np.int64))


@pytest.mark.parametrize("k", [1, 2, 8, 9, 30, 64])
def test_candidate_list_equals_the_reference_in_any_order_of_offers(run, tmp_path, k):
    """uniform targets with NaN and inf rows, the lattice with its exact ties, duplicates; offered ascending, descending and shuffled;
    without and with a radius that leaves most lists short"""
    rng = np.random.default_rng(k)
    t = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    t[5] = np.nan
    t[17, 1] = np.inf
    t[40:60] = t[39]
    q = np.concatenate([rng.uniform(-1.2, 1.2, (20, 3)).astype(np.float32), t[39:40], [[np.nan, 0, 0]]]).astype(np.float32)
    lat = N.lattice(5)
    lq = np.concatenate([lat[::7], lat[::11] + np.float32(0.5)])
    for targets, queries, radius in ((t, q, np.inf), (t, q, 0.35), (lat, lq, np.inf), (lat, lq, 1.5)):
        ref = N.knn_brute(queries, targets, k, radius)
        n = len(targets)
        for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
            dist, idx, count = _knn(run, tmp_path / "case.txt", queries, targets, k, radius, order)
            assert (idx == ref[1]).all() and (count == ref[2]).all()
            assert (dist == ref[0].view(np.uint32)).all()


def _normals(run, path, points, idx, count, origin, viewpoint, want_eig=True):
    m, k = idx.shape
    v = np.zeros((0, 3), np.float32) if viewpoint is None else np.asarray(viewpoint, np.float32).reshape(-1, 3)
    rows = run("normals", path, [words([len(points), m, k, len(v), int(want_eig)]), bits32(points), words(idx), words(count), bits32(origin),
                                 bits32(v)])
    out = dict(normals=np.array(rows[0].split(), np.uint32).reshape(m, 3))
    if want_eig:
        out["eigenvalues"] = np.array(rows[1].split(), np.uint64).reshape(m, 3)
    out["valid"] = np.array(rows[1 + want_eig].split(), np.int64).astype(bool)
    out["sweeps"] = np.array(rows[2 + want_eig].split(), np.int64)
    return out


def _compare(got, ref):
    assert (got["valid"] == ref["valid"]).all()
    assert (got["normals"] == ref["normals"].view(np.uint32)).all(), np.nonzero(got["normals"] != ref["normals"].view(np.uint32))[0]
    if "eigenvalues" in got:
        assert (got["eigenvalues"] == ref["eigenvalues"].view(np.uint64)).all()


@pytest.mark.parametrize("family", N.FAMILIES)
def test_scatter_jacobi_and_normal_equal_the_reference_bit_for_bit(run, tmp_path, family):
    rng = np.random.default_rng(N.FAMILIES.index(family))
    points, idx, count = N.neighbourhoods(family, 150, rng)
    origin = points[idx[:, 0]]
    for viewpoint in (None, np.float32([0.3, -2.0, 1.0]), rng.normal(size=(len(idx), 3)).astype(np.float32)):
        ref = N.normals_from(points, idx, count, origin, viewpoint)
        got = _normals(run, tmp_path / "case.txt", points, idx, count, origin, viewpoint)
        _compare(got, ref)
        ok = count >= 1
        assert (got["sweeps"][ok] == ref["sweeps"][ok]).all()
        assert ref["valid"].sum() > 100


def test_rows_that_are_not_valid(run, tmp_path):
    """count 0, 1, 2, above k; an index below 0 and one past n inside and behind count; collinear, duplicate and NaN points; an exact plane"""
    rng = np.random.default_rng(9)
    k = 8
    points = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    points[8:16] = np.float32([0.5, -0.25, 0.125]) + np.outer(np.arange(8), np.float32([0.25, 0, 0]))    # collinear along x, exact: w1 == 0
    points[16:24] = points[16]                                                                             # duplicates
    points[24:32, 2] = 0.5                                                                                 # an exact plane: w0 == 0
    points[24:32, :2] = np.round(points[24:32, :2] * 64) / 64
    points[33] = np.nan
    idx = np.arange(64).reshape(8, 8)
    count = np.full(8, 8)
    idx = np.concatenate([idx, idx[:6]])
    count = np.concatenate([count, [0, 1, 2, 9, 8, 8]])
    idx[12, 3] = -1
    idx[13, 7] = 64
    idx[0, 7] = 64
    count[0] = 7                                                                                           # behind count: not read
    origin = points[np.clip(idx[:, 0], 0, 63)]
    ref = N.normals_from(points, idx, count, origin)
    assert ref["valid"].tolist() == [True, False, False, True, False, True, True, True, False, False, False, False, False, False]
    assert ref["eigenvalues"][3, 0] == 0.0 and not ref["normals"][~ref["valid"]].any()
    _compare(_normals(run, tmp_path / "case.txt", points, idx, count, origin, None), ref)
    got = _normals(run, tmp_path / "case.txt", points, idx, count, origin, None, want_eig=False)
    _compare(got, ref)
