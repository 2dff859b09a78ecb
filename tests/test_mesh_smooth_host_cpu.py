"""The bodies the smoothing kernels call (csrc/smooth_passes.hpp: the ring's offsets, fill and row lookup, the state and neighbour
passes, one vertex's step, one vertex's area normal), compiled by the host compiler with -ffp-contract=off into
tests/smooth_host_check.cpp and held to tests/smooth_ref.py bit for bit; once plain and once under the address and
undefined-behaviour sanitizers where the host compiler has them."""
import numpy as np
import pytest

import clean_ref
import host_program
from host_program import words
import simplify_ref
import smooth_ref as S
import topology_ref as T


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("smooth_host_check.cpp", tmp_path_factory.mktemp("smooth_host"), sanitize, flags=("-ffp-contract=off",))

    def call(path, verts, faces, factors, boundary, fixed=None, max_move=None):
        v = np.ascontiguousarray(verts, np.float32)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        fx = np.zeros(len(v), np.uint32) if fixed is None else (np.asarray(fixed).reshape(-1) != 0).astype(np.uint32)
        mm = np.array([np.inf if max_move is None else max_move], np.float64)
        head = [len(v), len(f), len(factors), S.BOUNDARY.index(boundary), int(max_move is not None), int(mm.view(np.uint64)[0])]
        with open(path, "w") as fh:
            fh.write("\n".join([words(head), words(v.view(np.uint32)), words(f), words(fx),
                                words(np.asarray(factors, np.float64).view(np.uint64))]) + "\n")
        out = host_program.run(exe, [str(path)], 120, sanitize)
        assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr
        rows = [np.array(line.split(), np.int64) for line in out.stdout.split("\n")[:6]]
        return dict(ring_start=rows[0], ring=rows[1], ring_edge=rows[2], out=rows[3].astype(np.uint32).reshape(-1, 3), state=rows[4],
                    normals=rows[5].astype(np.uint32).reshape(-1, 3))
    return call


def _compare(got, verts, faces, factors, boundary, fixed=None, max_move=None):
    v = np.ascontiguousarray(verts, np.float32)
    ring = S.vertex_ring(faces, len(v))
    for k in ("ring_start", "ring", "ring_edge"):
        assert got[k].tolist() == ring[k].tolist(), k
    out, state = S.smooth_steps(v, faces, factors, boundary, fixed, max_move, ring=ring)
    assert got["state"].tolist() == state.tolist()
    assert (got["out"] == out.view(np.uint32)).all(), int((got["out"] != out.view(np.uint32)).any(1).sum())
    assert (got["normals"] == S.vertex_normals(v, faces, "area").view(np.uint32)).all()


CASES = {
    "tetrahedron": lambda: (np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3]], np.float32), T.TET),
    "noisy icosphere": lambda: S.noisy_icosphere(2)[:2],
    "fan": lambda: S.fan_mesh(40),
    "grid with a hole": lambda: S.grid_mesh(9, (3, 3, 2), 0.5),
    "high indices": lambda: (S.index_only_mesh(*T.high_index_faces(300)), T.high_index_faces(300)[0]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bodies_equal_the_oracle_bit_for_bit(run, tmp_path, name):
    v, f = CASES[name]()
    rng = np.random.default_rng(1)
    fixed = rng.random(len(v)) < 0.2
    for factors, boundary, fx, mm in (([0.5], "curve", None, None), ([0.5, -0.53] * 3, "free", None, None),
                                      ([0.5, 0.5, 0.5], "fixed", fixed, None), ([0.7, -0.75], "curve", fixed, 0.01), ([], "free", None, None)):
        got = run(tmp_path / "case.txt", v, f, factors, boundary, fx, mm)
        _compare(got, v, f, factors, boundary, fx, mm)


def test_adversarial_lists_and_non_finite_vertices(run, tmp_path):
    for name, (f, V) in clean_ref.adversarial_cases(200).items():
        v = simplify_ref.adversarial_mesh(f, V)
        got = run(tmp_path / "case.txt", v, f, [0.5, -0.53, 0.5], "curve")
        _compare(got, v, f, [0.5, -0.53, 0.5], "curve")
        bad = ~np.isfinite(v).all(1)
        assert (got["out"][bad] == v.view(np.uint32)[bad]).all() and np.isfinite(got["out"][~bad].view(np.float32)).all()
