"""tests/intersect_ref.py, the rational statement of header Section 25, pinned by hand-built pairs whose answers are known; and the
Python-integer decision of nicer_slam_amd/mesh_intersect.py (the host's route for what the device leaves unresolved) held to it on
the same pairs and on the lattice soup, where nearly every predicate is degenerate."""
import functools

import numpy as np
import pytest

import intersect_ref as R
from nicer_slam_amd import mesh_intersect as M

CASES = R.known_answers()


@pytest.mark.parametrize("name", sorted(CASES))
def test_known_answers(name):
    a, b, kind, coplanar, s = CASES[name]
    want = R.code_of(kind, coplanar, s) if kind else 0
    assert R.shared_positions(a, b) == s
    for x, y in ((a, b), (b, a), (a[[1, 2, 0]], b[[2, 1, 0]])):        # the answer depends on the sets alone
        assert R.pair(x, y) == want
        assert M.pair_code(x, y) == want


def test_candidates_are_exact_boxes():
    a, b = CASES["coplanar and disjoint, boxes overlap"][:2]
    assert len(R.candidates(**R.concat([a, b]))) == 1
    far = b + np.float32(10)
    assert len(R.candidates(**R.concat([a, far]))) == 0
    touching = a + np.array([4, 0, 0], np.float32)                       # closed boxes: sharing a face of the box counts
    assert len(R.candidates(**R.concat([a, touching]))) == 1


def test_the_slanted_plane_needs_exact_signs():
    """the tip exactly on the plane: the float64 determinant is a zero nobody can trust, one fp32 step decides either way"""
    on, above, below = (CASES["near 2^23, the tip %s the plane" % k] for k in ("on", "above", "below"))
    assert (on[2], above[2], below[2]) == (R.TOUCH, 0, R.PROPER)
    assert np.abs(on[1] - above[1]).max() == np.float32(2.0 ** -22) and np.abs(on[1] - below[1]).max() == np.float32(2.0 ** -23)


def test_a_coordinate_of_2_to_the_minus_100():
    a, b, kind, coplanar, s = R.unresolved_case()
    assert R.pair(a, b) == M.pair_code(a, b) == R.code_of(kind, coplanar, s)
    exps = [np.frexp(float(x))[1] for x in np.concatenate([a, b]).reshape(-1) if x != 0]
    assert max(exps) - min(exps) > 59                                      # beyond what 256 bits cover


def test_exactly_collinear_faces():
    line = np.array([(0, 0, 0), (1, 2, 3), (3, 6, 9)], np.float32)
    assert R.face_state(line, [[0, 1, 2]])[0] == 3 and M.exactly_collinear(line)
    assert not M.exactly_collinear(np.array([(0, 0, 0), (1, 2, 3), (3, 6, np.nextafter(np.float32(9), np.float32(10)))], np.float32))
    # exactly collinear, and the float64 cross product of Section 14 is not zero: only the exact stage can tell
    c = R.collinear_case().astype(np.float64)
    u, w = c[1] - c[0], c[2] - c[0]
    assert any(x != 0 for x in (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]))
    assert R.face_state(R.collinear_case(), [[0, 1, 2]])[0] == 4 and M.exactly_collinear(R.collinear_case())


@functools.lru_cache(maxsize=None)
def _lattice():
    mesh = R.lattice_soup()
    return mesh, R.self_intersections(**mesh)


def test_lattice_soup_python_integers_equal_the_rationals():
    mesh, ref = _lattice()
    v, f = mesh["verts"], mesh["faces"]
    assert ref["n_candidates"] > 1000 and ref["n_proper"] > 100 and ref["n_touch"] > 100 and min(ref["n_candidates_s"][:3]) > 10
    got = [(i, j, M.pair_code(v[f[i]], v[f[j]])) for i, j in R.candidates(v, f)]
    got = [g for g in got if g[2]]
    assert [g[:2] for g in got] == [tuple(p) for p in ref["pairs"]]
    assert [g[2] for g in got] == ref["code"].tolist()
    assert (np.bincount(ref["pairs"].reshape(-1), minlength=len(f)) > 0).tolist() == (ref["flags"] != 0).tolist()


def test_between_keeps_pairs_across_the_mask():
    mesh, ref = _lattice()
    mask = np.arange(len(mesh["faces"])) % 3 == 0
    part = R.self_intersections(**mesh, between=mask)
    keep = mask[ref["pairs"][:, 0]] != mask[ref["pairs"][:, 1]]
    assert part["pairs"].tolist() == ref["pairs"][keep].tolist() and part["code"].tolist() == ref["code"][keep].tolist()


def test_argument_checks_without_a_device():
    with pytest.raises(ValueError):
        M._kinds(("crossing",))
    with pytest.raises(ValueError):
        M._kinds(())
    assert M._kinds("all") == M.KINDS and M._kinds("touch") == ("touch",)
