"""The bodies the decimation kernels call (csrc/decimate_passes.hpp: the quadric sums and locks, placement and cost, the link count,
the fold test, m1 / m2 / select, the prefix rule, apply, rename and compose), compiled by the host compiler with -ffp-contract=off
into tests/decimate_host_check.cpp, run one item at a time and held to tests/decimate_ref.py bit for bit; once plain and once under
the address and undefined-behaviour sanitizers where the host compiler has them."""
import numpy as np
import pytest

import clean_ref
import decimate_ref as D
import host_program
from host_program import words
import simplify_ref
import smooth_ref as S
import topology_ref as T


def _bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("decimate_host_check.cpp", tmp_path_factory.mktemp("decimate_host"), sanitize, flags=("-ffp-contract=off",))

    def call(path, mesh, target_faces=None, max_error=None, boundary="quadric", boundary_weight=1.0, min_cos=0.2, eps=1e-3, fixed=None,
             max_rounds=256):
        v = np.ascontiguousarray(mesh["verts"], np.float32)
        f = np.ascontiguousarray(mesh["faces"], np.int32).reshape(-1, 3)
        c = mesh.get("colors")
        fx = np.zeros(len(v), np.uint32) if fixed is None else (np.asarray(fixed).reshape(-1) != 0).astype(np.uint32)
        me2 = 0.0 if max_error is None else np.float64(max_error) * np.float64(max_error)
        head = [len(v), len(f), int(target_faces is not None), int(target_faces or 0), int(max_error is not None), _bits(me2),
                _bits(np.float64(min_cos) * np.float64(min_cos)), _bits(eps), D.BOUNDARY.index(boundary), _bits(boundary_weight),
                max_rounds, int(c is not None)]
        with open(path, "w") as fh:
            fh.write("\n".join([words(head), words(v.view(np.uint32)), words(f), words(fx),
                                words(np.zeros(0) if c is None else np.ascontiguousarray(c, np.float32).view(np.uint32))]) + "\n")
        out = host_program.run(exe, [str(path)], 120, sanitize)
        assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr
        rows = [np.array([int(x) for x in line.split()], np.int64 if i == 2 else np.uint64)       # (the faces may hold -1)
                for i, line in enumerate(out.stdout.split("\n")[:8])]
        return dict(totals=rows[0], log=rows[1].reshape(-1, 4), faces=rows[2].astype(np.int32).reshape(-1, 3),
                    vmap=rows[3].astype(np.int64), out=rows[4].astype(np.uint32).reshape(-1, 3),
                    colors=rows[5].astype(np.uint32).reshape(-1, 3), locked=rows[6], quad0=rows[7].reshape(-1, 11))
    return call


def _compare(got, mesh, **kw):
    ref = D.decimate(mesh, normals=None, **kw)
    st, t = ref["state"], ref["totals"]
    assert (got["quad0"] == st.Q0.view(np.uint64)).all(), "initial quadrics"
    assert got["locked"].tolist() == st.locked.astype(int).tolist()
    assert got["totals"].tolist() == [t[k] for k in D.TOTALS[:8]]
    assert (got["log"] == ref["log"]).all()
    assert (got["faces"] == st.faces.astype(np.int32)).all()
    assert got["vmap"].tolist() == st.vmap.tolist()
    want = st.v32.copy()
    want[st.moved] = st.X[st.moved].astype(np.float32)
    assert (got["out"] == want.view(np.uint32)).all()
    if st.C is not None:
        wc = st.c32.copy()
        wc[st.moved] = st.C[st.moved].astype(np.float32)
        assert (got["colors"] == wc.view(np.uint32)).all()
    return ref


CASES = {
    "tetrahedron": lambda: D.mesh_of(simplify_ref.TET_V, simplify_ref.TET_F),
    "icosphere": lambda: D.mesh_of(*simplify_ref.icosphere(2), colors=True),
    "fan": lambda: D.mesh_of(*S.fan_mesh(40)),
    "grid with a hole": lambda: D.mesh_of(*S.grid_mesh(9, (3, 3, 2), 0.5), colors=True),
    "high indices": lambda: D.mesh_of(S.index_only_mesh(*T.high_index_faces(300)), T.high_index_faces(300)[0]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bodies_equal_the_oracle_bit_for_bit(run, tmp_path, name):
    mesh = CASES[name]()
    fixed = np.random.default_rng(1).random(len(mesh["verts"])) < 0.2
    F = len(mesh["faces"])
    for kw in (dict(target_faces=F // 2), dict(target_faces=F // 8, min_cos=0.0), dict(max_error=0.05),
               dict(target_faces=F // 3, max_error=0.2, boundary="fixed", fixed=fixed), dict(target_faces=F // 2, max_rounds=1),
               dict(max_error=0.02, boundary_weight=10.0, eps=0.0)):
        _compare(run(tmp_path / "case.txt", mesh, **kw), mesh, **kw)


def test_adversarial_lists_and_non_finite_vertices(run, tmp_path):
    for name, (f, V) in clean_ref.adversarial_cases(200).items():
        mesh = D.mesh_of(simplify_ref.adversarial_mesh(f, V), f)
        kw = dict(target_faces=len(f) // 4, min_cos=0.0)
        ref = _compare(run(tmp_path / "case.txt", mesh, **kw), mesh, **kw)
        assert np.isfinite(ref["state"].X[ref["state"].moved]).all(), name
