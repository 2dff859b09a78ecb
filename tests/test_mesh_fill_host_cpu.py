"""The bodies the hole-filling kernels call (csrc/fill_passes.hpp: the boundary test, the successor by rotation, the pinch mark, the
rounds of pointer jumping and list ranking, the row of a loop, the faces and vertices of the patch), compiled by the host compiler
with -ffp-contract=off into tests/fill_host_check.cpp, run one item at a time and held to tests/fill_ref.py bit for bit; once plain
and once under the address and undefined-behaviour sanitizers where the host compiler has them."""
import numpy as np
import pytest

import clean_ref
import fill_ref as R
import host_program
from host_program import words
import simplify_ref


def _bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("fill_host_check.cpp", tmp_path_factory.mktemp("fill_host"), sanitize, flags=("-ffp-contract=off",))

    def call(path, mesh, max_edges=None, max_size=None, rings="auto", max_rings=64, skip_folded=True):
        v = np.ascontiguousarray(mesh["verts"], np.float32)
        f = np.ascontiguousarray(mesh["faces"], np.int32).reshape(-1, 3)
        c = mesh.get("colors")
        ms2 = 0.0 if max_size is None else np.float64(max_size) * np.float64(max_size)
        head = [len(v), len(f), int(c is not None), int(max_edges is not None), int(max_edges or 0), int(max_size is not None), _bits(ms2),
                0 if rings == "auto" else int(rings), max_rings, int(skip_folded)]
        with open(path, "w") as fh:
            fh.write("\n".join([words(head), words(v.view(np.uint32)), words(f),
                                words(np.zeros(0) if c is None else np.ascontiguousarray(c, np.float32).view(np.uint32))]) + "\n")
        out = host_program.run(exe, [str(path)], 120, sanitize)
        assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr
        rows = [np.array([int(x) for x in line.split()], np.uint64 if i in (0, 8) else np.int64)
                for i, line in enumerate(out.stdout.split("\n")[:12])]
        keys = ("totals", "halfedges", "next", "flags", "leader", "rank", "order", "ints", "reals", "new_verts", "new_colors", "new_faces")
        return dict(zip(keys, rows))
    return call


def compare(got, mesh, **kw):
    """every array of ``got`` (flat integers; floats as their bits) against the oracle"""
    ref = R.fill_holes(mesh, **kw)
    tr, V = ref["trace"], len(mesh["verts"])
    assert [int(x) for x in got["totals"]] == [ref["totals"][k] for k in R.TOTALS]
    assert got["halfedges"].tolist() == tr["halfedges"].tolist()
    assert got["next"].tolist() == tr["next"].tolist()
    assert got["flags"].tolist() == (tr["blocked"] * 1 + tr["pinch"] * 2 + tr["open_chain"] * 4).tolist()
    assert got["leader"].tolist() == tr["leader"].tolist()
    assert got["rank"].tolist() == tr["rank"].tolist()
    assert got["order"].tolist() == tr["order"].tolist()
    assert got["ints"].tolist() == ref["ints"].reshape(-1).tolist()
    assert (got["reals"] == ref["reals"].reshape(-1).view(np.uint64)).all()
    assert (got["new_verts"] == ref["verts"][V:].reshape(-1).view(np.uint32)).all()
    if "colors" in mesh:
        assert (got["new_colors"] == ref["colors"][V:].reshape(-1).view(np.uint32)).all()
    assert got["new_faces"].tolist() == ref["faces"][len(mesh["faces"]):].reshape(-1).tolist()
    return ref


@pytest.mark.parametrize("name", sorted(R.table_cases()))
def test_bodies_equal_the_oracle_bit_for_bit(run, tmp_path, name):
    mesh, kw = R.table_cases()[name]
    compare(run(tmp_path / "case.txt", mesh, **kw), mesh, **kw)


def test_adversarial_lists_and_non_finite_vertices(run, tmp_path):
    for name, (f, V) in clean_ref.adversarial_cases(200).items():
        mesh = R.with_colors(dict(verts=simplify_ref.adversarial_mesh(f, V), faces=np.ascontiguousarray(f, np.int32)))
        for kw in ({}, dict(skip_folded=False, rings=2), dict(max_edges=5, max_size=1.0)):
            compare(run(tmp_path / "case.txt", mesh, **kw), mesh, **kw)
