"""The bodies the hole-filling kernels call (csrc/fill_passes.hpp: the boundary test, the successor by rotation, the pinch mark, the
rounds of pointer jumping and list ranking, the row of a loop, the faces and vertices of the patch), compiled by the host compiler
with -ffp-contract=off into tests/fill_host_check.cpp, run one item at a time and held to tests/fill_ref.py bit for bit; once plain
and once under the address and undefined-behaviour sanitizers where the host compiler has them."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import clean_ref
import fill_ref as R
import simplify_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = "-fsanitize=address,undefined"


@functools.lru_cache(maxsize=None)
def _program(tmp, sanitize):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    assert cxx, "no host C++ compiler (the oracle's Makefile needs one as well)"
    exe = os.path.join(tmp, "fill_host_check" + ("_san" if sanitize else ""))
    cmd = [cxx, "-O1" if sanitize else "-O2", "-g", "-std=c++17", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "fill_host_check.cpp"), "-o", exe]
    if sanitize:
        if subprocess.run(cmd + [SANITIZE, "-fno-sanitize-recover=all"], capture_output=True, text=True).returncode != 0:
            pytest.skip("host compiler without " + SANITIZE)
    else:
        subprocess.run(cmd, check=True)
    return exe


def _bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    exe = _program(str(tmp_path_factory.mktemp("fill_host")), request.param)

    def call(path, mesh, max_edges=None, max_size=None, rings="auto", max_rings=64, skip_folded=True):
        v = np.ascontiguousarray(mesh["verts"], np.float32)
        f = np.ascontiguousarray(mesh["faces"], np.int32).reshape(-1, 3)
        c = mesh.get("colors")
        ms2 = 0.0 if max_size is None else np.float64(max_size) * np.float64(max_size)
        head = [len(v), len(f), int(c is not None), int(max_edges is not None), int(max_edges or 0), int(max_size is not None), _bits(ms2),
                0 if rings == "auto" else int(rings), max_rings, int(skip_folded)]
        words = lambda a: " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))
        with open(path, "w") as fh:
            fh.write("\n".join([words(head), words(v.view(np.uint32)), words(f),
                                words(np.zeros(0) if c is None else np.ascontiguousarray(c, np.float32).view(np.uint32))]) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
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
