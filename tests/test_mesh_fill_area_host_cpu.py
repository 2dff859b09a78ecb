"""The bodies the minimum-area kernels call (csrc/fill_area_passes.hpp: the plan row, the row of a loop vertex, the chord mask, the
cell minimum as one lane and as 64 striding lanes merged along the xor butterfly, the final class, a face by descent), compiled by the
host compiler with -ffp-contract=off into tests/fill_area_host_check.cpp, run one item at a time and held to tests/fill_area_ref.py
bit for bit; once plain and once under the address and undefined-behaviour sanitizers where the host compiler has them."""
import numpy as np
import pytest

import clean_ref
import fill_area_ref as A
import fill_ref as R
import host_program
from host_program import words
import simplify_ref
import topology_ref as T


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def run(request, tmp_path_factory):
    sanitize = "address,undefined" if request.param else None
    exe = host_program.build("fill_area_host_check.cpp", tmp_path_factory.mktemp("fill_area_host"), sanitize, flags=("-ffp-contract=off",))

    def call(path, mesh, method, max_area_edges=2048, min_sin=1e-6, **kw):
        """the program on the loops of the oracle; compares everything it prints with the oracle"""
        ref = A.fill_holes(mesh, method=method, max_area_edges=max_area_edges, min_sin=min_sin, **kw)
        v = np.ascontiguousarray(mesh["verts"], np.float32)
        f = np.ascontiguousarray(mesh["faces"], np.int32).reshape(-1, 3)
        tr, p = ref["trace"], ref["patches"]
        B, L = len(tr["halfedges"]), len(ref["ints"])
        edges = T.edge_table(f, len(v))["edges"]
        order = np.full(B, -1, np.int64)
        order[:len(tr["order"])] = tr["order"]
        ms2 = np.float64(min_sin) * np.float64(min_sin)
        mask = 1 << R.FOLDED if method == "auto" else 1 << R.FILLED | 1 << R.FOLDED
        head = [len(v), len(f), B, L, len(edges), mask, max_area_edges, int(np.array([ms2]).view(np.uint64)[0]), 0]
        with open(path, "w") as fh:
            fh.write("\n".join([words(head), words(v.view(np.uint32)), words(f), words(edges), words(order), words(ref["ints"])]) + "\n")
        out = host_program.run(exe, [str(path)], 300, sanitize)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
        rows = [np.array([int(x) for x in line.split()], np.uint64 if i in (3, 5) else np.int64)
                for i, line in enumerate(out.stdout.split("\n")[:8])]
        got = dict(zip(("plan", "final", "ints", "area", "mask", "W", "J", "faces"), rows))
        t = ref["area_totals"]
        n_tabled = len(ref["tables"])
        assert got["plan"].tolist() == [t["n_selected"], n_tabled, t["n_area_too_many_edges"], t["n_cells"], t["max_n"],
                                        len(p["plan_faces"]), p["n_rows"], 0]
        assert got["final"].tolist() == [t["n_area_filled"], t["n_area_too_many_edges"], t["n_no_triangulation"], t["n_area_faces"]]
        assert got["ints"].tolist() == ref["area_ints"].reshape(-1).tolist()
        assert (got["area"] == ref["area"].view(np.uint64)).all()
        assert got["mask"].tolist() == p["mask"].astype(np.int64).tolist()
        assert (got["W"] == p["W"].view(np.uint64)).all()
        assert got["J"].tolist() == p["J"].tolist()
        assert got["faces"].tolist() == p["plan_faces"].reshape(-1).tolist()
        return ref
    return call


@pytest.mark.parametrize("method", ["auto", "min_area"])
@pytest.mark.parametrize("name", sorted(A.small_cases()))
def test_small_loops_and_refusals(run, tmp_path, name, method):
    mesh, kw = A.small_cases()[name]
    run(tmp_path / "case.txt", mesh, method, **kw)


@pytest.mark.parametrize("name", sorted(A.collar_cases()))
def test_collars(run, tmp_path, name):
    mesh, kw, _ = A.collar_cases()[name]
    ref = run(tmp_path / "case.txt", mesh, "min_area", **kw)
    assert ref["area_totals"]["n_area_filled"] == 1


def test_over_the_cap_and_many_loops(run, tmp_path):
    mesh, kw, _ = A.collar_cases()["comb 66"]
    ref = run(tmp_path / "case.txt", mesh, "min_area", max_area_edges=65, **kw)
    assert ref["area_totals"]["n_area_too_many_edges"] == 1 and ref["area_totals"]["n_cells"] == 0
    ref = run(tmp_path / "case.txt", A.grid65(), "min_area", max_edges=4)
    assert ref["area_totals"]["n_area_filled"] == 256 and ref["area_totals"]["n_cells"] == 4096


def test_adversarial_lists_and_non_finite_vertices(run, tmp_path):
    for name, (f, V) in clean_ref.adversarial_cases(200).items():
        mesh = dict(verts=simplify_ref.adversarial_mesh(f, V), faces=np.ascontiguousarray(f, np.int32))
        for method, kw in (("auto", {}), ("min_area", dict(skip_folded=False)), ("min_area", dict(max_edges=40, min_sin=0.0))):
            run(tmp_path / "case.txt", mesh, method, **kw)
