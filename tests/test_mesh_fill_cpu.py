"""tests/fill_ref.py, the numpy statement of header Section 23, pinned on cases that can be derived by hand -- the rows of
DESIGN 4v's table, each through tests/topology_ref.py -- and on the theorems every fill obeys; then the argument checks of
``mesh_fill.fill_holes``, which run without a GPU.  (The rows with two removed cells of ``grid_mesh(7)`` are the one-ring fills: with
rings="auto" the outer loop of 24 edges takes four rings.)"""
import numpy as np
import pytest

import clean_ref
import decimate_ref as D
import fill_ref as R
import simplify_ref
import smooth_ref as S
import topology_ref as T


def _row(r):
    return T.row_of(T.topology(r["faces"], len(r["verts"])))


def _loops(r):
    return [(int(a[1]), int(a[4]), R.CLASSES[a[3]]) for a in r["ints"]]


@pytest.fixture(scope="module")
def cases():
    return R.table_cases()


@pytest.fixture(scope="module")
def filled(cases):
    return {name: R.fill_holes(mesh, **kw) for name, (mesh, kw) in cases.items()}


def test_cut_sphere(cases, filled):
    mesh = cases["cut sphere"][0]
    one, auto = filled["cut sphere, one ring"], filled["cut sphere"]
    assert _loops(one) == [(32, 1, "filled")] and _row(one) == (550, 277, 825, 0, 0, 0, 2, 1, 0)
    assert _loops(auto) == [(32, 5, "filled")] and auto["verts"].shape == (405, 3) and auto["faces"].shape == (806, 3)
    assert _row(auto)[6] == 2
    vol = S.volume(one["verts"], one["faces"])
    assert vol == S.volume(auto["verts"], auto["faces"]) and abs(vol - 0.74312368) < 1e-8      # the cap lies in the box face x = 1
    x = mesh["verts"][mesh["faces"].reshape(-1)[auto["trace"]["order"]], 0]
    assert (x.view(np.uint32) == x.view(np.uint32)[0]).all()
    assert (auto["verts"][auto["new_vertex"], 0].view(np.uint32) == x.view(np.uint32)[0]).all()
    three = filled["cut sphere, three rings"]
    assert _loops(three) == [(32, 3, "filled")] and len(three["verts"]) == 276 + 65 and len(three["faces"]) == 518 + 160


def test_grid_with_a_hole(filled):
    small, both = filled["grid with a hole, small loops only"], filled["grid with a hole"]
    assert _loops(small) == [(32, 5, "too_many_edges"), (12, 2, "filled")]
    row = _row(small)
    assert row[3] == 32 and row[8] == 1 and row[6] == 1
    assert D.area(small["verts"], small["faces"]) == 64.0 and (small["verts"][:, 2].view(np.uint32) == 0).all()
    assert _loops(both) == [(32, 5, "filled"), (12, 2, "filled")]
    assert both["verts"].shape == (223, 3) and both["faces"].shape == (434, 3) and _row(both)[6] == 2
    assert D.area(both["verts"], both["faces"]) == 128.0
    limited = filled["grid with a hole, size limit"]                                      # the hole's diagonal is sqrt(18), the rim's sqrt(128)
    assert _loops(limited) == [(32, 5, "too_large"), (12, 2, "filled")]


def test_separate_and_touching_holes(filled):
    apart = filled["grid without two cells"]
    assert sorted(n for n, _, _ in _loops(apart)) == [4, 4, 24] and all(c == "filled" for _, _, c in _loops(apart))
    assert apart["verts"].shape == (52, 3) and apart["faces"].shape == (100, 3) and _row(apart)[6] == 2
    for name in ("grid without two touching cells", "grid without two touching cells, other diagonal"):
        r = filled[name]
        assert sorted(_loops(r)) == [(8, 1, "pinched"), (24, 1, "filled")], name
        assert _row(r) == (92, 50, 142, 8, 0, 0, 0, 1, 1), name
        assert r["trace"]["pinch"].sum() == 2 and r["totals"]["n_pinched"] == 1


def test_tetrahedron_and_cylinder(filled):
    tet = filled["open tetrahedron"]
    assert _loops(tet) == [(3, 1, "filled")] and tet["verts"].shape == (5, 3) and tet["faces"].shape == (6, 3) and _row(tet)[6] == 2
    cyl = filled["open cylinder"]
    assert _loops(cyl) == [(12, 2, "filled")] * 2 and cyl["verts"].shape == (86, 3) and cyl["faces"].shape == (168, 3)
    assert _row(cyl)[6] == 2 and T.topology(cyl["faces"], 86)["is_oriented"]
    prism = 0.5 * 12 * np.sin(2 * np.pi / 12) * 4
    assert abs(S.volume(cyl["verts"], cyl["faces"]) / prism - 1.0) < 1e-6


def test_open_chains_and_folded_loops(cases, filled):
    for name, n_open in (("moebius strip", 16), ("fan", 600)):
        r, mesh = filled[name], cases[name][0]
        assert len(r["ints"]) == 0 and r["totals"]["n_open_chain"] == n_open == r["totals"]["n_boundary"]
        assert r["verts"].tobytes() == mesh["verts"].tobytes() and np.array_equal(r["faces"], mesh["faces"])
    r = filled["strip"]
    assert _loops(r) == [(52, 1, "folded")] and len(r["faces"]) == 50 and r["totals"]["n_folded"] == 1
    r = filled["strip, folded kept"]
    assert _loops(r) == [(52, 1, "filled")] and _row(r)[6] == 2


def test_theorems(cases, filled):
    for name, (mesh, kw) in cases.items():
        r, tr = filled[name], filled[name]["trace"]
        V, F = len(mesh["verts"]), len(mesh["faces"])
        before, after = T.topology(mesh["faces"], V), T.topology(r["faces"], len(r["verts"]))
        n_filled = r["totals"]["n_filled"]
        assert r["verts"][:V].tobytes() == np.ascontiguousarray(mesh["verts"], np.float32).tobytes(), name
        assert r["faces"][:F].tobytes() == np.ascontiguousarray(mesh["faces"], np.int32).tobytes(), name
        assert r["totals"]["n_new_verts"] == len(r["verts"]) - V and r["totals"]["n_new_faces"] == len(r["faces"]) - F
        assert sum(r["totals"]["n_" + c] for c in R.CLASSES) == r["totals"]["n_loops"]
        if tr["pinch"].any() or tr["blocked"].any():
            continue
        assert len(tr["loop_n"]) == before["n_boundary_loops"], name
        assert after["euler"] == before["euler"] + n_filled and after["n_boundary_loops"] == before["n_boundary_loops"] - n_filled, name
        assert after["n_components"] == before["n_components"], name
        assert after["n_inconsistent"] == 0 or before["n_inconsistent"] != 0, name
        again = R.fill_holes(dict(verts=r["verts"], faces=r["faces"]), **kw)
        if after["n_boundary"] == 0:
            assert again["totals"]["n_new_faces"] == 0 and len(again["faces"]) == len(r["faces"]), name


def test_order_follows_the_boundary(cases, filled):
    """every loop is a closed walk along boundary half-edges: the end of each is the start of the next"""
    for name, (mesh, _) in cases.items():
        tr, f = filled[name]["trace"], np.asarray(mesh["faces"], np.int64)
        for s, n in zip(tr["loop_start"], tr["loop_n"]):
            h = tr["order"][s:s + n]
            assert h[0] == h.min() and np.array_equal(f[h // 3, (h % 3 + 1) % 3], np.roll(f.reshape(-1)[h], -1)), name
        assert len(tr["order"]) + tr["open_chain"].sum() == len(tr["halfedges"])
        assert np.array_equal(np.sort(tr["order"]), tr["halfedges"][~tr["open_chain"]])


def test_a_nan_on_a_loop(cases):
    mesh = dict(cases["grid with a hole"][0])
    v = mesh["verts"].copy()
    v[3 * 9 + 3, 1] = np.nan                                                              # a corner of the hole
    r = R.fill_holes(dict(mesh, verts=v))
    assert _loops(r) == [(32, 5, "filled"), (12, 0, "nonfinite")] and (r["reals"][1] == 0).all()
    assert r["totals"]["n_nonfinite"] == 1 and len(r["verts"]) == 81 + 129


def test_colours_are_interpolated(filled):
    r = filled["open cylinder"]
    ints, reals, V = r["ints"], r["reals"], 60
    for l in range(2):
        n, vo = int(ints[l, 1]), int(ints[l, 7])
        ring0 = r["faces"].reshape(-1)[r["trace"]["order"][int(ints[l, 2]):][:n]]
        mean = r["colors"][ring0].astype(np.float64).mean(0)
        assert np.abs(reals[l, 3:6] - mean).max() < 1e-15
        assert np.array_equal(r["colors"][V + vo + n], reals[l, 3:6].astype(np.float32))                       # the centre
        half = (reals[l, 3:6][None] + 0.5 * (r["colors"][ring0].astype(np.float64) - reals[l, 3:6][None])).astype(np.float32)
        assert np.array_equal(r["colors"][V + vo:V + vo + n], half)                                             # K = 2: t_1 = 1 / 2


def test_fairing_is_smoothing_with_the_old_vertices_fixed(filled):
    """what ``fill_holes(fair=5)`` composes: five Laplacian steps of header Section 21 on the filled mesh, old vertices held"""
    r = filled["cut sphere"]
    fixed = ~r["new_vertex"]
    out, _ = S.smooth_steps(r["verts"], r["faces"], S.factors_of("laplacian", 5, 0.5), fixed=fixed)
    assert out[fixed].tobytes() == r["verts"][fixed].tobytes() and (out[~fixed] != r["verts"][~fixed]).any()
    assert (out[~fixed, 0].view(np.uint32) == r["verts"][~fixed, 0].view(np.uint32)).all()    # the cap stays in its plane, bit for bit
    assert T.topology(r["faces"], len(out))["is_oriented"]


def test_adversarial_lists(filled):
    seen = set()
    for name, (f, V) in clean_ref.adversarial_cases(200).items():
        mesh = dict(verts=simplify_ref.adversarial_mesh(f, V), faces=np.ascontiguousarray(f, np.int32))
        r = R.fill_holes(mesh, skip_folded=False)
        seen.update(c for _, _, c in _loops(r))
        assert r["totals"]["status"] == 0 and r["faces"][:len(f)].tobytes() == mesh["faces"].tobytes(), name
        new = r["faces"][len(f):]
        assert ((new >= 0) & (new < len(r["verts"]))).all(), name
    assert "filled" in seen


def test_argument_checks_need_no_gpu():
    from nicer_slam_amd import mesh_fill as M
    mesh = dict(verts=simplify_ref.TET_V, faces=simplify_ref.TET_F[:3])
    for kw in (dict(max_edges=-1), dict(max_edges=2.5), dict(max_size=-1.0), dict(max_size=float("nan")), dict(rings=0), dict(rings="many"),
               dict(rings=1 << 16), dict(max_rings=0), dict(fair=-1), dict(lam=0.0), dict(normals="flat")):
        with pytest.raises(ValueError):
            M.fill_holes(mesh, **kw)
    with pytest.raises(ValueError):
        M.fill_holes(dict(verts=simplify_ref.TET_V))
    with pytest.raises(ValueError):
        M.fill_holes(dict(verts=simplify_ref.TET_V, faces=np.zeros((2, 4), np.int32)))
    with pytest.raises(SystemExit):
        M.main(["in.ply"])
    assert M.CLASSES == R.CLASSES and M.TOTALS == R.TOTALS and M.INT_COLS == R.INT_COLS


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes
    from nicer_slam_amd._native import lib
    EBADARG = 4
    fake = ctypes.c_void_p(256)
    big_f = (2 ** 31 - 1) // 3 + 1
    assert lib.nsa_mesh_fill_workspace(0, 3) == 0 and lib.nsa_mesh_fill_workspace(4, 0) == 0 and lib.nsa_mesh_fill_workspace(big_f, 3) == 0
    assert lib.nsa_mesh_fill_workspace(4, 13) == 0                                     # more boundary half-edges than half-edges
    assert lib.nsa_mesh_fill_workspace(1000, 300) >= 4 * 3000 + 13 * 4 * 300 + 4 * 300
    loops = lambda *a: lib.nsa_mesh_fill_loops(*a)
    ok = [fake, None, 4, fake, None, 4, fake, fake, fake, fake, fake, fake, 3, 0, 0, 0, 0.0, 0, 64, 1] + [fake] * 10 + [None]
    for i in (0, 3, 6, 7, 8, 9, 10, 11) + tuple(range(20, 30)):                         # every required pointer in turn
        a = list(ok)
        a[i] = None
        assert loops(*a) == EBADARG, i
    for i, x in ((2, 2 ** 31), (5, big_f), (12, 13), (17, 65536), (18, 0), (18, 65536)):
        a = list(ok)
        a[i] = x
        assert loops(*a) == EBADARG, (i, x)
    for ms2 in (-1.0, float("nan")):
        a = list(ok)
        a[15], a[16] = 1, ms2
        assert loops(*a) == EBADARG
    nothing = [None, None, 4, None, None, 4, None, None, None, None, None, None, 0, 0, 0, 0, 0.0, 0, 64, 1] + [None] * 11
    assert loops(*nothing) == 0                                                        # B = 0: nothing to do
    nothing[5] = 0
    assert loops(*nothing) == 0                                                        # F = 0
    emit = lambda *a: lib.nsa_mesh_fill_emit(*a)
    ok = [fake, None, 4, fake, 4, fake, 3, fake, fake, fake, 1, 3, fake, None, fake, None]
    for i in (0, 3, 5, 7, 8, 9, 12, 14):
        a = list(ok)
        a[i] = None
        assert emit(*a) == EBADARG, i
    for i, x in ((2, 2 ** 31), (4, big_f), (6, 13), (10, 2 ** 31), (11, 2 ** 31)):
        a = list(ok)
        a[i] = x
        assert emit(*a) == EBADARG, (i, x)
    a = list(ok)
    a[1] = fake                                                                        # colours in without colours out
    assert emit(*a) == EBADARG
    a = list(ok)
    a[11] = 0
    a[12] = a[14] = None
    assert emit(*a) == 0                                                               # no new face: nothing to do
