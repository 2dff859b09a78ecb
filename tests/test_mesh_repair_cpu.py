"""The sequential oracle of header Section 26 (tests/manifold_ref.py) pinned on the hand rows of DESIGN 4y, on the properties the
statement claims over random face soups and on the clustered torus, plus the argument validation of the entry points.  No GPU."""
import ctypes

import numpy as np
import pytest

import clean_ref as C
import manifold_ref as M
import topology_ref as T


def test_hand_rows():
    for name, (f, V, want, src) in M.hand_rows().items():
        r = M.split_fans(f, V)
        assert r["faces"].tolist() == want, name
        assert r["new_source"].tolist() == src and r["n_new"] == len(src), name
    r = M.split_fans(*M.bow_tie())
    assert M.totals_of(r) == [2, 6, 1, 1, 0, 1, 2, 0]                    # a pinch only: no cut edge
    assert r["corner_fan"].tolist() == [0, 1, 2, 3, 4, 5] and r["vertex_fans"].tolist() == [2, 1, 1, 1, 1]
    r = M.split_fans(*M.book())
    assert M.totals_of(r) == [3, 9, 2, 0, 1, 4, 3, 0]
    assert r["vertex_fans"].tolist() == [3, 3, 1, 1, 1]


def test_two_tetrahedra_on_one_edge_become_two_closed_tetrahedra():
    f, V = T.two_tets_sharing_edge()
    r = M.split_fans(f, V)
    assert r["n_new"] == 2 and r["new_source"].tolist() == [0, 1] and r["n_cut_edges"] == 1 and r["n_pinch_only"] == 0
    assert r["faces"][:4].tolist() == f[:4].tolist()                     # the first fans keep their names
    rep = T.topology(r["faces"], V + 2)
    assert rep["is_oriented"] and rep["n_components"] == 2 and rep["euler"] == 4
    assert C.components(r["faces"], V + 2)[2] == 2
    f, V = T.two_tets_sharing_vertex()
    r = M.split_fans(f, V)
    assert M.totals_of(r) == [8, 8, 1, 1, 0, 1, 2, 0] and r["new_source"].tolist() == [3]
    assert C.components(r["faces"], V + 1)[2] == 2


def test_manifold_meshes_are_unchanged():
    for f, V in (T.tetrahedron(), T.moebius(8), T.strip(500)):
        r = M.split_fans(f, V)
        assert r["n_new"] == 0 and r["n_cut_edges"] == 0 and r["max_fans"] == 1 and (r["faces"] == f).all()
    f, V = T.moebius(8)                                                   # its one inconsistent edge is cut on request
    r = M.split_fans(f, V, cut_inconsistent=True)
    assert r["n_cut_edges"] == 1 and r["n_new"] == 2 and T.topology(r["faces"], V + 2)["n_inconsistent"] == 0
    f, V = T.fan(300)
    r = M.split_fans(f, V)
    assert M.totals_of(r) == [300, 900, 2, 0, 1, 598, 300, 0]
    f, V = M.vertex_star(300)
    assert M.totals_of(M.split_fans(f, V)) == [300, 900, 1, 1, 0, 299, 300, 0]


def test_labels_cut_the_seams_between_patches_and_the_mask_removes_faces():
    f, V = T.tetrahedron()
    r = M.split_fans(f, V, labels=np.array([0, 0, 1, 1]))
    assert r["n_cut_edges"] == 4 and r["n_new"] == 4 and r["vertex_fans"].tolist() == [2, 2, 2, 2]
    rep = T.topology(r["faces"], V + 4)
    assert rep["n_components"] == 2 and rep["n_boundary"] == 8 and rep["n_nonmanifold"] == 0
    f, V = M.book()
    r = M.split_fans(f, V, face_mask=np.array([1, 1, 0], np.uint8))
    assert r["n_new"] == 0 and r["corner_fan"].tolist() == [0, 1, 2, 1, 0, 5, -1, -1, -1] and (r["faces"] == f).all()
    r = M.split_fans(np.array([[0, 1, 2], [7, 1, 9], [-1, 5, 2]]), 5)     # a face that does not contribute reaches no new vertex
    assert r["faces"].tolist() == [[0, 1, 2], [-1, 1, -1], [-1, -1, 2]] and r["n_contributing"] == 1
    assert M.totals_of(M.split_fans(np.zeros((0, 3), np.int32), 4)) == [0] * 8


def _check_properties(f, V, **kw):
    r = M.split_fans(f, V, **kw)
    F, n = len(f), r["n_new"]
    ok = r["corner_fan"].reshape(-1, 3)[:, 0] >= 0
    out = r["faces"]
    # old vertices and every face index keep their place; the sources map back
    source = np.concatenate([np.arange(V), r["new_source"]])
    assert len(out) == F and out.min(initial=0) >= -1 and out.max(initial=-1) < V + n
    assert (source[out[ok]] == np.asarray(f, np.int64)[ok]).all()
    assert (out[~ok] == np.where(np.asarray(f, np.int64)[~ok] >= V, -1, f[~ok])).all()
    assert r["n_fans"] == int((r["vertex_fans"] > 0).sum()) + n and r["vertex_fans"].sum() == r["n_fans"]
    # a fan holds at most two faces on any input edge
    t = T.edge_table(f, V, kw.get("face_mask"))
    flat = np.asarray(f, np.int64).reshape(-1)
    for e in range(t["n_edges"]):
        he = t["edge_halfedges"][t["edge_start"][e]:t["edge_start"][e + 1]]
        for v in t["edges"][e]:
            fans = [r["corner_fan"][h if flat[h] == v else 3 * (h // 3) + (h % 3 + 1) % 3] for h in he]
            assert max(np.bincount(np.unique(fans, return_inverse=True)[1])) <= 2
    # no edge above two faces, one fan per vertex, idempotent
    mask = kw.get("face_mask")
    t2 = T.edge_table(out, V + n, mask)
    assert t2["n_nonmanifold"] == 0 and t2["n_contributing"] == r["n_contributing"]
    again = M.split_fans(out, V + n, **kw)
    assert again["n_new"] == 0 and again["max_fans"] <= 1 and again["n_cut_edges"] == 0 and (again["faces"] == out).all()
    assert again["n_fans"] == r["n_fans"]
    return r


def test_properties_on_random_soups():
    rng = np.random.default_rng(2024)
    new = 0
    for i in range(1200):
        f, V = M.random_soup(rng)
        kw = {}
        if i % 4 == 1:
            kw["cut_inconsistent"] = True
        if i % 4 == 2:
            kw["labels"] = rng.integers(0, 3, len(f))
        if i % 4 == 3:
            kw["face_mask"] = rng.integers(0, 2, len(f)).astype(np.uint8)
        new += _check_properties(f, V, **kw)["n_new"]
    assert new > 1200                                                     # the soups are not manifold: the properties were exercised


def test_clustered_torus_and_the_concatenated_soups():
    m = T.mc_mesh("torus", 16)
    assert len(m["faces"]) == 896 and T.topology(m["faces"], len(m["verts"]))["is_watertight"]
    f, V = M.clustered_torus(16, 0.45)
    assert len(f) == 66 and T.topology(f, V)["n_nonmanifold"] == 17
    r = _check_properties(f, V)
    assert T.topology(r["faces"], V + r["n_new"])["n_nonmanifold"] == 0 and r["n_cut_edges"] == 17
    f24, V24 = M.clustered_torus(24, 0.45)
    assert T.topology(f24, V24)["n_nonmanifold"] == 5
    f, V = M.concatenated_soups(60, seed=5)
    r = _check_properties(f, V)
    label, n = M.fan_components(f, V)
    assert (label >= 0).sum() == r["n_contributing"]
    assert C.components(r["faces"][label >= 0], V + r["n_new"])[2] == n  # (clean_ref joins degenerate faces too: leave them out)


def test_weld_oracle_undoes_the_split():
    f, V = T.two_tets_sharing_edge()
    r = M.split_fans(f, V)
    names = np.concatenate([np.arange(V), r["new_source"]])               # a new vertex has the coordinates of its source
    g, rep, dropped = M.weld(r["faces"], names, V + r["n_new"])
    assert (g == f).all() and rep.tolist() == list(range(V)) and dropped == 0
    g, rep, dropped = M.weld(np.array([[0, 1, 2], [2, 3, 4], [1, 3, 9]]), np.array([0, 1, 2, 1, 4]), 5)
    assert g.tolist() == [[0, 1, 2], [2, 1, 3]] and rep.tolist() == [0, 1, 2, 4] and dropped == 1


def test_argument_validation_needs_no_gpu():
    """Section 26's entry points check their arguments before touching the device (the pointers are never dereferenced)."""
    from nicer_slam_amd._native import lib
    NSA_EBADARG = 4
    fake = ctypes.c_void_p(4096)
    big_f = (2 ** 31 - 1) // 3 + 1
    ws = lib.nsa_mesh_split_fans_workspace
    assert ws(9, 5) > 0 and ws(9, 5) % 256 == 0 and ws(0, 5) > 0
    assert ws(9, 0) == 0 and ws(9, big_f) == 0 and ws(1 << 31, 5) == 0 and ws(2 ** 31 - 15, 5) == 0 and ws(2 ** 31 - 17, 5) > 0
    split = lib.nsa_mesh_split_fans
    n_args = len(split.argtypes)
    assert split(*([None, 0, 7, None, 0] + [None] * (n_args - 5))) == 0                                  # F = 0: a no-op
    full = [fake, 5, 9, None, 0] + [fake] * 13 + [None]
    assert len(full) == n_args
    for k in (0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17):                                           # each pointer NULL in turn
        args = list(full)
        args[k] = None
        assert split(*args) == NSA_EBADARG, k
    for k, val in ((1, big_f), (2, 1 << 31), (2, 2 ** 31 - 15), (4, 8)):                                   # counts, V + 3 F, flags
        args = list(full)
        args[k] = val
        assert split(*args) == NSA_EBADARG, (k, val)


def test_python_entry_points_reject_bad_arguments_without_a_gpu():
    import torch
    from nicer_slam_amd import mesh_repair, mesh_simplify
    v, f = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    for bad in (lambda: mesh_repair.split_nonmanifold({"faces": f}),
                lambda: mesh_repair.split_nonmanifold({"verts": v[:, :2], "faces": f}),
                lambda: mesh_repair.split_nonmanifold({"verts": v, "faces": f}, labels=np.zeros(3, np.int32)),
                lambda: mesh_repair.split_nonmanifold({"verts": v, "faces": f}, labels=np.zeros(2, np.float32)),
                lambda: mesh_repair.split_nonmanifold({"verts": v, "faces": f, "normals": v[:3]}),
                lambda: mesh_repair.vertex_fans({"verts": v, "faces": f.astype(np.float32)}),
                lambda: mesh_repair.weld({"verts": v}),
                lambda: mesh_simplify.simplify({"verts": v, "faces": f}, cell=1.0, split=3)):
        with pytest.raises(ValueError):
            bad()
    if not torch.cuda.is_available():                     # no CPU path: a missing GPU is an error that says so
        with pytest.raises(RuntimeError, match="needs a GPU"):
            mesh_repair.split_nonmanifold({"verts": v, "faces": f})
