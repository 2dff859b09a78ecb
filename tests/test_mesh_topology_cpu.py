"""The numpy oracle of header Section 18 (tests/topology_ref.py) pinned on meshes whose answers can be derived by hand, against the
older helpers of tests/mc_ref.py and tests/clean_ref.py, and the argument validation of the four entry points.  No GPU."""
import ctypes

import numpy as np
import pytest

import clean_ref as C
import host_program
import mc_ref
import topology_ref as T


@pytest.fixture(scope="module")
def cases():
    return T.table_cases()


def test_oracle_on_hand_derived_cases(cases):
    assert len(cases) == 9
    for name, (f, V, row) in cases.items():
        assert T.row_of(T.topology(f, V)) == row, name


def test_vertex_rule_joins_the_two_tetrahedra_the_edge_rule_splits():
    f, V = T.two_tets_sharing_vertex()
    assert C.components(f, V)[2] == 1
    label, n = T.face_components(f, V)
    assert n == 2 and label.tolist() == [0] * 4 + [4] * 4
    f, V = T.two_tets_sharing_edge()                     # joined across the non-manifold edge: the departure from trimesh
    assert T.face_components(f, V)[1] == 1
    adj = T.face_adjacency(f, V)
    assert len(adj) == 10 and (adj[:, 0] < adj[:, 1]).all()
    assert not ((adj[:, 0] < 4) & (adj[:, 1] >= 4)).any()          # trimesh's pairs do not cross it


def test_edge_table_of_a_tetrahedron_by_hand():
    f, V = T.tetrahedron()                               # [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]
    t = T.edge_table(f, V)
    assert t["edges"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert t["edge_count"].tolist() == [2] * 6 and t["edge_forward"].tolist() == [1] * 6
    assert t["edge_start"].tolist() == [0, 2, 4, 6, 8, 10, 12]
    assert t["edge_halfedges"].tolist() == [2, 3, 0, 11, 5, 9, 1, 6, 4, 8, 7, 10]
    assert t["face_edges"].tolist() == [[1, 3, 0], [0, 4, 2], [3, 5, 4], [2, 5, 1]]
    assert T.face_adjacency(f, V).tolist() == [[0, 1], [0, 3], [1, 3], [0, 2], [1, 2], [2, 3]]


def test_faces_that_do_not_contribute_and_the_mask():
    f, V = C.adversarial_cases(1000)["invalid, degenerate, trailing"]
    ok = T.contributing(f, V)
    assert ok.tolist() == [True, False, False, False, False, False, False]
    t = T.edge_table(f, V)
    assert (t["n_edges"], t["n_contributing"], t["n_used_verts"], t["n_boundary"], t["n_boundary_loops"]) == (3, 1, 3, 3, 1)
    assert (t["face_edges"][1:] == -1).all()
    f, V = T.tetrahedron()
    t = T.edge_table(f, V, np.array([1, 0, 1, 7], np.uint8))
    assert (t["n_edges"], t["n_contributing"], t["n_boundary"], t["n_boundary_loops"]) == (6, 3, 3, 1)
    assert T.edge_table(np.zeros((0, 3), np.int32), 5)["n_edges"] == 0
    assert T.topology(np.zeros((0, 3), np.int32), 0)["is_watertight"] is False


def test_agrees_with_mc_ref_closed_and_euler(cases):
    for name in ("mc sphere", "mc torus", "mc cut sphere"):
        f, V, _ = cases[name]
        r = T.topology(f, V)
        assert r["is_oriented"] == mc_ref.is_closed(f), name
        assert r["euler"] == mc_ref.euler(f), name
    assert T.topology(*cases["mc sphere"][:2])["is_oriented"] and not T.topology(*cases["mc cut sphere"][:2])["is_oriented"]


def test_edge_components_refine_vertex_components():
    for name, (f, V) in C.adversarial_cases(2000).items():
        _, fl, n_vertex, _ = C.components(f, V)
        label, n_edge = T.face_components(f, V)
        ok = label >= 0
        assert (fl[ok] >= 0).all(), name                 # a contributing face is a valid one
        if ok.any():
            # one vertex component per edge component, so at least as many edge components
            pairs = np.unique(np.stack([label[ok], fl[ok]], 1), axis=0)
            assert len(pairs) == n_edge and n_edge >= len(np.unique(fl[ok])), name


def test_argument_validation_needs_no_gpu():
    """The four Section 18 entry points check their arguments before touching the device (the pointers are never dereferenced)."""
    from nicer_slam_amd._native import lib
    NSA_EBADARG = 4
    fake = ctypes.c_void_p(4096)
    big_f, big_v = (2 ** 31 - 1) // 3 + 1, 1 << 31
    ws = lib.nsa_mesh_edges_workspace
    assert ws(9, 5) > 5 * 4 * 15 and ws(0, 5) > 0 and ws(9, 5) % 256 == 0
    assert ws(9, 0) == 0 and ws(9, big_f) == 0 and ws(big_v, 5) == 0
    assert ws(2 ** 31 - 1, big_f - 1) > 0
    edges = lib.nsa_mesh_edges
    assert edges(None, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0            # F = 0: a no-op
    assert edges(None, 0, 5, None, None, None, None, None, None, None, None, None, None) == 0
    full = [fake, 5, 9, fake, fake, fake, fake, fake, fake, fake, fake, fake, None]
    for k in (0, 4, 5, 6, 7, 8, 9, 10, 11):                                                              # each pointer NULL in turn
        args = list(full)
        args[k] = None
        assert edges(*args) == NSA_EBADARG, k
    for k, val in ((1, big_f), (2, big_v)):
        args = list(full)
        args[k] = val
        assert edges(*args) == NSA_EBADARG, (k, val)
    ws = lib.nsa_mesh_face_components_workspace
    assert ws(5) > 0 and ws(5) % 256 == 0 and ws(0) == 0 and ws(big_f) == 0
    comps = lib.nsa_mesh_face_components
    assert comps(None, None, None, 0, None, None, None, None) == 0                                       # F = 0: a no-op
    full = [fake, fake, fake, 5, fake, fake, fake, None]
    for k in (0, 1, 2, 4, 5, 6):
        args = list(full)
        args[k] = None
        assert comps(*args) == NSA_EBADARG, k
    args = list(full)
    args[3] = big_f
    assert comps(*args) == NSA_EBADARG


def test_python_entry_points_reject_bad_arguments_without_a_gpu():
    import torch
    from nicer_slam_amd import mesh_sdf, mesh_topology
    f = torch.zeros(4, 3, dtype=torch.int32)
    for bad in (lambda: mesh_topology.edge_table(f[:, :2], 4), lambda: mesh_topology.face_components(f.numpy().astype(np.float32), 4),
                lambda: mesh_topology.edge_table(f, -1), lambda: mesh_topology.edge_table(f, 1 << 31),
                lambda: mesh_topology.edge_table(f, 4, face_mask=np.ones(3, np.uint8)),
                lambda: mesh_topology.face_adjacency(f.long() + (1 << 40), 4),
                lambda: mesh_topology.topology({"verts": np.zeros((4, 2), np.float32), "faces": f.numpy()}),
                lambda: mesh_topology.topology({"faces": f.numpy()})):
        with pytest.raises(ValueError):
            bad()
    if not torch.cuda.is_available():                     # no CPU path: a missing GPU is an error that says so
        with pytest.raises(RuntimeError, match="needs a GPU"):
            mesh_topology.edge_table(f, 4)
    assert "auto" in mesh_sdf.SIGNS and mesh_sdf.SIGNS[:2] == ("normal", "winding")
    with pytest.raises(ValueError):
        mesh_sdf.resolve_sign(None, "nearest")
    assert mesh_sdf.resolve_sign(None, "normal") == "normal" and mesh_sdf.resolve_sign(None, "winding") == "winding"
    from nicer_slam_amd import mesh_clean
    with pytest.raises(ValueError):
        mesh_clean.keep_components(dict(verts=np.zeros((3, 3), np.float32), faces=np.zeros((1, 3), np.int32)), connectivity="face")


@pytest.mark.parametrize("sanitize", [False, True])
def test_union_find_passes_on_host_threads(tmp_path, sanitize):
    """The pass bodies the kernels run (csrc/topo_passes.hpp on uf_passes.hpp), compiled as host C++ into a stand-alone program and
    run by 8 threads on a host-built edge table: face labels, boundary marks and loop roots equal a sequential union-find; once more
    under the thread sanitizer where the host compiler has it."""
    sanitize = "thread" if sanitize else None
    exe = host_program.build("topology_host_check.cpp", tmp_path, sanitize, flags=("-pthread",))
    run = host_program.run(exe, ["8", "10000" if sanitize else "50000"], 600, sanitize)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
