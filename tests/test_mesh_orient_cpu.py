"""The numpy oracle of header Section 20 (tests/orient_ref.py) pinned on meshes whose answers can be derived by hand, its volume sums
against exact rationals, the argument validation of the four entry points and of the Python functions, and the pass bodies of
csrc/orient_passes.hpp on host threads.  No GPU."""
import ctypes

import numpy as np
import pytest

import host_program
import orient_ref as O
import topology_ref as T


def flips(f, V):
    return set(np.nonzero(O.orientation(f, V)["flip"])[0].tolist())


@pytest.fixture(scope="module")
def mc():
    return {kind: T.mc_mesh(kind, 16, centre) for kind, centre in (("sphere", (0.0, 0.0, 0.0)), ("torus", (0.0, 0.0, 0.0)))} | \
        {"cut sphere": T.mc_mesh("sphere", 16, (0.7, 0.0, 0.0))}


def test_tetrahedron_rows():
    f, V = T.tetrahedron()
    r = O.orientation(f, V)
    assert flips(f, V) == set() and (r["n_components"], r["n_nonorientable"]) == (1, 0) and r["orient_label"].tolist() == [0] * 4
    assert flips(O.reverse(f, [2]), V) == {2}
    assert flips(T.tetrahedron_one_reversed()[0], V) == {2}                   # reversed the other way round: the same winding
    g = O.reverse(f, [0])
    r = O.orientation(g, V)
    assert set(np.nonzero(r["flip"])[0].tolist()) == {1, 2, 3}                # the smallest face keeps its winding
    vol = O.volume(O.TET_VERTS, g, V, r)
    assert vol["closed"].tolist() == [True] and vol["decided"].tolist() == [True] and vol["toggled"].tolist() == [True]
    assert set(np.nonzero(vol["flip"])[0].tolist()) == {0}                    # outward: the one reversed face is the one to turn
    assert vol["S"][0] == -1.0 / 6.0 and vol["n"].tolist() == [4]
    vol = O.volume(O.TET_VERTS, f, V, O.orientation(f, V))
    assert vol["S"][0] == 1.0 / 6.0 and not vol["toggled"][0] and not vol["flip"].any()


def test_moebius_fan_and_the_two_tetrahedra():
    f, V = T.moebius(8)
    r = O.orientation(f, V)
    assert (r["n_components"], r["n_nonorientable"], r["n_flipped"]) == (1, 1, 0) and not r["orientable"].any()
    assert (r["orient_label"] == 0).all()
    f, V = T.two_tets_sharing_edge()                                          # cut at the non-manifold edge: trimesh's split
    r = O.orientation(f, V)
    assert r["n_components"] == 2 and r["orient_label"].tolist() == [0] * 4 + [4] * 4 and r["orientable"].all()
    v = np.concatenate([O.TET_VERTS, [[0, -1, 0], [0, 0, -1]]]).astype(np.float32)
    vol = O.volume(v, f, V, r)
    assert vol["closed"].tolist() == [False, False] and not vol["decided"].any()          # the strict rule: not closed
    f, V = T.fan(300)
    r = O.orientation(f, V)
    assert r["n_components"] == 300 and r["orient_label"].tolist() == list(range(300)) and r["n_flipped"] == 0
    f, V = O.moebius_beside_tet()
    r = O.orientation(f, V)
    assert (r["n_components"], r["n_nonorientable"]) == (2, 1) and set(np.nonzero(r["flip"])[0].tolist()) == {17}
    assert r["orientable"].tolist() == [False] * 16 + [True] * 4


def test_faces_that_do_not_contribute_and_the_mask():
    import clean_ref as C
    f, V = C.adversarial_cases(1000)["invalid, degenerate, trailing"]
    r = O.orientation(f, V)
    assert r["orient_label"].tolist() == [0] + [-1] * 6 and not r["flip"].any() and r["n_components"] == 1
    f, V = T.tetrahedron()
    g = O.reverse(f, [1])
    r = O.orientation(g, V, np.array([1, 0, 1, 1], np.uint8))
    assert r["orient_label"].tolist() == [0, -1, 0, 0] and not r["flip"].any()
    r = O.orientation(np.zeros((0, 3), np.int32), 5)
    assert r["n_components"] == 0 and len(r["flip"]) == 0


@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_scrambled_marching_cubes_mesh_is_restored_exactly(mc, kind):
    m = mc[kind]
    f, V = m["faces"], len(m["verts"])
    g, which = O.seeded_reversal(f, 0.3, seed=11)
    assert 0.2 < which.mean() < 0.4
    r = O.orientation(g, V)
    vol = O.volume(m["verts"], g, V, r)
    assert r["n_components"] == 1 and vol["closed"].all() and vol["decided"].all()
    assert bool(vol["toggled"][0]) == bool(which[0]) == bool(vol["S"][0] < 0)  # wound like face 0: inward when that was reversed
    assert (vol["flip"] == which).all()
    assert (O.reverse(g, vol["flip"]) == f).all()
    assert T.topology(O.reverse(g, vol["flip"]), V)["is_oriented"]


def test_cut_sphere_is_open_and_undecided_by_volume(mc):
    m = mc["cut sphere"]
    f, V = m["faces"], len(m["verts"])
    g, which = O.seeded_reversal(f, 0.3, seed=12)
    r = O.orientation(g, V)
    vol = O.volume(m["verts"], g, V, r)
    assert r["n_components"] == 1 and r["orientable"].all()
    assert vol["closed"].tolist() == [False] and vol["decided"].tolist() == [False] and (vol["flip"] == r["flip"]).all()
    h = O.reverse(g, r["flip"])                                               # consistent either way: like face 0 of the scrambled mesh
    assert T.edge_table(h, V)["n_inconsistent"] == 0
    assert (h == (f if not which[0] else O.reverse(f, np.ones(len(f), bool)))).all()


def test_view_votes_by_hand():
    f, V = T.tetrahedron()
    d = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0, 1]], np.float32)
    hit = np.array([0, 0, 0, -1])                                             # face 0 = (0, 2, 1): normal -z
    votes = O.view_votes(O.TET_VERTS, f, np.zeros(4, bool), hit, d)
    assert votes.tolist() == [0, 0, 0, 0]                                     # +1 (d = +z), -1 (d = -z), 0 (in the plane)
    votes = O.view_votes(O.TET_VERTS, f, np.zeros(4, bool), hit[:1], d[:1])
    assert votes.tolist() == [1, 0, 0, 0]
    votes = O.view_votes(O.TET_VERTS, f, np.array([True, False, False, False]), hit[:1], d[:1])
    assert votes.tolist() == [-1, 0, 0, 0]
    assert O.component_votes(votes, np.array([0, 0, 0, 0]))[1].tolist() == [-1]


def test_volume_sums_stay_within_the_bound_of_the_exact_rationals(mc):
    """|S_c - exact| <= (n_c + 16) 2^-52 P_c for the oracle on every case: the threshold is a bound, not a tuning"""
    cases = [(O.TET_VERTS, T.tetrahedron()[0]), (O.TET_VERTS, O.reverse(T.TET, [0]))]
    cases += [(m["verts"], O.seeded_reversal(m["faces"], 0.3, seed=11)[0]) for m in mc.values()]
    cases += [(mc["sphere"]["verts"] * np.float32(1e-3) + np.float32(37.25), mc["sphere"]["faces"])]      # far from zero, small
    v, f = O.disjoint_tets(40, seed=3)
    cases.append((v, f))
    n_checked = 0
    for v, f in cases:
        V = len(v)
        r = O.orientation(f, V)
        vol = O.volume(v, f, V, r, exact=True)
        for S, P, n, ex in zip(vol["S"], vol["P"], vol["n"], vol["S_exact"]):
            err = abs(ex - O.Fraction(float(S)))
            assert err <= O.Fraction(float(O.bound(n, P))), (float(err), float(O.bound(n, P)))
            n_checked += 1
    assert n_checked >= 45


def test_argument_validation_needs_no_gpu():
    """The four Section 20 entry points check their arguments before touching the device (the pointers are never dereferenced)."""
    from nicer_slam_amd._native import lib
    NSA_EBADARG = 4
    fake = ctypes.c_void_p(4096)
    big_f, big_v = (2 ** 31 - 1) // 3 + 1, 1 << 31
    ws = lib.nsa_mesh_orient_workspace
    assert ws(5) >= 5 * 8 and ws(5) % 256 == 0 and ws(0) == 0 and ws(big_f) == 0 and ws(big_f - 1) > 0
    orient = lib.nsa_mesh_orient
    assert orient(*([None, 0] + [None] * 10)) == 0                                                      # F = 0: a no-op
    full = [fake, 5, fake, fake, fake, fake, fake, fake, fake, fake, fake, None]
    for k in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10):                                                            # each pointer NULL in turn
        args = list(full)
        args[k] = None
        assert orient(*args) == NSA_EBADARG, k
    args = list(full)
    args[1] = big_f
    assert orient(*args) == NSA_EBADARG
    ws = lib.nsa_mesh_orient_volume_workspace
    assert ws(5) >= 5 * 4 * 5 and ws(5) % 256 == 0 and ws(0) == 0 and ws(big_f) == 0 and ws(big_f - 1) > 0
    volume = lib.nsa_mesh_orient_volume
    assert volume(*([None, 0, None, 0] + [None] * 14)) == 0
    assert volume(*([None, 7, None, 0] + [None] * 14)) == 0
    full = [fake, 9, fake, 5] + [fake] * 13 + [None]
    for k in [0, 2] + list(range(4, 17)):
        args = list(full)
        args[k] = None
        assert volume(*args) == NSA_EBADARG, k
    for k, val in ((1, big_v), (3, big_f)):
        args = list(full)
        args[k] = val
        assert volume(*args) == NSA_EBADARG, (k, val)


def test_python_entry_points_reject_bad_arguments_without_a_gpu():
    import torch
    from nicer_slam_amd import mesh_sdf, mesh_topology
    v, f = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.int32)
    for bad in (lambda: mesh_topology.orient({"verts": v, "faces": f}, outward="inward"),
                lambda: mesh_topology.orient({"verts": v, "faces": f}, outward="views"),
                lambda: mesh_topology.orient({"verts": v, "faces": f}, outward="views", c2w=np.eye(4)),
                lambda: mesh_topology.orient({"faces": f}),
                lambda: mesh_topology.orient({"verts": v[:, :2], "faces": f}),
                lambda: mesh_topology.orientation({"verts": v, "faces": f[:, :2]}),
                lambda: mesh_topology.orientation({"verts": v, "faces": f.astype(np.float32)})):
        with pytest.raises(ValueError):
            bad()
    if not torch.cuda.is_available():                     # no CPU path: a missing GPU is an error that says so
        with pytest.raises(RuntimeError, match="needs a GPU"):
            mesh_topology.orientation({"verts": v, "faces": f})
    assert mesh_topology.OUTWARD == ("volume", "views", None)
    import inspect
    for fn in (mesh_sdf.signed_distance, mesh_sdf.contains, mesh_sdf.mesh_sdf_grid, mesh_sdf.sdf_field_metrics):
        assert inspect.signature(fn).parameters["orient"].default is False
    assert mesh_topology.REPORT_KEYS == ("n_faces", "n_contributing", "n_used_verts", "n_edges", "n_boundary", "n_nonmanifold",
                                         "n_inconsistent", "n_boundary_loops", "n_components", "euler", "is_watertight", "is_oriented")
    with pytest.raises(SystemExit):
        mesh_topology.main(["x.ply", "--orient", "y.ply", "--outward", "views"])


@pytest.mark.parametrize("sanitize", [False, True])
def test_orientation_passes_on_host_threads(tmp_path, sanitize):
    """The pass bodies the kernels run (csrc/orient_passes.hpp on uf_passes.hpp), compiled as host C++ into a stand-alone program and
    run by 8 threads on a host-built edge table: labels, orientability and flips equal a sequential two-colouring; once more under
    the thread sanitizer where the host compiler has it."""
    sanitize = "thread" if sanitize else None
    exe = host_program.build("orient_host_check.cpp", tmp_path, sanitize, flags=("-pthread",))
    run = host_program.run(exe, ["8", "10000" if sanitize else "50000"], 600, sanitize)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
