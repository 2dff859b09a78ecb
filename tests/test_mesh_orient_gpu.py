"""Mesh orientation on the device (header Section 20, csrc/mesh_orient.hip) against the sequential oracle of
tests/orient_ref.py: every per-face array and every total element for element, the volume sums within their float64 bound of the
fsum oracle, a second run bit-identical; then the public interface on the device's own marching cubes, the views rule against the
oracle's count from the device's own hits, mesh_sdf's orient=True and the command line."""
import json

import numpy as np
import pytest
import torch

import clean_ref as C
import orient_ref as O
import topology_ref as T

pytestmark = pytest.mark.gpu


def _run(faces, V, verts=None, mask=None):
    from nicer_slam_amd import mesh_topology as M
    f, V, F, m, _ = M._checked(faces, V, mask, "test")
    t, _ = M._edge_table(f, V, F, m)
    label, orientable, flip, totals = M._orientation(f, t, F)
    out = dict(orient_label=label.cpu().numpy(), orientable=orientable.cpu().numpy() != 0, flip=flip.cpu().numpy() != 0, **totals)
    if verts is not None:
        flip_out, vol = M._orient_volume(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).cuda(), f, V, F, t, label, orientable, flip)
        comp = np.nonzero(out["orient_label"] == np.arange(F))[0]
        out["vol"] = dict(flip=flip_out.cpu().numpy() != 0, label=comp, S=vol["S"].cpu().numpy()[comp], P=vol["P"].cpu().numpy()[comp],
                          n=vol["n"].cpu().numpy()[comp], flags=vol["flags"].cpu().numpy()[comp], origin=vol["origin"].cpu().numpy(),
                          totals=tuple(vol[k] for k in ("n_closed", "n_decided", "n_toggled", "n_flipped")))
    return out


def _same(a, b):
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k                       # bit for bit, NaN or not
        else:
            assert a[k] == b[k], k


def _check(faces, V, verts=None, mask=None, ref=None):
    """the device against the oracle (on ``ref`` = (faces, V, verts, face map) when the oracle runs on another list); twice"""
    got = _run(faces, V, verts, mask)
    _same(got, _run(faces, V, verts, mask))
    rf, rV, rv, fmap = ref if ref is not None else (faces, V, verts, None)
    r = O.orientation(rf, rV)
    F = len(np.asarray(faces).reshape(-1, 3))
    exp = {k: r[k] for k in ("orient_label", "orientable", "flip")}
    if fmap is not None:                                                    # oracle faces -> faces of the full list
        full = dict(orient_label=np.full(F, -1, np.int64), orientable=np.zeros(F, bool), flip=np.zeros(F, bool))
        full["orient_label"][fmap] = fmap[r["orient_label"]]
        full["orientable"][fmap], full["flip"][fmap] = r["orientable"], r["flip"]
        exp = full
    for k in exp:
        assert (got[k] == exp[k]).all(), k
    assert (got["n_components"], got["n_nonorientable"], got["n_flipped"]) == (r["n_components"], r["n_nonorientable"], r["n_flipped"])
    if verts is not None:
        vol, g = O.volume(rv, rf, rV, r), got["vol"]
        assert (g["origin"] == vol["origin"]).all()
        assert (g["label"] == (vol["label"] if fmap is None else fmap[vol["label"]])).all() and (g["n"] == vol["n"]).all()
        assert (((g["flags"] & 1) != 0) == vol["closed"]).all()
        b = O.bound(vol["n"], vol["P"])
        assert (np.abs(g["S"] - vol["S"]) <= b).all() and (np.abs(g["P"] - vol["P"]) <= b).all()
        assert (((g["flags"] & 2) != 0) == vol["decided"]).all() and (((g["flags"] & 4) != 0) == vol["toggled"]).all()
        ef = vol["flip"]
        if fmap is not None:
            ef = np.zeros(F, bool)
            ef[fmap] = vol["flip"]
        assert (g["flip"] == ef).all()
        assert g["totals"] == (int(vol["closed"].sum()), int(vol["decided"].sum()), int(vol["toggled"].sum()), int(ef.sum()))
    return got


def _random_verts(V, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (V, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def mc():
    return {"sphere": T.mc_mesh("sphere", 16), "torus": T.mc_mesh("torus", 16), "cut sphere": T.mc_mesh("sphere", 16, (0.7, 0.0, 0.0))}


def test_hand_derived_rows(mc):
    f, V = T.tetrahedron()
    for g in (f, O.reverse(f, [2]), O.reverse(f, [0]), T.tetrahedron_one_reversed()[0]):
        _check(g, V, O.TET_VERTS)
    got = _check(O.reverse(f, [0]), V, O.TET_VERTS)
    assert np.nonzero(got["flip"])[0].tolist() == [1, 2, 3] and np.nonzero(got["vol"]["flip"])[0].tolist() == [0]
    f, V = T.moebius(8)
    got = _check(f, V, _random_verts(V))
    assert (got["n_components"], got["n_nonorientable"], got["n_flipped"]) == (1, 1, 0)
    f, V = T.two_tets_sharing_edge()
    got = _check(f, V, np.concatenate([O.TET_VERTS, [[0, -1, 0], [0, 0, -1]]]).astype(np.float32))
    assert got["n_components"] == 2 and got["vol"]["totals"][0] == 0                 # neither is closed
    f, V = T.fan(300)
    assert _check(f, V, _random_verts(V))["n_components"] == 300
    f, V = O.moebius_beside_tet()
    got = _check(f, V, _random_verts(V))
    assert (got["n_components"], got["n_nonorientable"]) == (2, 1) and np.nonzero(got["vol"]["flip"])[0].tolist() in ([17], [16, 18, 19])
    for kind in ("sphere", "torus"):
        m = mc[kind]
        g, which = O.seeded_reversal(m["faces"], 0.3, seed=11)
        got = _check(g, len(m["verts"]), m["verts"])
        assert (got["vol"]["flip"] == which).all()                                     # restored exactly
    m = mc["cut sphere"]
    g, _ = O.seeded_reversal(m["faces"], 0.3, seed=12)
    got = _check(g, len(m["verts"]), m["verts"])
    assert got["vol"]["totals"][:3] == (0, 0, 0) and (got["vol"]["flip"] == got["flip"]).all()      # open: undecided


def test_no_faces_and_a_single_face():
    from nicer_slam_amd import mesh_topology as M
    got = _check(np.zeros((0, 3), np.int32), 5, _random_verts(5))
    assert got["n_components"] == 0 and got["vol"]["totals"] == (0, 0, 0, 0)
    got = _check(np.array([[2, 0, 1]], np.int32), 3, _random_verts(3))
    assert got["orient_label"].tolist() == [0] and got["n_components"] == 1 and not got["flip"].any()
    _check(np.array([[2, 0, 1]], np.int32), 0)                                         # no vertex: nothing contributes
    mesh = {"verts": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32)}
    out, rep = M.orient(mesh, return_report=True)
    assert out["faces"].shape == (0, 3) and rep["n_components"] == 0 and rep["n_undecided"] == 0
    label, orientable, flip, rep = M.orientation(mesh)
    assert label.shape == (0,) and rep["is_orientable"] and rep["component_faces"].shape == (0,)


def test_face_mask_against_the_compacted_list(mc):
    m = mc["sphere"]
    g, _ = O.seeded_reversal(m["faces"], 0.3, seed=4)
    mask = np.random.default_rng(8).random(len(g)) < 0.8
    keep = np.nonzero(mask)[0]
    _check(g, len(m["verts"]), m["verts"], mask.astype(np.uint8), ref=(g[keep], len(m["verts"]), m["verts"], keep))


def test_adversarial_face_lists():
    for name, (f, V) in C.adversarial_cases(2000).items():
        g = O.reverse(f, np.arange(len(f)) % 3 == 1)
        _check(g, V, _random_verts(V, 2) if V else None)


def test_highest_indices_of_a_wide_key():
    f, V = T.high_index_faces((1 << 16) + 3)
    v = np.zeros((V, 3), np.float32)
    v[V - 4:] = O.TET_VERTS
    got = _check(O.reverse(f, [0, 3]), V, v)
    assert np.nonzero(got["vol"]["flip"])[0].tolist() == [0, 3]


def test_strip_across_workgroups():
    f, V = O.strip_reversed(5000, 7)
    got = _check(f, V, _random_verts(V, 5))
    assert got["n_components"] == 1 and got["n_nonorientable"] == 0


@pytest.mark.parametrize("a,b", [(7, 73), (16, 32), (19, 27), (419, 419)])
def test_sheets_at_the_seams_of_the_counts(a, b):
    """a consistently wound a x b quad sheet (topology_ref.quad_sheet) of F = 1022, 1024, 1026 faces -- just below, at and just above
    the 1024 lanes of a block of the per-block counts -- and of F = 351 122, 343 blocks for the one workgroup that adds them: one
    orientable component, nothing flipped; flat and open, so the volume rule decides nothing"""
    from nicer_slam_amd import mesh_topology as M
    f, V = T.quad_sheet(a, b)
    F = 2 * a * b
    t, _ = M._edge_table(f, V, F, None)
    label, orientable, flip, totals = M._orientation(f, t, F)
    assert totals == dict(n_components=1, n_nonorientable=0, n_flipped=0)
    assert int(label.abs().max()) == 0 and bool((orientable == 1).all()) and not bool(flip.any())
    i = torch.arange(V, device="cuda")
    v = torch.stack([i // (b + 1), i % (b + 1), torch.zeros_like(i)], 1).float()
    out, vol = M._orient_volume(v, f, V, F, t, label, orientable, flip)
    assert [vol[k] for k in ("n_closed", "n_decided", "n_toggled", "n_flipped")] == [0, 0, 0, 0] and not bool(out.any())
    assert vol["n"][0].item() == F and vol["flags"][0].item() == 0


def test_many_segments_and_one_across_blocks():
    """1500 tetrahedra (segments of four faces that cross the blocks of the reduction) and one component of 5000 faces, their faces in
    a seeded order and half of them reversed: every one is wound outward"""
    big = O.torus_grid(50, 50)
    v, f = O.disjoint_tets(1500, seed=5, big=big)
    got = _check(f, len(v), v)
    assert got["n_components"] == 1501 and got["vol"]["totals"][:2] == (1501, 1501) and got["vol"]["n"].max() == 5000
    fixed = O.reverse(f, got["vol"]["flip"])
    assert T.topology(fixed, len(v))["is_oriented"]
    r = O.orientation(fixed, len(v))
    assert (O.volume(v, fixed, len(v), r)["S"] > 0).all()


# ---- the public interface ---------------------------------------------------------------------------------------------------------------

def _four_spheres():
    from nicer_slam_amd import inference
    ax = torch.linspace(-1, 1, 64, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = None
    for c, r in (((-0.5, -0.5, -0.5), 0.30), ((0.5, 0.5, -0.4), 0.22), ((0.5, -0.5, 0.5), 0.15), ((-0.5, 0.6, 0.6), 0.08)):
        s = torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r
        vol = s if vol is None else torch.minimum(vol, s)
    step = float(ax[1] - ax[0])
    return inference.marching_cubes(vol.float().cuda(), 0.0, (step,) * 3, (-1.0,) * 3)


def test_scrambled_marching_cubes_mesh_comes_back_exactly():
    from nicer_slam_amd import mesh_sdf, mesh_topology as M
    m = _four_spheres()
    f, V = m["faces"], m["verts"].shape[0]
    label, n = M.face_components(f, V)
    assert n == 4
    comps = torch.unique(label)
    gen = torch.Generator().manual_seed(3)
    which = (label == comps[1]) | ((label == comps[2]) & (torch.rand(f.shape[0], generator=gen) < 0.3).cuda())
    assert 0 < int(((label == comps[2]) & which).sum()) < int((label == comps[2]).sum())
    scrambled = dict(m, faces=torch.where(which[:, None], f[:, [0, 2, 1]], f))
    assert not M.topology(scrambled)["is_oriented"]
    out, rep = M.orient(scrambled, outward="volume", return_report=True)
    assert torch.equal(out["faces"], f) and out["faces"].dtype == f.dtype and out["verts"] is scrambled["verts"]
    assert M.topology(out)["is_oriented"]
    assert (rep["n_components"], rep["n_closed"], rep["n_open"], rep["n_undecided"], rep["n_nonorientable"]) == (4, 4, 0, 0, 0)
    assert rep["n_flipped"] == int(which.sum()) and rep["is_orientable"] and rep["n_toggled"] >= 1
    assert rep["component_faces"].tolist() == [int((label == c).sum()) for c in comps]
    # the fsum oracle on the same mesh: the same decisions, the sums within the bound
    r = O.orientation(scrambled["faces"].cpu().numpy(), V)
    vol = O.volume(m["verts"].cpu().numpy(), scrambled["faces"].cpu().numpy(), V, r)
    assert (np.abs(rep["component_volume"].cpu().numpy() - vol["S"]) <= O.bound(vol["n"], vol["P"])).all()
    assert (rep["component_toggled"].cpu().numpy() == vol["toggled"]).all()
    pts = torch.rand(4096, 3, generator=gen).cuda() * 2 - 1
    d0 = mesh_sdf.signed_distance(m, pts, sign="normal")
    assert torch.equal(mesh_sdf.signed_distance(out, pts, sign="normal"), d0)
    # mesh_sdf(..., orient=True): the scrambled mesh gives the same field, and "auto" resolves to "normal" on the result
    assert torch.equal(mesh_sdf.signed_distance(scrambled, pts, sign="normal", orient=True), d0)
    assert torch.equal(mesh_sdf.signed_distance(scrambled, pts, sign="auto", orient=True), d0)
    assert mesh_sdf.resolve_sign(scrambled, "auto") == "winding"
    assert torch.equal(mesh_sdf.contains(scrambled, pts, orient=True), d0 < 0)
    g0 = mesh_sdf.mesh_sdf_grid(m, 16, band=0.2)
    assert torch.equal(torch.nan_to_num(mesh_sdf.mesh_sdf_grid(scrambled, 16, band=0.2, orient=True)), torch.nan_to_num(g0))
    # every face inwards: "oriented" for the topology, the opposite sign everywhere -- until it is turned outward
    inward = dict(m, faces=f[:, [0, 2, 1]].contiguous())
    assert M.topology(inward)["is_oriented"]
    out, rep = M.orient(inward, return_report=True)
    assert torch.equal(out["faces"], f) and rep["n_toggled"] == 4 and rep["n_flipped"] == f.shape[0]


def test_normals_kinds_and_the_index_cache(mc):
    from nicer_slam_amd import mesh_topology as M
    from nicer_slam_amd.mesh_eval import TriIndex
    m = mc["sphere"]
    f = m["faces"]
    inward = dict(verts=m["verts"], faces=O.reverse(f, np.ones(len(f), bool)).astype(np.int64), normals=m["normals"], colors=m["verts"] * 0.5)
    out, rep = M.orient(inward, return_report=True)
    assert isinstance(out["faces"], np.ndarray) and out["faces"].dtype == np.int64 and (out["faces"] == f).all()
    assert (out["normals"] == -m["normals"]).all() and rep["n_mixed_normals"] == 0 and out["colors"] is inward["colors"]
    g, which = O.seeded_reversal(f, 0.3, seed=11)
    out, rep = M.orient(dict(inward, faces=g), return_report=True)
    at = np.zeros(len(m["verts"]), np.int64)
    fl = np.zeros(len(m["verts"]), np.int64)
    np.add.at(at, g.reshape(-1), 1)
    np.add.at(fl, g[which].reshape(-1), 1)
    assert (out["faces"] == f).all() and rep["n_mixed_normals"] == int(((fl > 0) & (fl < at)).sum()) > 0
    neg = (at > 0) & (fl == at)
    assert (out["normals"] == np.where(neg[:, None], -m["normals"], m["normals"])).all()
    # outward=None: step 1 alone; torch on the host comes back on the host
    host = {"verts": torch.from_numpy(m["verts"]), "faces": torch.from_numpy(g)}
    out = M.orient(host, outward=None)
    r = O.orientation(g, len(m["verts"]))
    assert not out["faces"].is_cuda and (out["faces"].numpy() == O.reverse(g, r["flip"])).all()
    label, orientable, flip, rep = M.orientation(host)
    assert not label.is_cuda and (flip.numpy() == r["flip"]).all() and orientable.all() and rep["n_flipped"] == r["n_flipped"]
    # weld: a soup of the tetrahedron's faces with one reversed is one component only when welded; the flips land on the soup's faces
    soup = dict(verts=O.TET_VERTS[O.reverse(T.TET, [2])].reshape(-1, 3), faces=np.arange(12, dtype=np.int32).reshape(4, 3))
    assert M.orientation(soup)[3]["n_components"] == 4
    out, rep = M.orient(soup, weld=True, return_report=True)
    assert rep["n_components"] == 1 and rep["n_closed"] == 1 and (out["faces"] == O.reverse(soup["faces"], [2])).all()
    ix = TriIndex(torch.from_numpy(m["verts"]).cuda(), torch.from_numpy(g).cuda())
    a, b = ix.orientation(weld=False), ix.orientation(weld=False)
    assert a[2] is b[2] and (a[2].cpu().numpy() == r["flip"]).all() and a[3]["n_flipped"] == r["n_flipped"] and a[3] is not b[3]


def _look(eye, forward, right):
    z, x = np.asarray(forward, np.float64), np.asarray(right, np.float64)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, np.cross(z, x), z, eye
    return P


def test_views_turn_the_normals_towards_the_cameras(mc):
    from nicer_slam_amd import mesh_topology as M
    m = mc["cut sphere"]                                                     # centre (0.7, 0, 0), r 0.6, cut open by the plane x = 1
    g, _ = O.seeded_reversal(m["faces"], 0.3, seed=12)
    V, K, size = len(m["verts"]), (20.0, 20.0, 15.5, 15.5), (32, 32)
    centre = np.array([0.7, 0.0, 0.0])

    def radial(faces):
        tri = m["verts"][faces].astype(np.float64)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        return (n * (tri.mean(1) - centre)).sum(1)

    r = O.orientation(g, V)
    for P, outward in ((_look((-0.6, 0, 0), (1, 0, 0), (0, 1, 0)), True), (_look(centre, (-1, 0, 0), (0, 1, 0)), False)):
        out, rep = M.orient(dict(verts=m["verts"], faces=g), outward="views", c2w=P, intrinsics=K, size=size, return_report=True)
        d = radial(out["faces"])
        assert (d > 0).all() if outward else (d < 0).all()
        hit, dirs = M._view_hits(torch.from_numpy(m["verts"]).cuda(), torch.from_numpy(g).cuda(), P, K, size)
        assert int((hit >= 0).sum()) > 100
        votes = O.view_votes(m["verts"], g, r["flip"], hit.cpu().numpy(), dirs.cpu().numpy())
        assert rep["component_votes"].tolist() == O.component_votes(votes, r["orient_label"])[1].tolist()
        assert rep["component_votes"][0] != 0 and rep["n_undecided"] == 0 and rep["n_open"] == 1
        assert bool(rep["component_toggled"][0]) == bool(rep["component_votes"][0] < 0)
    # a camera that sees nothing: undecided, the winding of step 1
    out, rep = M.orient(dict(verts=m["verts"], faces=g), outward="views", c2w=_look((-1.5, 0, 0), (-1, 0, 0), (0, 1, 0)), intrinsics=K,
                        size=size, return_report=True)
    assert rep["n_undecided"] == 1 and rep["component_votes"].tolist() == [0] and (out["faces"] == O.reverse(g, r["flip"])).all()


def test_a_non_orientable_component_beside_an_orientable_one():
    from nicer_slam_amd import mesh_topology as M
    f, V = O.moebius_beside_tet()
    v = _random_verts(V, 9)
    v[V - 4:] = O.TET_VERTS
    out, rep = M.orient(dict(verts=v, faces=f), return_report=True)
    assert (out["faces"][:16] == f[:16]).all() and (out["faces"][16:] == T.TET + 16).all()
    assert (rep["n_components"], rep["n_nonorientable"], rep["n_closed"], rep["n_undecided"]) == (2, 1, 1, 1) and not rep["is_orientable"]
    assert rep["component_faces"].tolist() == [16, 4] and rep["component_closed"].tolist() == [False, True]
    label, orientable, flip, rep = M.orientation(dict(verts=v, faces=T.moebius(8)[0]))
    assert not orientable.any() and not flip.any() and (label == 0).all() and rep["n_nonorientable"] == 1


def test_command_line_round_trips_through_a_ply(tmp_path, capsys, mc):
    from nicer_slam_amd import inference, mesh_topology as M
    m = mc["torus"]
    g, _ = O.seeded_reversal(m["faces"], 0.3, seed=2)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    inference.write_ply(src, {"verts": torch.from_numpy(m["verts"]), "normals": torch.from_numpy(m["normals"]), "faces": torch.from_numpy(g)})
    before = M.main([src, "--json"])
    assert list(json.loads(capsys.readouterr().out)) == list(M.REPORT_KEYS) and not before["is_oriented"]
    rep = M.main([src, "--orient", dst, "--json"])
    assert json.loads(capsys.readouterr().out) == rep
    assert (rep["n_components"], rep["n_closed"], rep["n_undecided"], rep["outward"]) == (1, 1, 0, "volume")
    back = inference.read_ply(dst)
    assert (back["faces"] == m["faces"]).all() and (back["verts"] == m["verts"]).all()
    assert M.topology(back)["is_oriented"]
    M.main([src, "--orient", dst, "--outward", "none"])
    assert "faces reversed" in capsys.readouterr().out
    r = O.orientation(g, len(m["verts"]))
    assert (inference.read_ply(dst)["faces"] == O.reverse(g, r["flip"])).all()
