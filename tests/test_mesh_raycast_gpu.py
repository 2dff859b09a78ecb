"""Ray casting against a mesh on the GPU (csrc/mesh_raycast.hip, header Section 17) against the numpy oracle tests/raycast_ref.py:
the tree's layout, then t, the face and the barycentrics BIT FOR BIT and the two per-ray counts exactly, for the tree kernel and for
the brute-force kernel; the any-hit flag, windows and culling; and nicer_slam_amd.mesh_raycast end to end -- a camera inside a room
of twelve faces, which the rasteriser cannot draw, the rasteriser's own images where it can, occlusion and visibility, pruning."""
import functools

import numpy as np
import pytest
import torch

import p2m_ref as P
import raster_ref as rr
import raycast_ref as R
from test_mesh_closest_gpu import _cuda, _index, _mc_sphere
from test_mesh_raycast_cpu import (FACE_MARGIN, cases, mixed_rays, raster_depth_bound, room_case, same_answer, same_bits, sphere_view,
                                   tree_of, walked)
from test_mesh_sdf_gpu import _mixed_mesh

pytestmark = pytest.mark.gpu


def _gpu(ix, o, d, **kw):
    t, face, bary, nn, nt = ix.raycast(_cuda(o, torch.float32), _cuda(d, torch.float32), counts=True, **kw)
    return dict(t=t.cpu().numpy(), face=face.cpu().numpy(), bary=bary.cpu().numpy(), nodes=nn.cpu().numpy(), tested=nt.cpu().numpy())


def _same_counts(got, ref, what):
    for k in ("nodes", "tested"):
        bad = np.nonzero(got[k] != ref[k])[0]
        assert bad.size == 0, (what, k, bad[:5], got[k][bad][:5], ref[k][bad][:5])


def _check(v, f, o, d, what, tree=None, ref=None):
    """index over (v, f): the layout, then the tree kernel and the brute-force kernel against the oracle's walk, the any-hit flag,
    a window that cuts off the first hit of half the rays, and back-face culling"""
    ix = _index(v, f)
    tree = tree if tree is not None else R.Tree(v, f)
    lay = ix.ray_layout()
    assert (lay["L"], lay["nodes"], lay["usable faces"]) == (tree.L, tree.n_nodes, tree.n_usable), (what, lay)
    assert R.workspace_bound(ix.F) <= lay["bytes"] <= R.workspace_bound(ix.F) + 12 * 256
    ref = ref if ref is not None else R.walk(o, d, tree)
    got = _gpu(ix, o, d)
    same_answer(got, ref, what + ", tree")
    _same_counts(got, ref, what)
    same_answer(_gpu(ix, o, d, brute=True), ref, what + ", brute force")
    hits = np.isfinite(ref["t"])
    flag = ix.raycast(_cuda(o, torch.float32), _cuda(d, torch.float32), any_hit=True)
    assert flag.dtype == torch.bool and np.array_equal(flag.cpu().numpy(), hits), what
    assert np.array_equal(ix.raycast(_cuda(o, torch.float32), _cuda(d, torch.float32), any_hit=True, brute=True).cpu().numpy(), hits)
    print("%s: %d of %d rays hit; %.1f nodes and %.1f faces tested per ray of %d usable faces"
          % (what, hits.sum(), hits.size, got["nodes"].mean(), got["tested"].mean(), tree.n_usable))
    if hits.any():
        cut = float(np.median(ref["t"][hits]))
        for kw in (dict(tmin=cut), dict(tmax=cut)):
            ref2 = R.walk(o, d, tree, **kw)
            got2 = _gpu(ix, o, d, **kw)
            same_answer(got2, ref2, "%s, %s" % (what, kw))
            _same_counts(got2, ref2, "%s, %s" % (what, kw))
            same_answer(_gpu(ix, o, d, brute=True, **kw), ref2, "%s, %s, brute force" % (what, kw))
        # where the window cut off the first hit and something lies behind it, the answer is that second hit
        behind = R.brute(o, d, tree, tmin=cut, box=False)
        second = hits & (ref["t"] < cut) & np.isfinite(behind["t"])
        got2 = _gpu(ix, o, d, tmin=cut)
        assert np.array_equal(got2["t"][second], behind["t"][second]) and (got2["t"][second] > ref["t"][second]).all(), what
    for cull, flags in (("back", R.CULL_BACK), ("front", R.CULL_FRONT)):
        ref3 = R.walk(o[:65], d[:65], tree, flags=flags)
        got3 = _gpu(ix, o[:65], d[:65], cull=cull)
        same_answer(got3, ref3, "%s, cull %s" % (what, cull))
        _same_counts(got3, ref3, "%s, cull %s" % (what, cull))
    return ix, tree, got


def _case(name):
    v, f, o, d = cases()[name]
    return _check(v, f, o, d, name, tree_of(name), walked(name))


# ---- kernels against the oracle -------------------------------------------------------------------------------------------------

def test_both_boxes():
    ix, tree, _ = _case("unit box")
    assert tree.L == 1
    _case("stretched box")
    v, f = P.box_mesh()                                              # eight faces: L = 0, the root is the only node
    o, d = cases()["unit box"][2:]
    ix, tree, got = _check(v, f[:8], o[:257], d[:257], "eight faces of the box")
    assert tree.L == 0 and tree.n_nodes == 1 and (got["nodes"] == 1).all()


def test_spike_with_rays_through_its_apex():
    ix, tree, got = _case("spike")
    assert np.isfinite(got["t"][:33]).sum() > 16                     # aimed at the apex: most hit, the rest pass 1e-7 beside the tip


@pytest.mark.parametrize("name", ["lat-long sphere", "lat-long soup"])
def test_latlong_sphere_welded_and_as_a_soup(name):
    ix, tree, _ = _case(name)
    assert tree.L == 5 and tree.n_usable == 2208


def test_watertight_sphere():
    v, f = R.welded_latlong_sphere(24, 48)
    o, d, _ = R.watertight_rays(v, f, 513, 1, 1.0, 15.0)
    ix, tree, got = _check(v, f, o, d, "watertight rays")
    assert np.abs(got["t"] - 1.0).max() <= 1e-6 and (got["t"] == 1.0).sum() > 50


def test_marching_cubes_sphere():
    m = _mc_sphere(32)
    v, f = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    o, d = R.sphere_rays(513, 2, 3.0, 0.6)
    ix, tree, got = _check(v, f, o, d, "MC sphere")
    hit = np.isfinite(got["t"])
    p = o[hit].astype(np.float64) + got["t"][hit, None] * d[hit].astype(np.float64)
    assert np.abs(np.linalg.norm(p, axis=1) - 0.5).max() < 0.01      # the hits lie on the sphere, on its near side
    assert ((p * d[hit]).sum(1) < 0).all()


def test_mixed_scales_invalid_faces_and_degenerate_rays():
    v, f = _mixed_mesh()
    o, d = mixed_rays()
    ix, tree, got = _check(v, f, o, d, "mixed scales")
    assert tree.n_usable == f.shape[0] - 7
    assert np.isnan(got["t"][-5:]).all() and (got["face"][-5:] == -1).all() and np.isnan(got["bary"][-5:]).all()
    assert (got["nodes"][-5:] == 0).all() and (got["tested"][-5:] == 0).all() and np.isfinite(got["t"][:-5]).sum() > 100
    stray = slice(160, 184)                                           # the rays at the component 1000 units away
    assert (got["face"][stray] >= 0).sum() >= 4 and (got["t"][stray][got["face"][stray] >= 0] > 0.99).all()


def test_worst_cases_and_empty_answers():
    ix, tree, got = _case("coincident centroids")
    assert tree.n_nodes == 3 and got["tested"].max() > 20            # one leaf of 40 faces: slow, and equal to the oracle
    for name in ("open square", "three on an edge", "opposite twins"):
        _case(name)
    v, f = P.box_mesh()
    bad = np.array([[0, 0, 1], [0, 1, 99], [-1, 2, 3]], np.int32)     # no usable face
    o, d = cases()["unit box"][2:]
    ix, tree, got = _check(v, bad, o[:65], d[:65], "no usable face")
    assert tree.n_nodes == 0 and (got["t"] == np.inf).all() and (got["face"] == -1).all() and (got["nodes"] == 0).all()
    empty = torch.empty(0, 3, device="cuda")
    out = ix.raycast(empty, empty, counts=True)
    assert len(out) == 5 and out[0].shape == (0,) and out[0].dtype == torch.float64 and out[2].shape == (0, 3)
    assert ix.raycast(empty, empty, any_hit=True).shape == (0,)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 513])
def test_partial_waves_and_blocks(m):
    v, f, o, d = cases()["lat-long sphere"]
    tree, ref = tree_of("lat-long sphere"), walked("lat-long sphere")
    ix = _sphere_index()
    got = _gpu(ix, o[:m], d[:m])
    same_answer(got, {k: x[:m] for k, x in ref.items()}, "m = %d" % m)
    _same_counts(got, {k: x[:m] for k, x in ref.items()}, "m = %d" % m)
    same_answer(_gpu(ix, o[:m], d[:m], brute=True), {k: x[:m] for k, x in ref.items()}, "m = %d, brute force" % m)


@functools.lru_cache(maxsize=None)
def _sphere_index():
    v, f = cases()["lat-long sphere"][:2]
    return _index(v, f)


def test_a_second_build_gives_identical_bits():
    v, f, o, d = cases()["lat-long sphere"]
    a, b = _sphere_index(), _index(v, f)
    la = a.ray_layout()
    assert la == b.ray_layout()
    ta, tb = a._ray[0], b._ray[0]
    n = la["usable faces"]
    assert torch.equal(ta[:48], tb[:48]) and torch.equal(ta[256:256 + 4 * n], tb[256:256 + 4 * n])     # the head and the order
    first, second = _gpu(a, o, d), _gpu(b, o, d)
    same_answer(first, second, "second build")
    _same_counts(first, second, "second build")


# ---- nicer_slam_amd.mesh_raycast end to end ----------------------------------------------------------------------------------------

def test_camera_inside_a_box_room():
    """The test that states the feature: twelve large faces, the camera inside.  The ray cast gives the closed-form wall depth at
    every pixel; the rasteriser, which has no near-plane clipping, draws nothing for the faces that reach behind the camera."""
    from nicer_slam_amd import mesh_raycast, mesh_render
    mesh, c2w, K, size, want, straddles = room_case()
    got = mesh_raycast.render_depth(mesh, c2w, K, size, near=0.01)
    assert got["depth"].shape == (1,) + size and got["depth"].dtype == np.float64 and got["face_id"].dtype == np.int32
    assert got["normal"].shape == (1,) + size + (3,) and got["normal"].dtype == np.float32
    depth, face = got["depth"][0], got["face_id"][0]
    assert (face >= 0).all()                                           # a closed room: every pixel sees a wall
    rel = np.abs(depth - want) / want
    print("room: largest relative error of the ray-cast depth against the closed form %.3e" % rel.max())
    assert rel.max() <= 1e-12
    n = got["normal"][0].astype(np.float64)
    o, d = R.camera_rays(c2w, K, size)
    assert ((n.reshape(-1, 3) * d).sum(1) < 0).all() and np.abs(np.abs(n).max(-1) - 1.0).max() < 1e-6   # axis-aligned, facing the camera
    drawn = mesh_render.render_mesh(mesh, c2w, K, size, near=0.01, channels=("depth", "face_id"))
    on_straddling = straddles[face]
    assert on_straddling.mean() > 0.3                                  # a large part of the image shows such faces
    assert (drawn["face_id"][0][on_straddling] == -1).all() and (drawn["depth"][0][on_straddling] == 0).all()
    assert drawn["totals"]["depth"] == int(straddles.sum())            # the rasteriser skipped exactly those, by its DEPTH rule
    front = ~on_straddling                                             # the wall ahead: both draw it
    assert np.array_equal(drawn["face_id"][0][front], face[front])
    # sampled pixels give the image's values without the image
    px = np.array([[0, 0], [63, 47], [31, 20], [5, 40], [60, 3]])
    dd, ff, nn = mesh_raycast.depth_at(mesh, c2w, K, px)
    same_bits(dd, depth[px[:, 1], px[:, 0]], "depth_at")
    assert np.array_equal(ff, face[px[:, 1], px[:, 0]].astype(np.int64)) and np.array_equal(nn, got["normal"][0][px[:, 1], px[:, 0]])
    l1, count = mesh_render.depth_l1(mesh, want.astype(np.float32), c2w, K, near=0.01, method="raycast")
    assert count == want.size and l1 < 1e-6
    l1_raster, count_raster = mesh_render.depth_l1(mesh, want.astype(np.float32), c2w, K, near=0.01)
    assert count_raster == int(front.sum())                            # the default path: only the wall ahead


@functools.lru_cache(maxsize=None)
def _sphere_mesh():
    m = _mc_sphere(32)
    return {"verts": m["verts"].cpu().numpy(), "faces": m["faces"].cpu().numpy()}


def test_ray_cast_and_rasterised_images_of_the_sphere_agree():
    from nicer_slam_amd import mesh_raycast, mesh_render
    mesh = _sphere_mesh()
    c2w, K, size = sphere_view(32)
    cast = mesh_raycast.render_depth(mesh, c2w, K, size, near=0.01)
    drawn = mesh_render.render_mesh(mesh, c2w, K, size, near=0.01, channels=("depth", "face_id"))
    o, d = R.camera_rays(c2w, K, size)
    t, face, bary = mesh_raycast.cast_rays(mesh, o, d, tmin=0.01)
    assert np.array_equal(face.reshape(size), cast["face_id"][0].astype(np.int64))
    hit = face >= 0
    inner = hit & (np.where(hit[:, None], bary, 0.0).min(1) > FACE_MARGIN)
    print("sphere: %d pixels hit, %d (%.1f %%) within the margin %g of an edge" % (hit.sum(), (hit & ~inner).sum(),
                                                                                   100.0 * (hit & ~inner).sum() / hit.sum(), FACE_MARGIN))
    assert (hit & ~inner).sum() <= 0.2 * hit.sum()
    rf, rd = drawn["face_id"][0].reshape(-1), drawn["depth"][0].reshape(-1).astype(np.float64)
    assert np.array_equal(rf[inner], face[inner].astype(np.int32))
    bound = raster_depth_bound(mesh, c2w, K, face[inner], rd[inner], t[inner])
    err = np.abs(rd[inner] - t[inner])
    print("sphere: largest |rasterised - ray-cast depth| %.3e, largest share of Section 12's bound %.3f" % (err.max(), (err / bound).max()))
    assert (err <= bound).all()


def test_occlusion_and_visibility_by_rays():
    from nicer_slam_amd import mesh_raycast, mesh_render
    mesh = _sphere_mesh()
    v = mesh["verts"]
    eye = np.array([0.0, 0.0, 3.0], np.float32)
    hidden = mesh_raycast.occluded(mesh, eye, v)
    assert hidden.dtype == bool and hidden.shape == (len(v),)
    assert not hidden[v[:, 2] > 0.2].any() and hidden[v[:, 2] < 0.0].all()      # the cap towards the eye, and the far side
    assert (v[:, 2] > 0.2).sum() > 100 and (v[:, 2] < 0.0).sum() > 400
    pairs = mesh_raycast.occluded(mesh, np.tile(eye, (3, 1)), np.float32([[0, 0, -3], [2, 0, 3], [np.nan, 0, 0]]))
    assert pairs.tolist() == [True, False, False]
    c2w, K, size = sphere_view(32)
    seen = mesh_render.visible_faces(mesh, c2w, K, size, method="raycast")
    frustum = mesh_render.visible_faces(mesh, c2w, K, size, mode="frustum")
    raster = mesh_render.visible_faces(mesh, c2w, K, size)
    assert seen.dtype == bool and not (seen & ~frustum).any()          # a subset of what lies in the frustum
    F = len(mesh["faces"])
    print("sphere: %d faces, %d in the frustum, %d seen by rays, %d by the depth images" % (F, frustum.sum(), seen.sum(), raster.sum()))
    assert 0.3 * F < seen.sum() < 0.7 * F                              # about the half that faces the camera
    centre = mesh["verts"][mesh["faces"]].mean(1)
    towards = (centre * c2w[:3, 3]).sum(1)                             # > 0 on the camera's side of the sphere
    assert seen[towards > 0.25].all() and not seen[towards < -0.1].any()
    assert np.array_equal(mesh_render.visible_faces(mesh, c2w, K, size, mode="frustum", method="raycast"), frustum)
    culled = mesh_render.cull_mesh(mesh, c2w, K, size, method="raycast")
    assert culled["faces"].shape[0] == int(seen.sum())


@pytest.mark.parametrize("res", [32, 64])
def test_camera_rays_test_a_small_share_of_the_faces(res):
    from nicer_slam_amd import mesh_raycast
    m = _mc_sphere(res)
    ix = _index(m["verts"].cpu().numpy(), m["faces"].cpu().numpy())
    c2w, K, size = sphere_view(res)
    o, d = mesh_raycast.camera_rays(c2w, K, size, device="cuda")
    t, face, bary, nodes, tested = ix.raycast(o, d, counts=True)
    F = ix.ray_layout()["usable faces"]
    mean_tested, mean_nodes = float(tested.double().mean()), float(nodes.double().mean())
    print("%d^3 sphere: %d usable faces, %d camera rays, %d hit; %.2f faces tested and %.1f nodes visited per ray; a brute force tests %d"
          % (res, F, o.shape[0], int((face >= 0).sum()), mean_tested, mean_nodes, F))
    assert int((face >= 0).sum()) > o.shape[0] // 4
    assert mean_tested < F / 20
    if res == 32:
        ref = R.walk(o.cpu().numpy(), d.cpu().numpy(), R.Tree(m["verts"].cpu().numpy(), m["faces"].cpu().numpy()))
        assert np.array_equal(tested.cpu().numpy(), ref["tested"]) and np.array_equal(nodes.cpu().numpy(), ref["nodes"])


def test_cli_writes_depth_frames_that_depth_l1_reads_back(tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_raycast, mesh_render
    mesh, c2w, K, size, want, _ = room_case()
    v = torch.from_numpy(mesh["verts"])
    inference.write_ply(str(tmp_path / "room.ply"), {"verts": v, "normals": torch.zeros_like(v), "faces": torch.from_numpy(mesh["faces"])})
    np.save(tmp_path / "poses.npy", c2w[None])
    mesh_raycast.main([str(tmp_path / "room.ply"), "--poses", str(tmp_path / "poses.npy"), "--intrinsics"] + [str(x) for x in K]
                      + ["--size", str(size[0]), str(size[1]), "--out", str(tmp_path / "out")])
    assert "1 depth images" in capsys.readouterr().out
    d = np.load(tmp_path / "out" / "000001.npy")
    assert d.dtype == np.float32 and np.abs(d - want).max() <= 1e-6 * want.max()
    frames = mesh_render.read_depth_dir(str(tmp_path / "out"), 1)      # the millimetre PNG
    assert frames.shape == (1,) + size and np.abs(frames[0] - want).max() <= 0.5e-3 + 1e-6
