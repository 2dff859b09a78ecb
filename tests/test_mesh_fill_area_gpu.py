"""Minimum-area hole patches on the device (header Section 24, csrc/mesh_fill_area.hip) against the numpy statement of
tests/fill_area_ref.py: the chord mask, W BIT FOR BIT, J, the classes, the totals and the new faces element for element -- the
statement is + - * and one correctly rounded square root on float64 in a stated order, and a minimum that is exact in any order, so no
tolerance takes part -- and a second run byte-identical.  Then the public interface, the other tools on the result, the
extract_mesh keywords, a PLY round trip, the command line and the rounding of the device's square root."""
import json

import numpy as np
import pytest
import torch

import clean_ref
import fill_area_ref as A
import fill_ref as R
import simplify_ref
import smooth_ref as S
import topology_ref as T

pytestmark = pytest.mark.gpu


def _tables(mesh, method, max_area_edges=2048, min_sin=1e-6, weld=False, **kw):
    """the three entry points of Section 24 on the device, with the views of the workspace"""
    from nicer_slam_amd import mesh_fill as M
    k_rings = M._checked_args(kw.get("max_edges"), kw.get("max_size"), "auto", 64, 0, 0.5, "none")
    v, f, names, mask, colors, V, F, _ = M._arrays(mesh, "test", weld, "cuda")
    r = M._loops(v, f, names, mask, colors, V, F, kw.get("max_edges"), kw.get("max_size"), k_rings, 64, kw.get("skip_folded", True))
    a = M._area(v, f, names, V, F, r, 1 << 5 if method == "auto" else 1 | 1 << 5, max_area_edges, min_sin, tables=True)
    torch.cuda.synchronize()
    return a


def _check(mesh, method, tables=True, **kw):
    """the device against the oracle, twice; returns (device result, device report, oracle result)"""
    from nicer_slam_amd import mesh_fill as M
    got, rep = M.fill_holes(mesh, normals="none", return_report=True, method=method, **kw)
    again, rep2 = M.fill_holes(mesh, normals="none", return_report=True, method=method, **kw)
    ref = A.fill_holes(mesh, method=method, **kw)
    p = ref["patches"]
    print(f"V {len(mesh['verts'])} F {len(mesh['faces'])} {method} -> {rep['totals']} {rep['area_totals']}")
    for k in ("verts", "faces", "colors"):
        assert (k in got) == (k in ref)
        if k in ref:
            assert got[k].tobytes() == again[k].tobytes(), k
            assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
    for k in ("order", "ints", "reals", "new_vertex", "area", "area_ints"):
        assert rep[k].tobytes() == rep2[k].tobytes(), k
    assert rep["totals"] == rep2["totals"] == ref["totals"] and rep["area_totals"] == rep2["area_totals"] == ref["area_totals"]
    assert (rep["ints"] == ref["ints"]).all() and (rep["reals"].view(np.uint64) == ref["reals"].view(np.uint64)).all()
    assert rep["area_ints"].shape == ref["area_ints"].shape and (rep["area_ints"] == ref["area_ints"]).all()
    assert (rep["area"].view(np.uint64) == ref["area"].view(np.uint64)).all()
    cls = ref["area_ints"][:, 0].tolist()
    assert rep["area_class"] == [A.AREA_CLASSES[c] if c >= 0 else None for c in cls]
    assert rep["area_faces"] == [int(n) - 2 if c == 0 else 0 for c, n in zip(cls, ref["area_ints"][:, 1])]
    assert rep["area_face_offset"] == ref["area_ints"][:, 5].tolist()
    polar = [method == "auto" and c == R.FILLED for c in ref["ints"][:, 3]]
    assert rep["method"] == ["min_area" if c >= 0 else "polar" if q else None for c, q in zip(cls, polar)]
    assert (got["faces"] == ref["faces"]).all()
    assert (got["verts"].view(np.uint32) == ref["verts"].view(np.uint32)).all()
    if "colors" in ref:
        assert (got["colors"].view(np.uint32) == ref["colors"].view(np.uint32)).all()
    if tables:
        a = _tables(mesh, method, **kw)
        assert a["totals"] == ref["area_totals"] and (a["ints"].cpu().numpy() == ref["area_ints"]).all()
        if ref["area_totals"]["n_cells"]:
            W, WT, J, mask = (a[k].cpu().numpy() for k in ("W", "WT", "J", "mask"))
            assert mask.tolist() == p["mask"].astype(np.uint8).tolist()
            bad = np.nonzero(W.view(np.uint64) != p["W"].view(np.uint64))[0]
            assert len(bad) == 0, (len(bad), bad[:5], W[bad[:5]], p["W"][bad[:5]])
            assert (J == p["J"]).all()
            o = 0
            for l in sorted(ref["tables"]):
                n = len(ref["tables"][l][0])
                assert WT[o:o + n * n].reshape(n, n).T.tobytes() == W[o:o + n * n].reshape(n, n).tobytes(), l
                o += n * n
        else:
            assert "W" not in a                                                       # no table was allocated
    return got, rep, ref


# ---- the loops of the issue -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["auto", "min_area"])
@pytest.mark.parametrize("name", sorted(A.small_cases()))
def test_small_loops_and_refusals(name, method):
    mesh, kw = A.small_cases()[name]
    got, rep, ref = _check(mesh, method, **kw)
    if name == "collinear tetrahedron":
        assert rep["area_class"] == ["no_triangulation"] and got["faces"].tobytes() == mesh["faces"].tobytes()
    if name == "strip" and method == "auto":
        top = T.topology(got["faces"], len(got["verts"]))
        assert rep["area_class"] == ["area_filled"] and top["euler"] == 2 and top["is_watertight"] and top["is_oriented"]


@pytest.mark.parametrize("name", sorted(A.collar_cases()))
def test_collars(name):
    mesh, kw, _ = A.collar_cases()[name]
    got, rep, ref = _check(R.with_colors(mesh), "min_area", **kw)
    assert rep["area_totals"]["n_area_filled"] == 1 and got["verts"].tobytes() == mesh["verts"].tobytes()
    if name.startswith("comb"):
        assert rep["class"][0] == "folded"
        auto, _, _ = _check(mesh, "auto", tables=False, **kw)
        assert auto["faces"].tobytes() == got["faces"].tobytes()


def test_u_grid():
    from nicer_slam_amd import mesh_topology
    mesh = A.u_grid()
    before = T.topology(mesh["faces"], len(mesh["verts"]))
    got, rep, _ = _check(mesh, "auto", max_edges=16)
    assert rep["class"] == ["too_many_edges", "folded"] and rep["area_class"] == [None, "area_filled"] and rep["area"][1] == 7.0
    assert len(got["faces"]) == len(mesh["faces"]) + 14 and T.topology(got["faces"], len(got["verts"]))["euler"] == before["euler"] + 1
    full, rep, _ = _check(mesh, "auto")
    top = mesh_topology.topology(full)
    assert rep["method"] == ["polar", "min_area"] and top["is_watertight"] and top["is_oriented"] and top["euler"] == 2


def test_over_the_cap_allocates_nothing():
    f, V = T.strip(5000)
    mesh = A.mesh(S.index_only_mesh(f, V), f)
    got, rep, _ = _check(mesh, "auto")
    assert rep["n"] == [5002] and rep["area_class"] == ["area_too_many_edges"] and rep["area_totals"]["n_cells"] == 0
    assert got["faces"].tobytes() == mesh["faces"].tobytes() and got["verts"].tobytes() == mesh["verts"].tobytes()


def test_many_small_loops_share_the_launches():
    got, rep, _ = _check(A.grid65(), "min_area", max_edges=4)
    assert rep["area_totals"] == dict(n_selected=256, n_area_filled=256, n_area_too_many_edges=0, n_no_triangulation=0, n_area_faces=512,
                                      n_cells=4096, max_n=4)
    top = T.topology(got["faces"], len(got["verts"]))
    assert top["n_boundary"] == 256 and top["n_boundary_loops"] == 1 and top["euler"] == 1 and top["n_nonmanifold"] == 0


def test_adversarial_lists_and_non_finite_vertices():
    for name, (f, V) in clean_ref.adversarial_cases(2000).items():
        mesh = R.with_colors(A.mesh(simplify_ref.adversarial_mesh(f, V), f))
        for method, kw in (("auto", {}), ("min_area", dict(skip_folded=False, max_edges=200, rings=2))):
            _check(mesh, method, max_area_edges=256, **kw)


# ---- the public interface -------------------------------------------------------------------------------------------------------------

def test_polar_is_the_default_and_unchanged():
    from nicer_slam_amd import mesh_fill as M
    for mesh in (A.u_grid(), R.table_cases()["cut sphere"][0]):
        a, ra = M.fill_holes(mesh, return_report=True)
        b, rb = M.fill_holes(mesh, method="polar", return_report=True)
        ref = R.fill_holes(mesh)
        new = {"method", "area_class", "area", "area_faces", "area_face_offset", "area_ints", "area_totals"}
        assert set(ra) == set(rb) and not new & set(ra)
        assert new <= set(M.fill_holes(mesh, method="auto", return_report=True)[1]) - set(ra)
        for k in ("verts", "faces", "colors"):
            if k in ref:
                assert a[k].tobytes() == b[k].tobytes() == ref[k].tobytes(), k
        assert ra["totals"] == rb["totals"] == ref["totals"]


def test_arguments():
    from nicer_slam_amd import mesh_fill as M
    mesh = A.u_grid()
    for kw in (dict(method="area"), dict(method="auto", skip_folded=False), dict(method="auto", max_area_edges=0),
               dict(method="auto", max_area_edges=16385), dict(method="min_area", min_sin=-1.0), dict(method="min_area", min_sin=np.nan)):
        with pytest.raises(ValueError):
            M.fill_holes(mesh, **kw)


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    from nicer_slam_amd._native import lib
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p, s = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    before = buf.clone()
    plan = lambda **kw: lib.nsa_mesh_fill_area_plan(*[{**dict(a=p, b=p, F=8, B=6, mask=33, cap=2048, c=p, d=p, s=s), **kw}[k]
                                                      for k in ("a", "b", "F", "B", "mask", "cap", "c", "d", "s")])
    assert plan(F=0, B=0) == 0 and plan(B=0) == 0                                      # nothing to do: nothing launched, nothing written
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(d=None), dict(cap=0), dict(cap=16385), dict(mask=64), dict(B=25),
               dict(F=2 ** 30)):
        assert plan(**kw) != 0, kw
    assert lib.nsa_mesh_fill_area_workspace(0, 0) == 0 and lib.nsa_mesh_fill_area_workspace(3, 9) == 0          # fewer cells than rows
    assert lib.nsa_mesh_fill_area_workspace(9, 3) % 256 == 0 and lib.nsa_mesh_fill_area_workspace(9, 3) > 0
    names = ("verts", "V", "faces", "names", "F", "edges", "etot", "order", "B", "lints", "ftot", "aints", "cells", "rows", "max_n", "nf",
             "ms2", "ws", "area", "new", "fin", "s")
    good = dict(verts=p, V=4, faces=p, names=None, F=8, edges=p, etot=p, order=p, B=6, lints=p, ftot=p, aints=p, cells=9, rows=3, max_n=3,
                nf=1, ms2=1e-12, ws=p, area=p, new=p, fin=p, s=s)
    tables = lambda **kw: lib.nsa_mesh_fill_area_tables(*[{**good, **kw}[k] for k in names])
    assert tables(cells=0, rows=0, max_n=0, nf=0) == 0                                 # no tabled loop: nothing launched
    for kw in (dict(verts=None), dict(faces=None), dict(edges=None), dict(etot=None), dict(order=None), dict(lints=None), dict(ftot=None),
               dict(aints=None), dict(ws=None), dict(area=None), dict(new=None), dict(fin=None), dict(ms2=-1.0), dict(ms2=float("nan")),
               dict(max_n=2), dict(max_n=16385), dict(rows=7), dict(cells=8), dict(nf=4), dict(B=25), dict(F=0), dict(cells=3 * 16384 + 1)):
        assert tables(**kw) != 0, kw
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_kinds_in_and_out():
    from nicer_slam_amd import mesh_fill as M
    mesh = R.with_colors(A.u_grid())
    ref = M.fill_holes(mesh, method="auto")
    assert all(isinstance(ref[k], np.ndarray) for k in ("verts", "faces", "colors"))
    for dev in ("cpu", "cuda"):
        out = M.fill_holes({k: torch.from_numpy(x).to(dev) for k, x in mesh.items()}, method="auto")
        for k in ("verts", "faces", "colors"):
            assert torch.is_tensor(out[k]) and out[k].device.type == dev and out[k].cpu().numpy().tobytes() == ref[k].tobytes(), (dev, k)


def _seam_mesh():
    """the U grid cut in two along x = 4, the right half on a copy of the vertices: the seam crosses the U's two arms"""
    v, f = R.grid_without(9, A.U_CELLS)
    left = f[v[f].mean(1)[:, 0] < 4.0]
    right = f[v[f].mean(1)[:, 0] >= 4.0] + len(v)
    return A.mesh(np.concatenate([v, v]), np.concatenate([left, right]))


def test_weld_across_a_seam():
    from nicer_slam_amd import mesh_eval, mesh_fill as M
    mesh = _seam_mesh()
    names = mesh_eval.welded_faces(torch.from_numpy(mesh["verts"]).cuda(), torch.from_numpy(mesh["faces"]).cuda()).cpu().numpy()
    got, rep = M.fill_holes(mesh, weld=True, method="auto", max_edges=16, return_report=True, normals="none")
    ref = A.fill_holes(mesh, method="auto", max_edges=16, names=names)
    assert rep["class"] == [R.CLASSES[c] for c in ref["ints"][:, 3]] and "folded" in rep["class"]
    assert (rep["area_ints"] == ref["area_ints"]).all() and (got["faces"] == ref["faces"]).all()
    assert rep["area_totals"]["n_area_filled"] == 1 and rep["area"][rep["area_class"].index("area_filled")] == 7.0
    new = got["faces"][len(mesh["faces"]):]
    assert len(new) == 14 and (new >= 81).any() and (new < 81).any()                   # the patch names duplicates of both halves
    plain = M.fill_holes(mesh, method="auto", max_edges=16, return_report=True)[1]
    assert plain["area_totals"]["n_area_filled"] == 0                                  # by index the seam is boundary: no loop of 16


def test_normals_are_kept():
    from nicer_slam_amd import mesh_fill as M
    mesh = A.u_grid()                                    # (the outer loop stays open: its flat patch would face the grid itself)
    V = len(mesh["verts"])
    stored = np.random.default_rng(0).standard_normal((V, 3)).astype(np.float32)
    kept = M.fill_holes(dict(mesh, normals=stored), method="min_area", max_edges=16)
    assert kept["normals"].tobytes() == stored.tobytes() and len(kept["verts"]) == V
    ref = A.fill_holes(mesh, method="min_area", max_edges=16)
    want = S.vertex_normals(ref["verts"], ref["faces"], "angle")
    assert np.abs(M.fill_holes(mesh, method="min_area", max_edges=16, normals="angle")["normals"] - want).max() <= 2.0 ** -22
    area = M.fill_holes(mesh, method="min_area", max_edges=16, normals="area")["normals"]
    assert area.tobytes() == S.vertex_normals(ref["verts"], ref["faces"], "area").tobytes()
    assert "normals" not in M.fill_holes(mesh, method="min_area", max_edges=16)


def test_sign_rule_and_ply_round_trip(tmp_path):
    """a prism over the comb outline, open at both ends, neither end star-shaped: closed by two minimum-area patches"""
    from nicer_slam_amd import inference, mesh_fill as M, mesh_sdf, mesh_topology
    mesh = {k: torch.from_numpy(x).cuda() for k, x in A.collar(A.comb(21)).items()}
    assert mesh_sdf.resolve_sign(mesh, "auto") == "winding"
    still, rep = M.fill_holes(mesh, return_report=True)
    assert rep["class"] == ["folded", "folded"] and mesh_sdf.resolve_sign(still, "auto") == "winding"
    out = M.fill_holes(mesh, method="auto", normals="angle")
    r = mesh_topology.topology(out)
    assert r["is_watertight"] and r["is_oriented"] and r["euler"] == 2
    assert mesh_sdf.resolve_sign(out, "auto") == "normal"
    path = str(tmp_path / "filled.ply")
    inference.write_ply(path, out)
    back = inference.read_ply(path)
    assert back["verts"].tobytes() == out["verts"].cpu().numpy().tobytes() and np.array_equal(back["faces"], out["faces"].cpu().numpy())


def test_command_line(tmp_path, capsys):
    from nicer_slam_amd import inference, mesh_fill as M
    mesh = A.u_grid()
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    full = dict(mesh, normals=S.vertex_normals(mesh["verts"], mesh["faces"], "area"))
    inference.write_ply(src, {k: torch.from_numpy(x) for k, x in full.items()})
    t = M.main([src, "--out", dst, "--method", "auto", "--max-edges", "16", "--json"])
    assert json.loads(capsys.readouterr().out) == t and t["n_area_filled"] == 1 and t["n_area_faces"] == 14 and t["n_folded"] == 1
    assert len(inference.read_ply(dst)["faces"]) == len(mesh["faces"]) + 14
    M.main([src, "--list", "--method", "min_area", "--max-area-edges", "20", "--min-sin", "1e-4"])
    out = capsys.readouterr().out
    assert "loop 0: 32 edges, filled, " in out and "area_too_many_edges" in out and "loop 1: 16 edges, folded" in out
    assert "area_filled, area 7" in out and "minimum-area patches: 1 of 2 loops, +14 faces, 1 over the edge cap" in out
    with pytest.raises(SystemExit):
        M.main([src, "--out", dst, "--method", "some"])
    capsys.readouterr()


def test_extract_mesh_keywords():
    """fill_holes=dict(method="auto") through both extract_mesh equals the call made by hand"""
    from nicer_slam_amd import inference, mesh_fill as M
    from nicer_slam_amd.tsdf import TSDFVolume
    from test_mesh_gpu import _model
    import tsdf_ref
    m = _model()
    kw = dict(method="auto", max_edges=4096, max_area_edges=256, normals="angle")
    plain = inference.extract_mesh(m, 32, (-0.5, 0.5))                                  # the box cuts the surface
    by_hand, rep = M.fill_holes(plain, return_report=True, **kw)
    fused = inference.extract_mesh(m, 32, (-0.5, 0.5), fill_holes=kw)
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)
    assert "area_totals" in rep
    poses = tsdf_ref.ring_poses(4)
    depth, rgb = tsdf_ref.room_frames(poses, 60, 80, 50.0)
    vl = 0.06
    vol = TSDFVolume((-0.72,) * 3, (0.72,) * 3, vl, 4 * vl, True)
    vol.integrate(depth, rgb, poses, tsdf_ref.pinhole(60, 80, 50.0))
    kw = dict(method="auto", max_area_edges=260)
    by_hand, rep = M.fill_holes(vol.extract_mesh(), return_report=True, **kw)
    fused = vol.extract_mesh(fill_holes=kw)
    print(rep["n"], rep["class"], rep["area_class"], rep["area_totals"])
    assert set(fused) == set(by_hand) and all(torch.equal(fused[k], by_hand[k]) for k in fused)


# ---- the square root ------------------------------------------------------------------------------------------------------------------

def test_the_device_square_root_is_correctly_rounded():
    """10^5 positive doubles against numpy.sqrt, bit for bit: half of them log-uniform over the exponent range with random
    mantissas, half beside a rounding boundary -- for an fp32-exact x with an odd last bit, x^2 is exact in float64, and the roots of
    x^2 minus and plus one ulp are x less or more about 2^-29 ulp of x, which must round back to x: a root that is off in its last
    place shows there -- and the ends of the range, a subnormal and zero"""
    from nicer_slam_amd._native import check, lib
    rng = np.random.default_rng(24)
    n = 25000
    rand = np.ldexp(rng.uniform(1.0, 2.0, 2 * n), rng.integers(-1000, 1000, 2 * n))
    m = (rng.integers(1 << 22, 1 << 23, n) * 2 + 1).astype(np.float64)                 # 24-bit odd mantissas
    x = np.ldexp(m, rng.integers(-500, 480, n))
    sq = x * x
    assert (sq.astype(np.float64) == x * x).all() and (np.sqrt(sq) == x).all()
    vals = np.concatenate([rand, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf),
                           [np.finfo(np.float64).tiny, np.finfo(np.float64).max, 5e-324, 1.0, 2.0, 0.0]])
    assert len(vals) >= 10 ** 5
    dev = torch.from_numpy(vals).cuda()
    out = torch.empty_like(dev)
    check(lib.nsa_mesh_fill_area_roots(dev.data_ptr(), len(vals), out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    got, want = out.cpu().numpy(), np.sqrt(vals)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    print(f"{len(vals)} roots, {len(bad)} differ from numpy.sqrt")
    assert len(bad) == 0, (len(bad), vals[bad[:5]], got[bad[:5]], want[bad[:5]])
