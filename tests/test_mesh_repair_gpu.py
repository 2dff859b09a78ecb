"""The fan split on the device (csrc/mesh_manifold.hip, nicer_slam_amd/mesh_repair.py; header Section 26) against the
sequential oracle tests/manifold_ref.py: every output array and every total element for element, each case run twice and compared bit
for bit; then where it plugs in -- topology, mesh_clean.components, weld, decimate, simplify(split=True), the command lines.  It is
all integer work: no tolerance anywhere."""
import json

import numpy as np
import pytest
import torch

import manifold_ref as M
import topology_ref as T

pytestmark = pytest.mark.gpu

ARRAYS = ("corner_fan", "vertex_fans", "faces", "new_source")
TOTALS = M.TOTALS[:7]


def _check(faces, V, **kw):
    """device == oracle on every array and total; a second run is bit-identical.  Returns the device result."""
    from nicer_slam_amd import mesh_repair as R
    dev = {k: (torch.as_tensor(np.asarray(x)).cuda() if k != "cut_inconsistent" else x) for k, x in kw.items()}
    f = torch.as_tensor(np.asarray(faces)).cuda()
    got = R.split_fans(f, V, **dev)
    ref = M.split_fans(faces, V, **kw)
    for k in TOTALS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ARRAYS:
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        assert np.array_equal(g, ref[k]), k
    again = R.split_fans(f, V, **dev)
    for k in TOTALS:
        assert again[k] == got[k], k
    for k in ARRAYS:
        assert torch.equal(again[k], got[k]), k
    return got


@pytest.fixture(scope="module")
def torus():
    """the device's own clustered torus: (mesh dict of CUDA tensors, faces as numpy, V)"""
    from nicer_slam_amd import mesh_simplify
    m = T.mc_mesh("torus", 16)
    mesh = {k: torch.from_numpy(np.ascontiguousarray(m[k])).cuda() for k in ("verts", "faces", "normals")}
    out = mesh_simplify.simplify(mesh, cell=0.45, placement="mean")
    return out, out["faces"].cpu().numpy(), out["verts"].shape[0]


def test_kernel_cases_equal_the_oracle_element_for_element():
    cases = M.kernel_cases()
    assert len(cases) == 21
    for name, f, V, kw in cases:
        got = _check(f, V, **kw)
        if name in M.hand_rows():
            assert got["faces"].tolist() == M.hand_rows()[name][2] and got["new_source"].tolist() == M.hand_rows()[name][3], name
        if name == "two tets sharing an edge":
            assert got["n_new"] == 2
        if name in ("moebius", "strip 5000"):
            assert got["n_new"] == 0 and np.array_equal(got["faces"].cpu().numpy(), f)        # unchanged
        if name == "vertex star 300":
            assert got["max_fans"] == 300 and got["n_pinch_only"] == 1


def test_no_faces_and_no_vertices():
    from nicer_slam_amd import mesh_repair as R
    r = R.split_fans(np.zeros((0, 3), np.int32), 5)
    assert r["vertex_fans"].tolist() == [0] * 5 and r["faces"].shape == (0, 3) and r["n_new"] == 0 and r["new_source"].shape == (0,)
    r = R.split_fans(np.zeros((0, 3), np.int32), 0)
    assert r["vertex_fans"].shape == (0,) and r["n_fans"] == 0
    _check(np.array([[0, 1, 2], [-1, 0, 5]], np.int32), 0)
    mesh = {"verts": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32)}
    assert R.split_nonmanifold(mesh)["verts"].shape == (0, 3) and R.is_manifold(mesh)


def test_clustered_torus_becomes_manifold(torus):
    from nicer_slam_amd import mesh_clean, mesh_repair as R, mesh_topology
    mesh, f, V = torus
    assert mesh_topology.topology(mesh)["n_nonmanifold"] > 0 and not R.is_manifold(mesh)
    ref = M.split_fans(f, V)
    out, rep = R.split_nonmanifold(mesh, return_report=True, return_map=True)
    assert [rep[k] for k in TOTALS] == M.totals_of(ref)[:7] and rep["n_verts_out"] == V + ref["n_new"] == out["verts"].shape[0]
    assert np.array_equal(out["faces"].cpu().numpy(), ref["faces"]) and out["faces"].dtype == mesh["faces"].dtype
    src = out["vertex_source"].long()
    assert np.array_equal(src.cpu().numpy(), np.concatenate([np.arange(V), ref["new_source"]]))
    for k in ("verts", "normals"):                        # the bits of the source
        assert torch.equal(out[k].view(torch.int32), mesh[k][src].view(torch.int32)), k
    top = mesh_topology.topology(out)
    assert top["n_nonmanifold"] == 0 and top["n_contributing"] == len(f)
    assert R.is_manifold(out)
    fans, totals = R.vertex_fans(mesh)
    assert np.array_equal(fans.cpu().numpy(), ref["vertex_fans"]) and totals["n_new"] == ref["n_new"]
    # the vertex-joined components of the result are the fan-joined components of the input
    label, n = M.fan_components(f, V)
    _, fl, C, _ = mesh_clean.components(out["faces"], out["verts"].shape[0])
    assert C == n
    fl = fl.cpu().numpy()
    firsts = {}
    for i, l in enumerate(fl):
        firsts.setdefault(int(l), i)
    assert np.array_equal(np.array([firsts[int(l)] for l in fl]), label)
    # numpy in, numpy out
    mesh_np = {k: x.cpu().numpy() for k, x in mesh.items()}
    out_np = R.split_nonmanifold(mesh_np)
    assert isinstance(out_np["verts"], np.ndarray) and np.array_equal(out_np["faces"], ref["faces"])
    assert np.array_equal(out_np["verts"].view(np.int32), out["verts"].cpu().numpy().view(np.int32))


def test_weld_undoes_the_split(torus):
    from nicer_slam_amd import mesh_repair as R
    mesh, f, V = torus
    out = R.split_nonmanifold(mesh)
    back, rep = R.weld(out, return_report=True, return_map=True)
    names = np.unique(out["verts"].cpu().numpy() + 0.0, axis=0, return_inverse=True)[1].reshape(-1)
    g, used, dropped = M.weld(out["faces"].cpu().numpy(), names, out["verts"].shape[0])
    assert np.array_equal(back["faces"].cpu().numpy(), g) and np.array_equal(back["vertex_source"].cpu().numpy(), used)
    assert rep["n_dropped"] == dropped == 0 and rep["n_verts_out"] == len(used)
    # the clustered torus uses every vertex and repeats no position: the renumbering is the identity
    assert np.array_equal(g, f) and used.tolist() == list(range(V))
    for k in ("verts", "normals"):
        assert torch.equal(back[k].view(torch.int32), mesh[k].view(torch.int32)), k
    soup = {"verts": np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [np.nan, 0, 0], [-0.0, 0, 0]], np.float32),
            "faces": np.array([[0, 1, 2], [5, 3, 2], [0, 3, 1], [0, 4, 2], [0, 1, 9]], np.int64)}
    w, rep = R.weld(soup, return_report=True, return_map=True)
    assert w["faces"].tolist() == [[0, 1, 2], [0, 1, 2], [0, 3, 2]] and w["faces"].dtype == np.int64
    assert w["vertex_source"].tolist() == [0, 1, 2, 4] and rep["n_dropped"] == 2


def test_decimate_after_split_and_simplify_with_split(torus):
    from nicer_slam_amd import mesh_decimate, mesh_repair as R, mesh_simplify, mesh_topology
    mesh, f, V = torus
    out = R.split_nonmanifold(mesh)
    dec = mesh_decimate.decimate(out, target_faces=40)
    top = mesh_topology.topology(dec)
    assert top["n_nonmanifold"] == 0 and 0 < top["n_faces"] < len(f)
    m = T.mc_mesh("torus", 16)
    src = {k: torch.from_numpy(np.ascontiguousarray(m[k])).cuda() for k in ("verts", "faces", "normals")}
    both = mesh_simplify.simplify(src, cell=0.45, placement="mean", split=True, return_map=True)
    assert torch.equal(both["faces"], out["faces"]) and torch.equal(both["verts"].view(torch.int32), out["verts"].view(torch.int32))
    assert both["vertex_cell"].shape[0] == both["verts"].shape[0] == both["vertex_source"].shape[0]
    plain = mesh_simplify.simplify(src, cell=0.45, placement="mean", split=None)
    assert torch.equal(plain["faces"], mesh["faces"])     # off by default: nothing changes
    cut = mesh_simplify.simplify(src, cell=0.45, placement="mean", split=dict(cut_inconsistent=True))
    assert mesh_topology.topology(cut)["n_inconsistent"] == 0


def test_command_lines(tmp_path, capsys, torus):
    from nicer_slam_amd import inference, mesh_repair as R, mesh_topology
    mesh, f, V = torus
    ref = M.split_fans(f, V)
    path, out_path = str(tmp_path / "torus.ply"), str(tmp_path / "split.ply")
    inference.write_ply(path, {k: x.cpu() for k, x in mesh.items()})
    r = R.main([path, "--out", out_path, "--json"])
    assert json.loads(capsys.readouterr().out) == r
    assert [r[k] for k in TOTALS] == M.totals_of(ref)[:7] and r["is_manifold"] is False and r["n_verts_out"] == V + ref["n_new"]
    back = inference.read_ply(out_path)
    assert np.array_equal(back["faces"], ref["faces"]) and back["verts"].shape[0] == V + ref["n_new"]
    assert mesh_topology.topology(back)["n_nonmanifold"] == 0
    r = R.main([out_path, "--list"])                       # the result, listed: nothing to cut
    text = capsys.readouterr().out
    assert r["is_manifold"] is True and r["n_new"] == 0 and "cut edges 0" in text and "->" not in text
    r = R.main([out_path, "--weld", "--out", str(tmp_path / "again.ply"), "--json"])
    capsys.readouterr()
    assert r["n_welded"] == ref["n_new"] and r["n_new"] == ref["n_new"]
    assert np.array_equal(inference.read_ply(str(tmp_path / "again.ply"))["faces"], ref["faces"])
    t = mesh_topology.main([path, "--split", "--json"])
    capsys.readouterr()
    assert t["n_nonmanifold"] == 0 and mesh_topology.main([path, "--json"])["n_nonmanifold"] == 17
    capsys.readouterr()
    with pytest.raises(SystemExit):
        R.main([path])
