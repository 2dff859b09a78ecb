"""Mesh evaluation without a GPU: the numpy oracle (tests/eval_ref.py) against scipy and known answers, read_ply, and the
argument checks of the C ABI Section 8 entry points."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import eval_ref as E


def test_philox_oracle_known_answers():
    """the vectorised generator of the oracle is Philox4x32-10 (Random123 kat_vectors)"""
    c = E.philox4x32_10(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]],
                                 np.uint64), (0, 0))
    assert c[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    c = E.philox4x32_10(np.array([[0xFFFFFFFF] * 4], np.uint64), (0xFFFFFFFF, 0xFFFFFFFF))
    assert c[0].tolist() == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    c = E.philox4x32_10(np.array([[0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint64), (0xA4093822, 0x299F31D0))
    assert c[0].tolist() == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_brute_force_rules():
    t = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0]], np.float32)
    q = np.array([[1, 0, 0], [0.5, 0, 0], [np.inf, 0, 0], [10, 0, 0]], np.float32)
    d, i = E.nn_brute(q, t)
    assert i.tolist() == [1, 0, -1, 1]                           # duplicate -> lowest index; exact tie 0 / 1 -> 0
    assert d[0] == 0 and d[1] == np.float32(0.5) and np.isnan(d[2]) and d[3] == 9
    d, i = E.nn_brute(q, t, max_dist=0.5)                         # strict: d2 == r2 is not inside
    assert i.tolist() == [1, -1, -1, -1] and d[1] == np.inf
    d, i = E.nn_brute(np.zeros((1, 3), np.float32), np.full((2, 3), np.nan, np.float32))
    assert i.tolist() == [-1] and d[0] == np.inf


def test_oracle_metrics_agree_with_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(3)
    rec = rng.random((3000, 3)).astype(np.float32)
    gt = (rng.random((2500, 3)) * 1.1 - 0.05).astype(np.float32)
    nr = rng.normal(size=(3000, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    ng = rng.normal(size=(2500, 3))
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    da, ia = E.nn_brute(rec, gt)
    dc, ic = E.nn_brute(gt, rec)
    got = E.metrics(da, ia, dc, ic, nr, ng)
    # the reference's own arithmetic (eval_rec.py: accuracy / completion / completion_ratio / eval_pointcloud) on cKDTree
    d_acc, i_acc = spatial.cKDTree(gt).query(rec)
    d_com, i_com = spatial.cKDTree(rec).query(gt)
    assert np.array_equal(i_acc, ia) and np.array_equal(i_com, ic)
    assert got["accuracy"] == pytest.approx(np.mean(d_acc), rel=1e-6)
    assert got["completion"] == pytest.approx(np.mean(d_com), rel=1e-6)
    assert got["completion ratio"] == np.mean((d_com < 0.05).astype(np.float64))
    th = np.linspace(1.0 / 1000, 1, 1000)
    prec = [(d_acc <= t).mean() for t in th]
    rec_ = [(d_com <= t).mean() for t in th]
    with np.errstate(invalid="ignore"):                  # (the reference's F is NaN where precision + recall = 0)
        F = [2 * prec[i] * rec_[i] / (prec[i] + rec_[i]) for i in range(len(prec))]
    assert got["f-score"] == pytest.approx(F[9]) and got["f-score-15"] == pytest.approx(F[14])
    assert got["f-score-20"] == pytest.approx(F[19])
    assert got["chamfer-L2"] == pytest.approx(0.5 * ((d_com ** 2).mean() + (d_acc ** 2).mean()), rel=1e-6)
    nc = 0.5 * np.abs((nr[i_com] * ng).sum(-1)).mean() + 0.5 * np.abs((ng[i_acc] * nr).sum(-1)).mean()
    assert got["normals"] == pytest.approx(nc, rel=1e-12)


def _asymmetric_cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * np.array([1.0, 0.6, 0.3])
    return np.concatenate([p, p[: n // 5] * np.array([0.2, 1.5, 0.4]) + np.array([0.8, 0.0, 0.5])]).astype(np.float32)


def test_icp_oracle_recovers_a_rigid_transform():
    tgt = _asymmetric_cloud(800, 0)
    T = E.rigid([0.3, -0.5, 1.0], 4.0, [0.02, -0.015, 0.01])
    src = E.transform(tgt.astype(np.float64), np.linalg.inv(T)).astype(np.float32)
    out = E.icp(src, tgt, max_corr=0.1)
    assert np.abs(out["transformation"] - T).max() < 1e-4, out
    assert out["fitness"] == 1.0 and out["inlier_rmse"] < 1e-5 and 1 < out["iterations"] <= 30


def test_area_cumsum_is_monotone_across_blocks():
    rng = np.random.default_rng(1)
    a = rng.random(5000) * 10.0 ** rng.uniform(-8, 3, 5000)
    a[::7] = 0.0
    cum, total = E.area_cumsum(a)
    assert (np.diff(cum) >= 0).all() and cum[-1] == total
    assert total == pytest.approx(a.sum(), rel=1e-12)


# ---- read_ply ----------------------------------------------------------------------------------------------------------------

def _mesh(colors):
    g = torch.Generator().manual_seed(5)
    m = {"verts": torch.randn(40, 3, generator=g), "normals": torch.randn(40, 3, generator=g),
         "faces": torch.randint(0, 40, (70, 3), generator=g, dtype=torch.int32)}
    if colors:
        m["colors"] = torch.rand(40, 3, generator=g)
    return m


@pytest.mark.parametrize("colors", [False, True])
def test_read_ply_round_trips_write_ply(tmp_path, colors):
    from nicer_slam_amd.inference import read_ply, write_ply
    m = _mesh(colors)
    write_ply(tmp_path / "m.ply", m)
    r = read_ply(tmp_path / "m.ply")
    assert np.array_equal(r["verts"], m["verts"].numpy()) and np.array_equal(r["normals"], m["normals"].numpy())
    assert r["faces"].dtype == np.int32 and np.array_equal(r["faces"], m["faces"].numpy())
    if colors:
        want = np.rint(np.clip(m["colors"].numpy(), 0, 1) * 255).astype(np.uint8)
        assert np.array_equal(np.rint(r["colors"] * 255).astype(np.uint8), want)
    else:
        assert "colors" not in r


def test_read_ply_ascii_with_quads(tmp_path):
    from nicer_slam_amd.inference import read_ply
    text = """ply
format ascii 1.0
comment hand written
element vertex 5
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
element face 2
property list uchar int vertex_indices
end_header
0 0 0 255 0 0
1 0 0 0 255 0
1 1 0 0 0 255
0 1 0 10 20 30
0.5 0.5 1e-1 1 2 3
4 0 1 2 3
3 0 1 4
"""
    (tmp_path / "a.ply").write_text(text)
    r = read_ply(tmp_path / "a.ply")
    assert r["verts"].shape == (5, 3) and r["verts"][4, 2] == np.float32(0.1)
    assert r["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
    assert r["colors"][3].tolist() == pytest.approx([10 / 255, 20 / 255, 30 / 255])
    assert "normals" not in r


def _binary_ply(vert_props, verts, face_count_t, face_idx_t, faces, extra_header=""):
    tmap = {"double": "d", "float": "f", "ushort": "H", "uint": "I", "uchar": "B", "int": "i", "short": "h"}
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}"]
    head += [f"property {t} {n}" for n, t in vert_props]
    head += [f"element face {len(faces)}", f"property list {face_count_t} {face_idx_t} vertex_indices"]
    if extra_header:
        head.append(extra_header)
    head.append("end_header")
    out = ("\n".join(head) + "\n").encode()
    vfmt = "<" + "".join(tmap[t] for _, t in vert_props)
    for v in verts:
        out += struct.pack(vfmt, *v)
    for f in faces:
        out += struct.pack("<" + tmap[face_count_t] + tmap[face_idx_t] * len(f), len(f), *f)
    return out


def test_read_ply_binary_property_types(tmp_path):
    from nicer_slam_amd.inference import read_ply
    verts = [(0.1, 0.2, 0.3, 7, 1.0), (1.5, 2.5, -3.5, 65535, 2.0), (1e-3, 4.0, 5.0, 0, 3.0), (2.0, 2.0, 2.0, 12, 4.0)]
    props = [("x", "double"), ("y", "double"), ("z", "double"), ("quality", "ushort"), ("w", "float")]
    faces = [(0, 1, 2, 3), (1, 2, 3)]                                   # quad + triangle: variable-length lists
    data = _binary_ply(props, verts, "uchar", "uint", faces)
    (tmp_path / "b.ply").write_bytes(data)
    r = read_ply(tmp_path / "b.ply")
    assert r["verts"].tolist() == np.array([v[:3] for v in verts], np.float64).astype(np.float32).tolist()
    assert r["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [1, 2, 3]]
    data = _binary_ply(props, verts, "ushort", "int", [(0, 1, 2, 3), (3, 2, 1, 0)])   # fixed-length quads
    (tmp_path / "c.ply").write_bytes(data)
    assert read_ply(tmp_path / "c.ply")["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 1], [3, 1, 0]]


@pytest.mark.parametrize("case", ["magic", "no_end", "format", "big_endian", "property", "unknown", "truncated_vertex",
                                  "truncated_face", "index_high", "index_negative", "no_xyz", "short_face", "ascii_short"])
def test_read_ply_rejects_malformed_files(tmp_path, case):
    from nicer_slam_amd.inference import read_ply
    props = [("x", "float"), ("y", "float"), ("z", "float")]
    verts = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    good = _binary_ply(props, verts, "uchar", "int", [(0, 1, 2)])
    data = {
        "magic": b"plx" + good[3:],
        "no_end": good.replace(b"end_header", b"end_heade_"),
        "format": good.replace(b"binary_little_endian 1.0", b"binary_little_endian"),
        "big_endian": good.replace(b"binary_little_endian", b"binary_big_endian"),
        "property": good.replace(b"property float y", b"property quad y"),
        "unknown": good.replace(b"element face", b"elephant face"),
        "truncated_vertex": _binary_ply(props, verts, "uchar", "int", [])[:-5],
        "truncated_face": good[:-2],
        "index_high": _binary_ply(props, verts, "uchar", "int", [(0, 1, 3)]),
        "index_negative": _binary_ply(props, verts, "uchar", "int", [(0, -1, 2)]),
        "no_xyz": _binary_ply([("x", "float"), ("y", "float"), ("w", "float")], verts, "uchar", "int", [(0, 1, 2)]),
        "short_face": _binary_ply(props, verts, "uchar", "int", [(0, 1)]),
        "ascii_short": b"ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                       b"end_header\n0 0 0\n1 1\n",
    }[case]
    (tmp_path / "bad.ply").write_bytes(data)
    with pytest.raises(ValueError):
        read_ply(tmp_path / "bad.ply")


# ---- C ABI -------------------------------------------------------------------------------------------------------------------

def test_section8_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib, EXPORTS
    NSA_EBADARG = 4
    for name in ("nsa_nn_workspace", "nsa_nn_build", "nsa_nn_query", "nsa_surface_sample_workspace", "nsa_surface_sample"):
        assert name in EXPORTS
    fake = ctypes.c_void_p(4096)                          # never dereferenced: every call below is rejected before a launch
    assert lib.nsa_nn_workspace(0) == 0 and lib.nsa_nn_workspace(1 << 31) == 0 and lib.nsa_nn_workspace(1000) > 16000
    assert lib.nsa_surface_sample_workspace(0) == 0 and lib.nsa_surface_sample_workspace(1000) >= 8000
    assert lib.nsa_nn_build(None, 10, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_build(fake, 10, None, None) == NSA_EBADARG
    assert lib.nsa_nn_build(fake, 0, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_build(fake, 1 << 31, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query(None, 10, fake, 5, math.inf, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query(fake, 0, fake, 5, math.inf, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query(fake, 10, None, 5, math.inf, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query(fake, 10, fake, 5, math.inf, None, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query(fake, 10, fake, 5, math.inf, fake, None, None) == NSA_EBADARG
    assert lib.nsa_nn_query(fake, 10, fake, 1 << 31, math.inf, fake, fake, None) == NSA_EBADARG
    for bad in (0.0, -1.0, math.nan):
        assert lib.nsa_nn_query(fake, 10, fake, 5, bad, fake, fake, None) == NSA_EBADARG
    assert lib.nsa_nn_query(fake, 10, None, 0, 1.0, None, None, None) == 0                  # nothing to do
    args = dict(v=fake, V=4, f=fake, F=2, n=10, seed=0, ws=fake, p=fake, fi=fake, tot=None)
    for key, val in (("v", None), ("f", None), ("ws", None), ("V", 0), ("F", 0), ("p", None), ("fi", None),
                     ("F", 1 << 31), ("n", 1 << 31), ("V", 1 << 31)):
        a = dict(args, **{key: val})
        assert lib.nsa_surface_sample(a["v"], a["V"], a["f"], a["F"], a["n"], a["seed"], a["ws"], a["p"], a["fi"], a["tot"],
                                      None) == NSA_EBADARG, key
