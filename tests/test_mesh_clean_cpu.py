"""Mesh clean-up without a GPU: the numpy oracle tests/clean_ref.py on hand-written cases (and against scipy where it is
installed), Umeyama, the torch plumbing of nicer_slam_amd/mesh_clean.py on CPU tensors, the error paths, the command lines'
parsing, the argument validation of C ABI Section 11, and the labelling passes of csrc/uf_passes.hpp run by host threads."""
import ctypes

import numpy as np
import pytest
import torch

import clean_ref as C
import eval_ref as E
import host_program


def _two_quads():
    """two unit squares (two faces each) one unit apart, a degenerate face on the second, an invalid face, a spare vertex"""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2], [9, 9, 9]], np.float32)
    f = np.array([[4, 5, 6], [0, 1, 2], [4, 6, 7], [0, 2, 3], [6, 6, 7], [0, 1, 9]], np.int32)
    return {"verts": v, "faces": f, "normals": np.tile(np.array([[0, 0, 1]], np.float32), (9, 1)),
            "colors": np.arange(27, dtype=np.float32).reshape(9, 3) / 27}


def test_oracle_on_hand_written_cases():
    m = _two_quads()
    vl, fl, n, used = C.components(m["faces"], 9)
    assert vl.tolist() == [0, 0, 0, 0, 4, 4, 4, 4, -1] and fl.tolist() == [4, 0, 4, 0, 4, -1] and (n, used) == (2, 8)
    st = C.component_stats(m["verts"], m["faces"])
    assert st["label"].tolist() == [0, 4] and st["n_faces"].tolist() == [2, 3] and st["n_verts"].tolist() == [4, 4]
    assert st["area"].tolist() == [1.0, 4.0]
    assert st["lo"].tolist() == [[0, 0, 0], [0, 0, 2]] and st["hi"].tolist() == [[1, 1, 0], [2, 2, 2]]
    assert st["vertex_comp"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, -1] and st["face_comp"].tolist() == [1, 0, 1, 0, 1, -1]
    big, _, kept = C.keep_components(m, "largest")
    assert kept.tolist() == [False, True]
    assert big["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [2, 2, 3]] and np.array_equal(big["verts"], m["verts"][4:8])
    assert np.array_equal(big["colors"], m["colors"][4:8])
    box = ([-0.5, -0.5, -0.5], [0.0, 0.0, 0.0])                       # the closed box holds vertex 0 only
    assert C.keep_components(m, "touching", box)[0]["faces"].tolist() == [[0, 1, 2], [0, 2, 3]]
    assert np.array_equal(C.keep_components(m, "not_touching", box)[0]["verts"], big["verts"])
    # sharing one vertex joins (the departure from trimesh's edge adjacency); a chain closes transitively
    vl, _, n, _ = C.components([[0, 1, 2], [2, 3, 4], [6, 7, 8], [8, 9, 4]], 11)
    assert n == 1 and vl.tolist() == [0] * 5 + [-1] + [0] * 4 + [-1]
    # non-finite coordinates: skipped by the box, the face that touches one has area 0
    v = m["verts"].copy()
    v[1, 0] = np.nan
    st = C.component_stats(v, m["faces"])
    assert st["area"].tolist() == [0.5, 4.0] and st["hi"][0].tolist() == [1, 1, 0] and st["lo"][0].tolist() == [0, 0, 0]
    assert C.component_stats(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32))["n_components"] == 0
    assert C._unord(C._ord(np.array([-0.0, 0.0, -1.5, np.inf], np.float32))).tolist() == [-0.0, 0.0, -1.5, np.inf]
    assert C._ord(np.float32(-0.0)) < C._ord(np.float32(0.0))


def test_oracle_agrees_with_scipy_on_the_adversarial_orders():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name, (f, V) in C.adversarial_cases(20000).items():
        vl, fl, n, used = C.components(f, V)
        ok = C.valid_faces(f, V)
        g = f[ok].astype(np.int64)
        rows, cols = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
        _, lab = connected_components(sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
        first = np.full(lab.max() + 1 if V else 0, V, np.int64)
        np.minimum.at(first, lab, np.arange(V))                         # canonical: the smallest index of each class
        ref = first[lab]
        refd = np.zeros(V, bool)
        refd[g.reshape(-1)] = True
        ref[~refd] = -1
        assert np.array_equal(vl, ref), name
        assert n == len(np.unique(ref[ref >= 0])) and used == refd.sum(), name


def test_umeyama_recovers_a_known_similarity():
    g = np.random.default_rng(3)
    src = g.normal(size=(500, 3))
    T = C.similarity([0.3, -1.0, 0.5], 37.0, [0.4, -0.2, 0.9], 1.7)
    got = C.umeyama(src, E.transform(src, T), with_scaling=True)
    assert np.abs(got - T).max() < 1e-12
    rigid = C.umeyama(src, E.transform(src, T), with_scaling=False)
    assert abs(np.linalg.det(rigid[:3, :3]) - 1.0) < 1e-12                # without the switch: a rotation, the scale is not absorbed
    assert np.abs(C.umeyama(src, src) - E.kabsch(src, src)).max() == 0.0


def test_kabsch_with_scaling_on_cpu_tensors_matches_oracle():
    from nicer_slam_amd.mesh_eval import _kabsch
    g = np.random.default_rng(4)
    src = g.normal(size=(800, 3))
    tgt = E.transform(src, C.similarity([1, 2, 3], 11.0, [0.1, 0.2, -0.3], 0.93)) + g.normal(0, 1e-3, (800, 3))
    for ws in (False, True):
        got = _kabsch(torch.from_numpy(src), torch.from_numpy(tgt), ws)
        assert np.abs(got - C.umeyama(src, tgt, ws)).max() < 1e-12
    with pytest.raises(ValueError):
        _kabsch(torch.zeros(5, 3, dtype=torch.float64), torch.from_numpy(tgt[:5]), True)


def test_select_faces_and_transform_mesh_on_cpu_match_oracle():
    from nicer_slam_amd import mesh_clean as M
    m = _two_quads()
    mask = np.array([1, 0, 1, 0, 0, 0], bool)
    ref = C.select_faces(m, mask)
    got = M.select_faces(m, mask)                                                                 # numpy in, numpy out
    tm = {k: torch.from_numpy(x) for k, x in m.items()}
    got_t = M.select_faces(tm, torch.from_numpy(mask))                                            # torch in, torch out
    for k in ("verts", "faces", "normals", "colors"):
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], ref[k]), k
        assert torch.is_tensor(got_t[k]) and np.array_equal(got_t[k].numpy(), ref[k]) and got_t[k].dtype == tm[k].dtype, k
    assert got["faces"].tolist() == [[0, 1, 2], [0, 2, 3]] and len(got["verts"]) == 4
    assert len(M.select_faces(m, np.zeros(6, bool))["verts"]) == 0
    g = np.random.default_rng(5)
    mesh = {"verts": g.normal(size=(300, 3)).astype(np.float32), "faces": g.integers(0, 300, (100, 3)).astype(np.int32),
            "normals": g.normal(size=(300, 3)).astype(np.float32)}
    mesh["normals"][7] = 0
    T = C.similarity([0.2, 0.4, -1.0], 37.0, [0.5, -1.5, 0.25], 1.7)
    ref, got = C.transform_mesh(mesh, T), M.transform_mesh(mesh, T)
    assert np.array_equal(got["verts"], ref["verts"]) and np.array_equal(got["faces"], mesh["faces"])
    assert np.abs(got["normals"] - ref["normals"]).max() < 1e-6 and (got["normals"][7] == 0).all()
    assert np.abs(np.linalg.norm(got["normals"][:7], axis=1) - 1).max() < 1e-6
    got_t = M.transform_mesh({k: torch.from_numpy(x) for k, x in mesh.items()}, torch.from_numpy(T))
    assert np.array_equal(got_t["verts"].numpy(), ref["verts"])


def test_value_errors():
    from nicer_slam_amd import mesh_clean as M
    m = _two_quads()
    T = C.similarity([0, 0, 1], 10.0, [0, 0, 0], 2.0)
    bad = [np.eye(3), np.diag([1.0, 1.0, -1.0, 1.0]), np.diag([1.0, 1.0, 1.001, 1.0]), np.zeros((4, 4)), T + np.eye(4)[[3, 3, 3, 0]] * 0.1]
    sheared = T.copy()
    sheared[0, 1] += 1e-4
    nan = T.copy()
    nan[0, 3] = np.nan
    for X in bad + [sheared, nan]:
        with pytest.raises(ValueError):
            M.transform_mesh(m, X)
    close = T.copy()
    close[:3, :3] *= 1 + 1e-9
    M.transform_mesh(m, close)                                          # within 1e-6: accepted
    with pytest.raises(ValueError):
        M.select_faces(m, np.ones(5, bool))
    with pytest.raises(ValueError):
        M.select_faces({"verts": m["verts"][:4], "faces": m["faces"]}, np.ones(6, bool))      # a kept index past V
    with pytest.raises(ValueError):
        M.select_faces({"verts": m["verts"]}, np.ones(6, bool))
    with pytest.raises(ValueError):
        M.keep_components(m, "smallest")
    with pytest.raises(ValueError):
        M.keep_components(m, "touching")                               # no region
    with pytest.raises(ValueError):
        M.keep_components(m, "not_touching", ([0, 0, 0], [1, -1, 1]))  # lo > hi
    with pytest.raises(ValueError):
        M.components(torch.zeros(4, 3, dtype=torch.int32), 4)          # not on the device
    with pytest.raises(ValueError):
        M.component_stats(torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int32))


def test_command_line_parsing():
    from nicer_slam_amd import mesh_clean as M
    a = M.parse_args(["in.ply", "--out", "out.ply"] + "--keep not_touching --region -1 -1 -1 -0.5 -0.5 -0.5 --transform T.npy".split())
    assert (a.mesh, a.out, a.keep, a.region, a.transform, a.list) == ("in.ply", "out.ply", "not_touching", [-1, -1, -1, -0.5, -0.5, -0.5],
                                                                     "T.npy", False)
    assert M.parse_args(["in.ply", "--list"]).list
    assert M.parse_args(["in.ply", "--out", "o.ply", "--keep", "largest"]).keep == "largest"
    for argv in (["in.ply"], ["in.ply", "--out", "o.ply"], ["in.ply", "--out", "o.ply", "--keep", "touching"],
                 ["in.ply", "--out", "o.ply", "--keep", "largest", "--region", "0", "0", "0", "1", "1", "1"],
                 ["in.ply", "--out", "o.ply", "--keep", "biggest"], ["in.ply", "--keep", "largest"]):
        with pytest.raises(SystemExit):
            M.parse_args(argv)


def test_command_line_reports_a_bad_file_cleanly(tmp_path, capsys):
    from nicer_slam_amd import mesh_clean as M
    (tmp_path / "bad.ply").write_bytes(b"not a ply")
    with pytest.raises(SystemExit) as e:
        M.main([str(tmp_path / "bad.ply"), "--out", str(tmp_path / "o.ply"), "--keep", "largest"])
    assert e.value.code == 2 and "mesh_clean:" in capsys.readouterr().err and not (tmp_path / "o.ply").exists()
    from nicer_slam_amd.inference import write_ply
    m = {k: torch.from_numpy(v) for k, v in _two_quads().items()}
    m["faces"] = m["faces"][:5]                                        # (read_ply rejects the face with an index past V)
    write_ply(tmp_path / "in.ply", m)
    np.save(tmp_path / "T.npy", np.diag([1.0, 2.0, 1.0, 1.0]))
    with pytest.raises(SystemExit):
        M.main([str(tmp_path / "in.ply"), "--out", str(tmp_path / "o.ply"), "--transform", str(tmp_path / "T.npy")])
    assert "multiple of a rotation" in capsys.readouterr().err
    np.save(tmp_path / "T.npy", C.similarity([0, 0, 1], 90.0, [1, 0, 0], 2.0))
    out = M.main([str(tmp_path / "in.ply"), "--out", str(tmp_path / "o.ply"), "--transform", str(tmp_path / "T.npy")])
    from nicer_slam_amd.inference import read_ply
    back = read_ply(tmp_path / "o.ply")
    assert np.array_equal(back["verts"], out["verts"]) and np.abs(back["verts"][1] - [1, 2, 0]).max() < 1e-6


def test_mesh_eval_command_line_accepts_the_new_switches(monkeypatch):
    from nicer_slam_amd import mesh_eval as M
    for argv in (["a.ply", "b.ply", "--clean", "touching"], ["a.ply", "b.ply", "--region", "0", "0", "0", "1", "1", "1"],
                 ["a.ply", "b.ply", "--clean", "largest", "--region", "0", "0", "0", "1", "1", "1"]):
        with pytest.raises(SystemExit):
            M.main(argv)


def test_argument_validation_needs_no_gpu():
    from nicer_slam_amd._native import lib
    NSA_EBADARG = 4
    fake = ctypes.c_void_p(4096)                                        # never dereferenced: rejected before any launch
    big = 1 << 31
    assert lib.nsa_mesh_components_workspace(1) > 0 and lib.nsa_mesh_components_workspace(354000) >= 4 * 354000
    assert lib.nsa_mesh_components_workspace(0) == 0 and lib.nsa_mesh_components_workspace(big) == 0
    assert lib.nsa_mesh_components(None, 0, 0, None, None, None, None, None) == 0                       # V = F = 0: a no-op
    assert lib.nsa_mesh_components(None, 5, 9, fake, fake, fake, fake, None) == NSA_EBADARG              # no faces
    assert lib.nsa_mesh_components(fake, 5, 9, None, fake, fake, fake, None) == NSA_EBADARG              # no workspace
    assert lib.nsa_mesh_components(fake, 5, 9, fake, None, fake, fake, None) == NSA_EBADARG              # no vertex_label
    assert lib.nsa_mesh_components(fake, 5, 9, fake, fake, None, fake, None) == NSA_EBADARG              # no face_label
    assert lib.nsa_mesh_components(fake, 5, 9, fake, fake, fake, None, None) == NSA_EBADARG              # no totals
    assert lib.nsa_mesh_components(fake, big, 9, fake, fake, fake, fake, None) == NSA_EBADARG            # F >= 2^31
    assert lib.nsa_mesh_components(fake, 5, big, fake, fake, fake, fake, None) == NSA_EBADARG            # V >= 2^31
    assert lib.nsa_mesh_component_stats_workspace(9, 5, 2) > 0 and lib.nsa_mesh_component_stats_workspace(9, 0, 0) > 0
    assert lib.nsa_mesh_component_stats_workspace(9, 5, 6) == 0 and lib.nsa_mesh_component_stats_workspace(0, 5, 1) == 0
    assert lib.nsa_mesh_component_stats_workspace(big, 5, 1) == 0
    stats = lib.nsa_mesh_component_stats
    assert stats(None, 0, None, 0, None, None, 0, None, None, None, None, None, None, None, None, None, None) == 0
    full = [fake, 9, fake, 5, fake, fake, 2, fake, fake, fake, fake, fake, fake, fake, fake, fake, None]
    for k in (0, 2, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15):                                              # each pointer NULL in turn
        args = list(full)
        args[k] = None
        assert stats(*args) == NSA_EBADARG, k
    for k, val in ((6, 6), (1, big), (3, big), (1, 0)):                                                  # C > F; counts; faces without vertices
        args = list(full)
        args[k] = val
        assert stats(*args) == NSA_EBADARG, (k, val)


@pytest.mark.parametrize("sanitize", [False, True])
def test_labelling_passes_on_host_threads(tmp_path, sanitize):
    """The device's pass bodies (csrc/uf_passes.hpp) as host C++ on 8 threads, adversarial orders, against a sequential
    union-find; once more under the thread sanitizer where the host compiler has it."""
    sanitize = "thread" if sanitize else None
    exe = host_program.build("uf_host_check.cpp", tmp_path, sanitize, flags=("-pthread",))
    run = host_program.run(exe, ["8", "20000" if sanitize else "100000"], 600, sanitize)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
