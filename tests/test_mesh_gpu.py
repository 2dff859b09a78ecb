"""Marching cubes on the device (csrc/mesh_extract.hip, inference.marching_cubes / extract_mesh) against the numpy oracle
tests/mc_ref.py, on analytic surfaces, and the vertex colours against the composed torch path of plots.py:137-147."""
import math

import numpy as np
import pytest
import torch

import mc_ref
from helpers import assert_close

pytestmark = pytest.mark.gpu


def _model():
    """tests/test_inference_gpu.py::_model"""
    from nicer_slam_amd.utils.conf import replica_model_conf
    from nicer_slam_amd.model.network import SLAMNetwork
    torch.manual_seed(4)
    m = SLAMNetwork(replica_model_conf(use_warp_loss=False)).cuda()
    with torch.no_grad():
        for enc in (m.implicit_network.coarse.encoding, m.implicit_network.fine.encoding, m.rendering_network.encoding):
            enc.embeddings.uniform_(-0.05, 0.05)
    return m.eval()


def _check_equal(got, ref, what):
    for k in ("verts", "normals", "faces"):
        assert tuple(got[k].shape) == ref[k].shape, (what, k, tuple(got[k].shape), ref[k].shape)
    assert got["faces"].dtype == torch.int32 and got["verts"].dtype == torch.float32
    np.testing.assert_array_equal(got["faces"].cpu().numpy(), ref["faces"], err_msg=f"{what}: faces")
    np.testing.assert_array_equal(got["verts"].cpu().numpy(), ref["verts"], err_msg=f"{what}: verts")
    np.testing.assert_allclose(got["normals"].cpu().numpy(), ref["normals"], rtol=0, atol=1e-6, err_msg=f"{what}: normals")


SPACING, ORIGIN = (0.5, 1.25, 2.0), (-1.0, 0.5, 3.0)


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 7), (33, 17, 65), (64, 64, 64)])
@pytest.mark.parametrize("level", [0.0, 0.3])
def test_marching_cubes_matches_oracle_on_noise(shape, level):
    """Uniform noise reaches every case, the ambiguous faces included."""
    from nicer_slam_amd.inference import marching_cubes
    g = np.random.default_rng(hash((shape, level)) % (1 << 32))
    vol = (g.random(shape, dtype=np.float32) * 2 - 1).astype(np.float32)
    got = marching_cubes(torch.from_numpy(vol).cuda(), level, SPACING, ORIGIN)
    ref = mc_ref.marching_cubes(vol, level, SPACING, ORIGIN)
    if shape == (64, 64, 64):
        assert ref["faces"].shape[0] > 100000
    _check_equal(got, ref, f"noise {shape} level {level}")


def test_marching_cubes_samples_at_the_level_and_nonfinite():
    from nicer_slam_amd.inference import marching_cubes
    g = np.random.default_rng(7)
    q = g.integers(-1, 2, (40, 33, 29)).astype(np.float32)                      # samples exactly at the level 0
    _check_equal(marching_cubes(torch.from_numpy(q).cuda(), 0.0, SPACING, ORIGIN), mc_ref.marching_cubes(q, 0.0, SPACING, ORIGIN),
                 "quantised")
    v = (g.random((37, 41, 45), dtype=np.float32) * 2 - 1).astype(np.float32)
    pick = g.random(v.shape)
    v[pick < 0.02] = np.nan
    v[(pick >= 0.02) & (pick < 0.03)] = np.inf
    v[(pick >= 0.03) & (pick < 0.04)] = -np.inf
    ref = mc_ref.marching_cubes(v, 0.1, SPACING, ORIGIN)
    _check_equal(marching_cubes(torch.from_numpy(v).cuda(), 0.1, SPACING, ORIGIN), ref, "non-finite")
    assert np.setdiff1d(np.arange(ref["verts"].shape[0]), ref["faces"]).size > 0   # unreferenced vertices exist


def _closed_and_euler(faces, n_verts):
    f = faces.long()
    d = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * n_verts + d[:, 1]
    rev = d[:, 1] * n_verts + d[:, 0]
    s, _ = torch.sort(key)
    once = bool((s[1:] != s[:-1]).all())
    pos = torch.searchsorted(s, rev).clamp(max=s.numel() - 1)
    paired = bool((s[pos] == rev).all())
    used = torch.unique(f).numel()
    return once and paired, used - key.numel() // 2 + f.shape[0]


def test_sphere_512_closed_outward_and_its_volume():
    from nicer_slam_amd.inference import marching_cubes
    n, r = 512, 0.5
    ax = torch.linspace(-1, 1, n, dtype=torch.float64, device="cuda").float()
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.sqrt(x * x + y * y + z * z) - r
    del x, y, z
    step = 2.0 / (n - 1)
    m = marching_cubes(vol, 0.0, (step,) * 3, (-1.0,) * 3)
    del vol
    V, F = m["verts"].shape[0], m["faces"].shape[0]
    assert F > 100000
    closed, chi = _closed_and_euler(m["faces"], V)
    assert closed and chi == 2
    v = m["verts"].double()
    f = m["faces"].long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = torch.cross(b - a, c - a, dim=1)
    assert bool(((nrm * (a + b + c)).sum(1) > 0).all())                         # every face away from the centre
    vol_enc = float((a * torch.cross(b, c, dim=1)).sum() / 6)
    exact = 4 / 3 * math.pi * r ** 3
    assert abs(vol_enc - exact) / exact < 1e-3, (vol_enc, exact)
    assert bool(((m["normals"].double() * v).sum(1) > 0).all())


def test_empty_surface_gives_empty_tensors():
    from nicer_slam_amd.inference import marching_cubes, extract_mesh
    out = marching_cubes(torch.ones(9, 8, 7, device="cuda"), 0.0)
    assert out["verts"].shape == (0, 3) and out["normals"].shape == (0, 3) and out["faces"].shape == (0, 3)
    assert out["faces"].dtype == torch.int32 and out["verts"].is_cuda
    out = marching_cubes(torch.zeros(1, 8, 7, device="cuda"), 0.5)
    assert out["verts"].shape == (0, 3) and out["faces"].shape == (0, 3)
    m = _model()
    mesh = extract_mesh(m, 16, (-1.0, 1.0), level=50.0)
    assert mesh["verts"].shape == (0, 3) and mesh["faces"].shape == (0, 3) and mesh["colors"].shape == (0, 3)


def test_extract_mesh_equals_sdf_grid_then_marching_cubes_and_colours_match_composed():
    from nicer_slam_amd import inference
    m = _model()
    res, bound = 96, (-1.0, 1.0)
    mesh = inference.extract_mesh(m, res, bound, chunk=1 << 18)
    assert mesh["faces"].shape[0] > 1000
    vol = inference.sdf_grid(m, res, bound, chunk=1 << 18)
    ax = torch.linspace(bound[0], bound[1], res, dtype=torch.float64)          # get_grid_uniform's axis
    step = float(ax[1] - ax[0])
    ref = inference.marching_cubes(vol, 0.0, (step,) * 3, (bound[0],) * 3)
    for k in ("verts", "normals", "faces"):
        assert torch.equal(mesh[k], ref[k]), k
    v, nrm = mesh["verts"], mesh["normals"]
    sdf, feat, grad = m.implicit_network.get_outputs(v.clone(), stage="fine")          # plots.py:137-147
    with torch.no_grad():
        rgb = m.rendering_network(v, grad.detach(), -nrm, feat.detach(), indices=None, color_stage="highfreq")
    assert_close(mesh["colors"], rgb, 2e-5, 1e-4, "vertex colours")
    # ragged colour chunks give the same colours
    again = inference.vertex_colours(m, v, nrm, chunk=777)
    assert torch.equal(again, mesh["colors"])


def test_two_calls_are_bit_identical():
    from nicer_slam_amd import inference
    g = torch.Generator().manual_seed(3)
    vol = (torch.rand(70, 66, 130, generator=g) * 2 - 1).cuda()
    a = inference.marching_cubes(vol, 0.1, SPACING, ORIGIN)
    b = inference.marching_cubes(vol, 0.1, SPACING, ORIGIN)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    m = _model()
    x = inference.extract_mesh(m, 48, (-1.0, 1.0))
    y = inference.extract_mesh(m, 48, (-1.0, 1.0))
    for k in ("verts", "normals", "faces", "colors"):
        assert torch.equal(x[k], y[k]), k


def test_write_ply_of_an_extracted_mesh(tmp_path):
    from nicer_slam_amd import inference
    mesh = inference.extract_mesh(_model(), 32, (-1.0, 1.0))
    p = tmp_path / "surface.ply"
    inference.write_ply(str(p), mesh)
    V, F = mesh["verts"].shape[0], mesh["faces"].shape[0]
    assert p.stat().st_size > 27 * V + 13 * F
