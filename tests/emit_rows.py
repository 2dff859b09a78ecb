"""From an emission buffer of the MAP kernels to PER-POINT weight gradients (test infrastructure): the float64, host-side mirror of
fused/mapping.py::sdf_flat_grad / colour_flat_grad WITHOUT the sum over the points.

The row maps are production's (mapping.se_rows, mapping.CE, mapping._sdf_rows, mapping._col_rows), not restated here; the formulas are
those of struct SE<NH> (csrc/render_sdfnet.hip):
    dW_0[p] = AB_1 (x) H0 + DA_1 (x) TIN,   dW_k[p] = AB_{k+1} (x) H_k + DA_{k+1} (x) TH_k  (0 < k < NH),   db_k[p] = AB_{k+1},
    dW_NH[p][0] = g_sdf[p] H_NH + TH_NH,   dW_NH[p][1:] = FB (x) H_NH,   db_NH[p] = [g_sdf[p], FB]
and of enum CE_* (csrc/render_colour.hip): dW_0[p] = AB1 (x) IN, dW_1[p] = AB2 (x) H1, dW_2[p] = OB (x) H2, db_l[p] = AB1 / AB2 / OB.
Every function returns, per layer, [P, out, in + 1] = the point's [dW_l | db_l] with the input features in the reference's order:
the layout of ref64.sdf_weight_grads / colour_weight_grads.  tests/test_gemm_float64_gpu.py ties the sum over the points to
sdf_flat_grad / colour_flat_grad on the same buffer.

Which regions depend on what (read off sdfnet_bwd_body.inc, sdfnet4_bwd_body.inc, colour_bwd_body.inc and the hidden_forward /
reverse_pass helpers they call):
  functions of the POINT alone: H0 (first-layer input), H_k (Softplus outputs), DA_k = sp'(a_k) dh_k (the reverse pass from the sdf
      row, which no cotangent enters); colour: IN, H1, H2;
  linear in g_grad alone:       TIN (the tangent of the first-layer input along nbar = g_grad), TH_k = sp'(a_k) ta_k;
  linear in all cotangents:     AB_k (total cotangent of a_k), FB (= g_feat); colour: AB1, AB2, OB (all linear in g_rgb)."""
import torch

from gate64 import fwd_norm, gate

F64 = torch.float64


def sdf_regions(NH, tile):
    """name -> (first row, rows, point_only?) of every region of an SDF emission buffer; H0 / TIN rows are first-layer slots"""
    from nicer_slam_amd.fused import mapping
    m = mapping.se_rows(NH, tile)
    out = {"H0": (m["H0"], m["IN"], True), "TIN": (m["TIN"], m["IN"], False), "FB": (m["FB"], 64, False)}
    for k in range(1, NH + 1):
        out[f"DA{k}"], out[f"H{k}"] = (m[f"DA{k}"], 64, True), (m[f"H{k}"], 64, True)
        out[f"TH{k}"], out[f"AB{k}"] = (m[f"TH{k}"], 64, False), (m[f"AB{k}"], 64, False)
    assert sum(n for _r, n, _p in out.values()) == m["ROWS"]
    return out


def colour_regions():
    from nicer_slam_amd.fused import mapping
    CE = mapping.CE
    out = {"IN": (CE["IN"], CE["H1"] - CE["IN"], True), "H1": (CE["H1"], 64, True), "H2": (CE["H2"], 64, True),
           "AB1": (CE["AB1"], 64, False), "AB2": (CE["AB2"], 64, False), "OB": (CE["OB"], 3, False)}
    assert sum(n for _r, n, _p in out.values()) == CE["ROWS"]
    return out


def _cols(emit, P, r0, n):
    """rows [r0, r0 + n) of the first P columns -> [P, n] float64 on the host"""
    return emit[r0:r0 + n, :P].detach().cpu().to(F64).t().contiguous()


def _outer(a, b):
    return a.unsqueeze(2) * b.unsqueeze(1)


def _with_bias(dw, db):
    return torch.cat((dw, db.unsqueeze(2)), dim=2)


def sdf_activations(emit, P, L, C, NH=1, tile=32):
    """-> [first-layer input [P, 39 + L C], h_1, .., h_NH [P, 64]]: the value-path regions H0, H_k in the reference's feature order"""
    from nicer_slam_amd.fused import mapping
    m = mapping.se_rows(NH, tile)
    feat = mapping._sdf_rows(L, C, tile)
    return [_cols(emit, P, m["H0"], m["IN"])[:, feat]] + [_cols(emit, P, m[f"H{k}"], 64) for k in range(1, NH + 1)]


def sdf_point_grads(emit, g_sdf, P, L, C, NH=1, tile=32, magnitude=False):
    """sdf_flat_grad per point.  g_sdf [P] or None: the per-point cotangent of the sdf value (column order = point order here).
    magnitude: every factor replaced by its absolute value (the sum over the points is then the sum |a b| of the products)."""
    from nicer_slam_amd.fused import mapping
    m = mapping.se_rows(NH, tile)
    feat = mapping._sdf_rows(L, C, tile)
    mag = torch.abs if magnitude else (lambda t: t)
    reg = lambda name, n=64: mag(_cols(emit, P, m[name], n))
    gs = torch.zeros(P, dtype=F64) if g_sdf is None else mag(g_sdf.detach().cpu().to(F64))
    h0, tin = reg("H0", m["IN"])[:, feat], reg("TIN", m["IN"])[:, feat]
    out = [_with_bias(_outer(reg("AB1"), h0) + _outer(reg("DA1"), tin), reg("AB1"))]
    for k in range(1, NH):
        ab = reg(f"AB{k + 1}")
        out.append(_with_bias(_outer(ab, reg(f"H{k}")) + _outer(reg(f"DA{k + 1}"), reg(f"TH{k}")), ab))
    h, fb = reg(f"H{NH}"), reg("FB")
    row0 = gs.unsqueeze(1) * h + reg(f"TH{NH}")
    out.append(_with_bias(torch.cat((row0.unsqueeze(1), _outer(fb, h)), dim=1), torch.cat((gs.unsqueeze(1), fb), dim=1)))
    return out


def colour_activations(emit, P):
    from nicer_slam_amd.fused import mapping
    CE = mapping.CE
    return [_cols(emit, P, CE["IN"], CE["H1"] - CE["IN"])[:, mapping._col_rows()], _cols(emit, P, CE["H1"], 64), _cols(emit, P, CE["H2"], 64)]


def colour_point_grads(emit, P, magnitude=False):
    """colour_flat_grad per point (magnitude: as sdf_point_grads)"""
    from nicer_slam_amd.fused import mapping
    CE = mapping.CE
    mag = torch.abs if magnitude else (lambda t: t)
    x0, h1, h2 = (mag(t) for t in colour_activations(emit, P))
    ab1, ab2, ob = (mag(_cols(emit, P, CE[k], n)) for k, n in (("AB1", 64), ("AB2", 64), ("OB", 3)))
    return [_with_bias(_outer(ab1, x0), ab1), _with_bias(_outer(ab2, h1), ab2), _with_bias(_outer(ob, h2), ob)]


def flat(rows):
    """per-layer [.., out, in + 1] -> the flat layout of pack.flat_params [W_0, b_0, W_1, b_1, .., 0] (leading dimensions kept)"""
    parts = []
    for r in rows:
        parts += [r[..., :-1].reshape(*r.shape[:-2], -1), r[..., -1]]
    return torch.cat(parts + [torch.zeros(*rows[0].shape[:-2], 1, dtype=rows[0].dtype)], dim=-1)


def gate_first_layer_input(what, got, refs, n_grid, keep, fails):
    """H0 / IN in two parts, each with fwd_norm of its own: the columns in front of the grid features (the point, the positional
    encoding, the inputs handed in: an fp32 evaluation errs only in sin and cos) and the grid features, whose float64 reference is
    the grid itself in float64 (in fp32 the interpolation weights of the fine levels cost orders of magnitude more than a sine: judged
    together, that error would hide one in the encoding)"""
    r, y = refs
    cut = r.shape[1] - n_grid
    assert got.shape == r.shape, (got.shape, r.shape)
    gate(what + " (in front of the grid features)", got[:, :cut], r[:, :cut], y[:, :cut], fwd_norm(r[:, :cut]), keep, failures=fails)
    gate(what + " (grid features)", got[:, cut:], r[:, cut:], y[:, cut:], fwd_norm(r[:, cut:]), keep, failures=fails)
