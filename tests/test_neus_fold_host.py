"""The fold of the SDF feature layer into the first colour layer (csrc/neus_fold.hip), stated in numpy float64 on the full-size
networks (oracle.geo.FULL_CFG: weight norm, skip layer, geometric init).

    feat   = W8f . h7 + b8f                                (the last SDF layer's rows 1.., no activation: fields.py:84-91)
    c0_pre = Wc0 . [pts, view, normal, feat] + bc0         (fields.py:147-166)
           = (Wfold . h7 + bfold) + Wc0[:, extras] . extras,   Wfold = Wc0[:, feat] . W8f,  bfold = bc0 + Wc0[:, feat] . b8f

`fold_reference` is the float64 statement the GPU test (tests/test_gpu_neus_fold.py) holds the device-built buffer to; the test
here checks the algebra -- bias term, feature column range, the skip layer's 1/sqrt(2) entering through h7 only -- with no GPU."""
import math

import numpy as np

from oracle import geo as og
from vqnerf_release_amd.geo import packing


def effective_weights64(params, n_lin):
    """[(W_l, b_l)] float64 from an oracle parameter dict (weight norm applied: g v / ||v||_row)."""
    out = []
    for l in range(n_lin):
        g, v = np.asarray(params[f'lin{l}.weight_g'], np.float64), np.asarray(params[f'lin{l}.weight_v'], np.float64)
        out.append((g * v / np.linalg.norm(v, axis=1, keepdims=True), np.asarray(params[f'lin{l}.bias'], np.float64)))
    return out


def fold64(w8, b8, wc0, bc0, extra):
    """(Wfold [C, H], bfold [C]) in float64 from the last SDF layer (w8 [1 + F, H], b8) and the first colour layer (wc0 [C, extra + F], bc0)."""
    w8, b8, wc0, bc0 = [np.asarray(a, np.float64) for a in (w8, b8, wc0, bc0)]
    return wc0[:, extra:] @ w8[1:], bc0 + wc0[:, extra:] @ b8[1:]


def fold_reference(w8, b8, wc0, bc0, extra):
    """The three appended blocks of the folded colour buffer as float64 arrays in pack order (zero where padded):
    (Wfold forward pack, bfold bias pack, Wc0[:, extras] forward pack).  Inputs: the f32 effective weights."""
    wf, bf = fold64(w8, b8, wc0, bc0, extra)
    C, H = wf.shape
    take = lambda m, ix: np.concatenate([np.asarray(m, np.float64).reshape(-1), [0.0]])[ix].reshape(-1)
    hid_rows = 4 * ((H + 31) // 32)
    blk_w = take(wf, packing.F32.gemm_index(C, H, [(hid_rows, H, 0)]))
    blk_b = take(bf, packing.F32.bias_index(C))
    blk_e = take(wc0, packing.F32.gemm_index(C, wc0.shape[1], [(packing.F32.rows_for(extra), extra, 0)]))
    return blk_w, blk_b, blk_e


def _h7_and_extras(cfg, sdf_w, n_pts, seed):
    """float64 last-hidden activations of the SDF net at random points, and random colour-net extras"""
    rng = np.random.default_rng(seed)
    c = cfg['sdf']
    x = rng.uniform(-1.2, 1.2, (n_pts, 3)) * c['scale']
    emb = [x]
    for k in range(c['multires']):
        emb += [np.sin(x * 2.0 ** k), np.cos(x * 2.0 ** k)]
    emb = np.concatenate(emb, 1)
    h = emb
    for l in range(len(sdf_w) - 1):
        if l in c['skip_in']:
            h = np.concatenate([h, emb], 1) / math.sqrt(2)
        t = h @ sdf_w[l][0].T + sdf_w[l][1]
        h = np.where(100.0 * t > 20.0, t, np.log1p(np.exp(np.minimum(100.0 * t, 20.0))) / 100.0)
    return h, rng


def test_folded_first_colour_layer_equals_the_unfolded_one_in_float64():
    cfg = og.FULL_CFG
    sdf_w = effective_weights64(og.make_sdf_params(cfg, 0), len(og.sdf_dims(cfg)) - 1)
    col_w = effective_weights64(og.make_color_params(cfg, 1), len(og.color_dims(cfg)) - 1)
    assert any(0 < s < len(sdf_w) - 1 for s in cfg['sdf']['skip_in'])              # the shapes the issue names: a skip layer ...
    (w8, b8), (wc0, bc0) = sdf_w[-1], col_w[0]
    F = w8.shape[0] - 1
    extra = wc0.shape[1] - F
    assert F == cfg['color']['d_feature'] and extra == 3 + (3 + 6 * cfg['color']['multires_view']) + 3      # idr: pts, view, normal
    h7, rng = _h7_and_extras(cfg, sdf_w, 257, 5)
    assert h7.shape[1] == w8.shape[1]
    extras = rng.normal(size=(h7.shape[0], extra))
    feat = h7 @ w8[1:].T + b8[1:]
    want = np.concatenate([extras, feat], 1) @ wc0.T + bc0
    wf, bf = fold64(w8, b8, wc0, bc0, extra)
    got = (h7 @ wf.T + bf) + extras @ wc0[:, :extra].T
    scale = np.abs(want).max()
    assert scale > 1e-3
    assert np.abs(got - want).max() <= 1e-12 * scale
    # a wrong feature column range or a dropped bias term is far outside that
    bad = (h7 @ (wc0[:, :F] @ w8[1:]).T + bf) + extras @ wc0[:, :extra].T
    assert np.abs(bad - want).max() > 1e-6 * scale
    assert np.abs((got - wc0[:, extra:] @ b8[1:]) - want).max() > 1e-9 * scale


def test_reference_blocks_have_the_pack_layout():
    """fold_reference's blocks: element (tile, K row, lane, j) of the forward pack is M[32 ot + phi(lane & 31)][feature(row, j, lane >> 5)]"""
    rng = np.random.default_rng(0)
    F, H, C, extra = 40, 70, 50, 33
    w8, b8 = rng.normal(size=(1 + F, H)).astype(np.float32), rng.normal(size=1 + F).astype(np.float32)
    wc0, bc0 = rng.normal(size=(C, extra + F)).astype(np.float32), rng.normal(size=C).astype(np.float32)
    blk_w, blk_b, blk_e = fold_reference(w8, b8, wc0, bc0, extra)
    wf, bf = fold64(w8, b8, wc0, bc0, extra)
    nt, hid_rows, er = 2, 12, packing.F32.rows_for(extra)
    assert blk_w.shape == (nt * hid_rows * 256,) and blk_b.shape == (nt * 32,) and blk_e.shape == (nt * er * 256,)
    W = blk_w.reshape(nt, hid_rows, 64, 4)
    E = blk_e.reshape(nt, er, 64, 4)
    for ot, r, lane, j in [(0, 0, 0, 0), (1, 5, 37, 2), (1, 11, 63, 3), (0, 8, 13, 1)]:
        row, f = 32 * ot + int(packing.PHI[lane & 31]), 32 * (r >> 2) + 2 * (4 * (r & 3) + j) + (lane >> 5)
        assert W[ot, r, lane, j] == (wf[row, f] if row < C and f < H else 0.0)
        if r < er:
            assert E[ot, r, lane, j] == (wc0[row, f] if row < C and f < extra else 0.0)
    B = blk_b.reshape(nt, 2, 16)
    assert B[1, 1, 3] == bf[32 + 2 * 3 + 1] and B[1, 0, 15] == 0.0
