"""CPU: the layer programs + weight packs of vqnerf_release_amd/decomp/packing.py, executed by a numpy emulator
of csrc/mlp_chain.hip's data movement (activation image, A-fragment packs, MFMA 32x32x2 operand maps: tests/chain_model.py),
reproduce the oracle's Dense stacks.  This pins the host logic (row allocation, gather indices, descriptor fields) without a GPU."""
import numpy as np
import pytest
import torch

from oracle import decomp as od
from tests.chain_model import _split, emulate, emulate_f16s, step_feat
from vqnerf_release_amd.decomp import packing as pk


def _params(names, p):
    out = {}
    for n in names:
        for i, (W, b) in enumerate(p[n]):
            out[f'{n}/{i}'] = (torch.tensor(W), torch.tensor(b))
    return out


def test_encoder_program_matches_oracle():
    p, specs = od.make_model_params(seed=3, K=15)
    fe, bn = specs['fine_enc'], specs['bottleneck']
    b = pk.ChainBuilder('posenc', 63, n_freqs=10)
    y = b.mlp('fine_enc', fe['widths'], fe['act'], fe['skip_at'], b.input)
    b.mlp('bottleneck', bn['widths'], bn['act'], bn['skip_at'], y, out_slot=0, small_last=False)
    plan = b.build()
    assert plan.macs_per_point() == 179968
    assert plan.n_waves == 4 and plan.total_rows <= 72
    wbuf, desc = plan.pack(_params(['fine_enc', 'bottleneck'], p))
    xyz = od.make_points(20, seed=5)['xyz']
    got = emulate(desc, wbuf.numpy(), xyz, [256])[0]
    pt = {k: [(torch.tensor(W, dtype=torch.float64), torch.tensor(bb, dtype=torch.float64)) for W, bb in v]
          for k, v in p.items() if isinstance(v, list)}
    want = od.pred_enc(pt, specs, torch.tensor(xyz, dtype=torch.float64)).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_three_heads_share_the_input_rows():
    p, specs = od.make_model_params(seed=4, K=15)
    for fam, widths in (('main', [3, 1, 1]), ('vq', [3, 3, 1])):
        names = [h + '_' + fam for h in ('diff', 'spec', 'rough')]
        b = pk.ChainBuilder('raw', 256)
        for slot, n in enumerate(names):
            s = specs[n]
            b.mlp(n, s['widths'], s['act'], s['skip_at'], b.input, keep=[b.input], out_slot=slot)
        plan = b.build()
        assert plan.macs_per_point() == (296832 if fam == 'main' else 297600)
        assert plan.total_rows * 1024 + 4096 <= 160 * 1024
        wbuf, desc = plan.pack(_params(names, p))
        z = np.random.default_rng(0).uniform(0, 1, (32, 256)).astype(np.float32)
        got = emulate(desc, wbuf.numpy(), z, widths)
        for g, n in zip(got, names):
            pt = [(torch.tensor(W, dtype=torch.float64), torch.tensor(bb, dtype=torch.float64)) for W, bb in p[n]]
            want = od.mlp_forward(pt, specs[n], torch.tensor(z, dtype=torch.float64)).numpy()
            np.testing.assert_allclose(g, want, rtol=0, atol=1e-9)


def test_regions_never_overlap_live_data():
    b = pk.ChainBuilder('raw', 256)
    x = b.input
    y0 = b.dense('a/0', [x], 256, 'relu', keep=[x])
    y1 = b.dense('a/1', [y0], 128, 'relu', keep=[x])
    y2 = b.dense('a/2', [y1, x], 64, 'relu')                   # y0 is dead here: its rows may be reused
    plan = b.build()
    disjoint = lambda a, c: a.row0 >= c.row0 + c.alloc_rows or a.row0 + a.alloc_rows <= c.row0
    assert disjoint(y0, x) and disjoint(y1, x) and disjoint(y1, y0) and disjoint(y2, y1) and disjoint(y2, x)
    assert plan.total_rows == 32 + 32 + 16                       # y2 fits into y0's rows


# ------------------------------------------------------------------ split-precision (f16 hi/lo) programs
def test_split_precision_programs_match_oracle():
    p, specs = od.make_model_params(seed=3, K=15)
    fe, bn = specs['fine_enc'], specs['bottleneck']
    b = pk.ChainBuilder('posenc', 63, n_freqs=10, mode='f16s')
    y = b.mlp('fine_enc', fe['widths'], fe['act'], fe['skip_at'], b.input)
    b.mlp('bottleneck', bn['widths'], bn['act'], bn['skip_at'], y, out_slot=0, small_last=False)
    plan = b.build()
    assert plan.macs_per_point() == 179968 and plan.total_rows <= 72
    wbuf, desc = plan.pack(_params(['fine_enc', 'bottleneck'], p))
    xyz = od.make_points(20, seed=5)['xyz']
    got = emulate_f16s(desc, wbuf.numpy(), xyz, [256])[0]
    pt = {k: [(torch.tensor(W, dtype=torch.float64), torch.tensor(bb, dtype=torch.float64)) for W, bb in v]
          for k, v in p.items() if isinstance(v, list)}
    want = od.pred_enc(pt, specs, torch.tensor(xyz, dtype=torch.float64)).numpy()
    # hi + lo carries ~22 bits, the lo*lo products are dropped: ~1e-6 of the layer's magnitude, not bitwise
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-6 * np.abs(want).max())
    assert np.abs(got - want).max() > 0                              # (and it is not the f32 path in disguise)

    names = ['diff_vq', 'spec_vq', 'rough_vq']
    b = pk.ChainBuilder('raw', 256, mode='f16s')
    for slot, n in enumerate(names):
        s = specs[n]
        b.mlp(n, s['widths'], s['act'], s['skip_at'], b.input, keep=[b.input], out_slot=slot)
    plan = b.build()
    wbuf, desc = plan.pack(_params(names, p))
    z = np.random.default_rng(0).uniform(0, 1, (32, 256)).astype(np.float32)
    got = emulate_f16s(desc, wbuf.numpy(), z, [3, 3, 1])
    for g, n in zip(got, names):
        ptn = [(torch.tensor(W, dtype=torch.float64), torch.tensor(bb, dtype=torch.float64)) for W, bb in p[n]]
        want = od.mlp_forward(ptn, specs[n], torch.tensor(z, dtype=torch.float64)).numpy()
        np.testing.assert_allclose(g, want, rtol=0, atol=3e-6 * max(1.0, np.abs(want).max()))
    with pytest.raises(ValueError):
        pk.LAYOUTS['f16s'].split(torch.full((1, 1, 64, 8), 7.0e4))


# ------------------------------------------------------------------ NeuS pack plans in split-precision mode
def test_sdf_pack_plan_f16s_forward_matches_oracle():
    """SdfPackPlan(mode='f16s'): the forward packs (f16 hi/lo A fragments in whole 64-feature blocks, register-order biases, the
    skip layer's two K segments, the sdf row image) run through a numpy model of csrc/neus_mlp_f16s.hip's forward reproduce
    oracle.geo.sdf_only to the split-precision tolerance."""
    from oracle import geo as og
    from vqnerf_release_amd.geo import packing as gp
    cfg = og.SMALL_CFG
    c = cfg['sdf']
    plan = gp.SdfPackPlan(og.sdf_dims(cfg), c['skip_in'], c['multires'], c['scale'], mode='f16s')
    p = og.to_torch(og.make_sdf_params(cfg, 0))
    W = [og.wn_weight(p, l) for l in range(plan.n_lin)]
    b = [p[f'lin{l}.bias'] for l in range(plan.n_lin)]
    wbuf, desc = plan.pack(W, b)
    wb = np.ascontiguousarray(wbuf.numpy())
    w16 = wb.view(np.float16).astype(np.float64).reshape(-1, 8)
    w4 = wb.astype(np.float64).reshape(-1, 4)
    n_lin, skip, multires, emb, emb_rows = [int(v) for v in desc[:5]]
    assert emb_rows % 2 == 0 and emb_rows == 2 * ((emb + 15) // 16)
    P = 20
    pts = np.random.default_rng(2).uniform(-1, 1, (P, 3))
    E = od.posenc(torch.tensor(pts * c['scale'], dtype=torch.float64), multires).numpy()          # [P, emb]

    def image(feats, n_rows):
        """[n_steps, part, h, n, jj] halves of a region holding `feats` [P, F]."""
        ns = n_rows // 2
        out = np.zeros((ns, 2, 2, 32, 8))
        for sl in range(ns):
            for h in range(2):
                for jj in range(8):
                    f = step_feat(sl, h, jj)
                    if f < feats.shape[1]:
                        hi, lo = _split(feats[:, f])
                        out[sl, 0, h, :P, jj], out[sl, 1, h, :P, jj] = hi, lo
        return out

    emb_img = image(E, emb_rows)
    cur = None
    for l in range(n_lin - 1):
        tiles, _, _, w_off, b_off = [int(v) for v in desc[12 + 8 * l: 12 + 8 * l + 5]]
        B = emb_img if l == 0 else (np.concatenate([cur, emb_img], 0) if l == skip else cur)
        ns = B.shape[0]
        nbr = 8 * ((2 * ns + 7) // 8)                                                            # pack rows per tile: whole blocks
        out = np.zeros((P, 32 * tiles))
        for ot in range(tiles):
            A = w16[w_off + ot * nbr * 64: w_off + (ot + 1) * nbr * 64].reshape(nbr // 2, 2, 2, 32, 8)
            assert not A[ns:].any()
            A = A[:ns]
            acc = np.einsum('shij,shnj->in', A[:, 0], B[:, 0]) + (np.einsum('shij,shnj->in', A[:, 0], B[:, 1]) +
                                                                 np.einsum('shij,shnj->in', A[:, 1], B[:, 0])) / 2048.0
            bias = w4[b_off + ot * 8: b_off + (ot + 1) * 8].reshape(2, 16)
            for h in range(2):
                for reg in range(16):
                    i = (reg & 3) + 8 * (reg >> 2) + 4 * h
                    x = acc[i, :P] + bias[h, reg]
                    out[:, 32 * ot + i] = np.where(100 * x > 20, x, np.log1p(np.exp(np.minimum(100 * x, 50))) / 100)
        cur = image(out[:, :32 * tiles], 4 * tiles)
    # sdf row: f32 image [1][n_steps][2][8]
    last_w = int(desc[7])
    ns = cur.shape[0]
    img = w4[last_w: last_w + ns * 4].reshape(ns, 2, 8)
    X = cur[:, 0] + cur[:, 1] / 2048.0                                                           # [step, h, n, jj]
    sdf = np.einsum('shj,shnj->n', img, X)[:P] + float(w4[int(desc[9])][0])
    with torch.no_grad():
        want = og.sdf_only({k: v.double() for k, v in p.items()}, cfg, torch.tensor(pts, dtype=torch.float64))[:, 0].numpy()
    np.testing.assert_allclose(sdf / c['scale'], want, rtol=0, atol=5e-6)
