"""The conditions tests/test_gpu_loss_kernels.py rests on, checked from the references alone (no GPU): every reference is finite,
float32 and float64 sit on the same side of every kink with a margin of at least 1e-5 (relative to eps where the kink is an eps
clamp), the closest pair of every code-separation case is separated from its runner-up, the known-answer ties are what they claim,
and no row of any case is left out of a comparison."""
import numpy as np
import pytest
import torch

from tests import loss_kernel_cases as lc

F32, F64 = torch.float32, torch.float64
BIG_N = 2 * 4 * 16 * lc.MI355X_CUS + 3


def _finite(tree):
    if isinstance(tree, dict):
        return all(_finite(v) for v in tree.values())
    if isinstance(tree, (list, tuple)):
        return all(_finite(v) for v in tree)
    if tree is None or isinstance(tree, (int, str)):
        return True
    return bool(np.isfinite(np.asarray(tree, np.float64)).all())


def _loss_conditions(N, D):
    """-> (pairs under the threshold, pairs over it, rough under 0.5, rough over, targets under the knee, over) of one case"""
    inp = lc.loss_inputs(N, D)
    gt, rough, spec = (inp[k].astype(np.float64) for k in ('rgb_gt', 'rough', 'spec'))
    assert (np.abs(gt - lc.SRGB_KNEE) >= lc.MARGIN).all() and (np.abs(rough - 0.5) >= lc.MARGIN).all()
    gap = lc.spec_gap(inp['spec'])
    ties = [inp['tie3']] + list(inp['tie2'])
    assert (gap[ties] == 0.0).all() and (np.delete(gap, ties) >= lc.MARGIN).all()
    assert (spec[inp['tie3']] == spec[inp['tie3'], 0]).all()
    for n_, r in enumerate(inp['tie2']):
        assert int(np.argmax(spec[r])) == (1, 0)[n_] and (spec[r] == spec[r].max()).sum() == 2
    assert not inp['vq_rgb'][inp['zero_rows']].any() and (np.abs(inp['vq_rgb'][~inp['zero_rows']]).sum(-1) > 0).all()
    under = over = 0
    if N >= 2:
        e32, e64 = lc.loss_pair_distance(inp, F32).astype(np.float64), lc.loss_pair_distance(inp, F64)
        assert (np.abs(e64 - lc.W['thres']) >= lc.MARGIN).all() and (np.abs(e32 - lc.W['thres']) >= lc.MARGIN).all()
        np.testing.assert_array_equal(e32 > lc.W['thres'], e64 > lc.W['thres'])
        np.testing.assert_allclose(e64, lc.pair_distance(inp['rgb_gt']), rtol=0, atol=1e-12)
        under, over = int((e64 < lc.W['thres']).sum()), int((e64 > lc.W['thres']).sum())
    for nerf in (True, False):
        r64, r32 = lc.loss_reference(inp, nerf, F64), lc.loss_reference(inp, nerf, F32)
        assert _finite(r64) and _finite(r32), (N, D, nerf)
        assert all(r64[k].shape[0] == N for k in r64)                      # the share of omitted rows is 0
        # the statement's own conventions, seen in the reference: first maximum only, nothing for a lone last point
        am = np.argmax(inp['spec'], -1)
        assert not np.delete(r64['g_spec'].reshape(-1), np.arange(N) * 3 + am).any()
        if N % 2:
            assert not r64['terms'][N - 1, 3] and not r64['g_z'][N - 1].any()
    return under, over, int((rough < 0.5).sum()), int((rough > 0.5).sum()), int((gt < lc.SRGB_KNEE).sum()), int((gt > lc.SRGB_KNEE).sum())


@pytest.mark.parametrize('D', lc.LOSS_D)
def test_loss_cases_hold_their_margins(D):
    for N in lc.LOSS_N:
        sides = _loss_conditions(N, D)
        if N >= 9:
            assert all(s > 0 for s in sides), (N, D, sides)               # both sides of every kink in one and the same case


def test_loss_grid_cap_case_and_variants():
    sides = _loss_conditions(BIG_N, 64)
    assert all(s > 100 for s in sides)
    inp = lc.loss_inputs(9, 64)
    full = lc.loss_reference(inp, True, F64)
    no_z, no_spec = lc.loss_reference(inp, True, F64, use_z=False), lc.loss_reference(inp, True, F64, use_spec=False)
    w0s, w0l = lc.loss_reference(inp, True, F64, w=dict(lc.W, smooth=0.0)), lc.loss_reference(inp, True, F64, w=dict(lc.W, lambert=0.0))
    assert no_z['g_z'] is None and no_spec['g_spec'] is None and not w0s['g_z'].any() and not w0l['g_spec'].any()
    for r, col in ((no_z, 3), (w0s, 3), (no_spec, 4), (w0l, 4)):
        assert not r['terms'][:, col].any() and full['terms'][:, col].any()
        keep = [c for c in range(5) if c != col]
        np.testing.assert_array_equal(r['terms'][:, keep], full['terms'][:, keep])
        np.testing.assert_array_equal(r['g_vq'], full['g_vq'])
    # the adjoints tell the five upstream columns apart: swapping two of them moves g_vq
    swapped = dict(inp, g_terms=inp['g_terms'][:, [0, 2, 1, 3, 4]].copy())
    r32 = lc.loss_reference(inp, True, F32)
    assert not lc.yardstick(lc.loss_reference(swapped, True, F32)['g_vq'], r32['g_vq'], full['g_vq'])['ok']
    assert lc.yardstick(r32['g_vq'], r32['g_vq'], full['g_vq'])['ok']


@pytest.mark.parametrize('D,K', lc.SIM_CASES + (lc.SIM_UNALIGNED,))
def test_sim_cases_have_a_separated_minimum(D, K):
    cb = lc.sim_inputs(D, K)
    r64, r32 = lc.sim_reference(cb, F64), lc.sim_reference(cb, F32)
    assert all(_finite(r[k]) for r in (r64, r32) for k in ('term', 'dist', 'g_cb'))
    assert r64['pair'] == r32['pair'] == ((K // 3, K - 1) if K > 2 else (0, 1))
    assert r64['gap'] > 1e-4 and r32['gap'] > 1e-4
    cols = list(r64['pair'])
    assert not np.delete(r64['g_cb'], cols, axis=1).any() and r64['g_cb'][:, cols].any(0).all()
    np.testing.assert_array_equal(r64['g_cb'][:, cols[0]], -r64['g_cb'][:, cols[1]])


@pytest.mark.parametrize('same_thread', [True, False])
def test_sim_tie_cases_are_exact_ties(same_thread):
    cb, q, pairs, want = lc.sim_tie_case(same_thread)
    K = q.shape[1]
    np.testing.assert_array_equal(cb.astype(np.float64) * 64, q)
    d2 = ((q[:, :, None] - q[:, None, :]) ** 2).sum(0)                       # integers: 4096 x the squared distances
    iu = np.triu_indices(K, 1)
    assert sorted(zip(*[a[d2[iu] == 1].tolist() for a in iu])) == sorted(pairs) and (d2[iu] >= 1).all()
    assert d2.max() < 8 * 4096
    flat = [i * K + j for i, j in pairs]
    assert (flat[0] % 256 == flat[1] % 256) == same_thread
    if not same_thread:                                                      # the smaller pair index belongs to the later thread
        assert min(flat) % 256 > max(flat) % 256
    assert want == pairs[int(np.argmin(flat))]
    r = lc.sim_reference(cb, F32)
    assert r['pair'] == want and float(r['dist'][0]) == 1.0 / 64.0


@pytest.mark.parametrize('D', lc.PREP_D)
def test_prep_cases_hold_their_margins(D):
    clamped = 0
    for K in lc.PREP_K:
        raw, gy = lc.prep_inputs(D, K)
        (cb64, g64, s64), (cb32, g32, s32) = lc.prep_reference(raw, gy, F64), lc.prep_reference(raw, gy, F32)
        assert _finite([cb64, g64, cb32, g32])
        assert (np.abs(s64 / lc.PREP_EPS - 1.0) >= 1e-3).all()
        np.testing.assert_array_equal(s32 > lc.PREP_EPS, s64 > lc.PREP_EPS)
        clamped += int((s64 < lc.PREP_EPS).sum())
        assert D == 1 or K == 1 or ((raw < 0).any() and (raw > 1).any())
        # the identity-gradient clip has get_codebook's values (whose eps is the double 1e-6, the kernel's the float32: 2e-9 apart)
        np.testing.assert_allclose(cb64, lc.od.get_codebook(torch.tensor(raw, dtype=F64)).numpy(), rtol=2e-9, atol=0)
    assert clamped >= 2


@pytest.mark.parametrize('K', lc.EMA_K)
def test_ema_cases(K):
    for D in lc.EMA_D:
        inp = lc.ema_inputs(K, D)
        r64, r32 = lc.ema_reference(inp, F64), lc.ema_reference(inp, F32)
        assert _finite(r64) and _finite(r32)
        hid = lc.ema_hidden_f32(inp)
        for c, (a, b) in enumerate(zip(r64, r32)):
            assert a['counter'] == b['counter'] == c + 1
            unused = inp['calls'][c]['counts'] == 0
            assert unused.any() == (c == 2)
            np.testing.assert_array_equal(a['update'][:, unused], inp['cb'][:, unused].astype(np.float64))
            # the float32 torch statement and the numpy float32 statement of `hidden` are the same bits
            np.testing.assert_array_equal(lc.bits(b['hidden_cs']), lc.bits(hid[c][0]))
            np.testing.assert_array_equal(lc.bits(b['hidden_dw']), lc.bits(hid[c][1]))
            # counts and dw, the kernel's inputs, are the statement's own intermediate values in both precisions
            x, idx = inp['calls'][c]['x'].astype(np.float64), inp['calls'][c]['idx']
            np.testing.assert_array_equal(x.T @ np.eye(K)[idx], inp['calls'][c]['dw'].astype(np.float64))


@pytest.mark.parametrize('D', lc.ROW_D)
def test_row_cases_hold_their_margins(D):
    for N in lc.ROW_N:
        inp = lc.row_inputs(N, D)
        s = lc.row_sums(inp['x'])
        assert (np.abs(s / lc.ROW_EPS - 1.0) >= 1e-3).all()
        s32 = (torch.tensor(inp['x']) ** 2).sum(1).numpy()
        np.testing.assert_array_equal(s32 > lc.ROW_EPS, s > lc.ROW_EPS)
        if N >= 3:
            assert 0 < s[1] < lc.ROW_EPS and s[2] == 0 and (inp['x'] < 0).any() and (inp['x'] > 0).any()
        refs = [lc.l2_bwd_reference(inp['x'], inp['g'], dt) for dt in (F64, F32)]
        refs += [lc.train_bwd_reference(inp, c, ste, dt) for c in (1.0, 0.1) for ste in (True, False) for dt in (F64, F32)]
        assert _finite(refs) and all(r.shape == (N, D) for r in refs)


def test_numpy_statements_round_once_per_operation():
    """The numpy float32 statements against the same formulas in float64 rounded once at the end: they differ somewhere (else the
    bit-exact GPU comparisons could not tell a fused multiply-add from the statement) yet never by more than a few ulps."""
    rng = np.random.default_rng(0)
    n = 4000
    x, q, gs = (rng.normal(size=n).astype(np.float32) for _ in range(3))
    got = lc.ste_loss_bwd_f32(x, q, gs, 0.37)
    one = (gs.astype(np.float64) + (x.astype(np.float64) - q) * (np.float64(np.float32(0.37)) * np.float32(2.0 / n))).astype(np.float32)
    assert (got != one).any() and np.abs(got - one).max() <= 4 * np.spacing(np.abs(one).max())
    v = np.array([0.0, 1.0, 0.5, -0.25, 1.5, np.nan, np.inf, -np.inf], np.float32)
    c = lc.clip_preserve_f32(v, 0.0, 1.0)
    np.testing.assert_array_equal(lc.bits(c), lc.bits(np.array([0.0, 1.0, 0.5, 0.0, 1.0, np.nan, np.nan, np.nan], np.float32)))
    bc, ks3, ga, gsp = (rng.uniform(0, 1, (n, 3)).astype(np.float32) for _ in range(4))
    alb, spec = lc.ks_split_fwd_f32(bc, ks3[:, :1])
    np.testing.assert_array_equal(spec, ks3[:, :1] * bc)
    g_bc, g_ks = lc.ks_split_bwd_f32(bc, ks3[:, :1], ga, gsp)
    assert g_ks.shape == (n, 1) and g_bc.shape == (n, 3)
    g_bc0, g_ks0 = lc.ks_split_bwd_f32(bc, ks3, None, gsp)
    np.testing.assert_array_equal(g_bc0, gsp * ks3)
    np.testing.assert_array_equal(g_ks0, gsp * bc)
    t = rng.normal(size=(n, 5)).astype(np.float32)
    assert (lc.loss_total_f32(t, 0.3, 0.01, 1, 1, 1) != lc.loss_total_f32(t, 0.3, None, 1, 1, 1)).any()
    np.testing.assert_array_equal(lc.loss_total_f32(t, 0.3, None, 0, 0, 0), (t[:, 0] + t[:, 1]) + np.float32(0.3))
