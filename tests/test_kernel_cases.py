"""The conditions the per-kernel GPU tests rest on, checked from the oracles alone (no GPU): the refactored oracle statements
still say what they said, the references are finite, float32 and float64 take the same branches on the compositing inputs, and
the float32 / float64 up-sampling oracles agree on at least seven rays in eight."""
import math

import numpy as np
import pytest
import torch

from oracle import decomp as od
from oracle import geo as og
from tests import kernel_cases as kc


def test_make_points_default_draws_unchanged():
    a, b = od.make_points(40, seed=7), od.make_points(40, seed=7, n_lights=1024)
    assert a['lvis'].shape == (40, 512) and b['lvis'].shape == (40, 1024)
    for k in ('xyz', 'normal', 'rayo', 'rgb'):
        np.testing.assert_array_equal(a[k], b[k])
    rng = np.random.default_rng(7)                             # the draws of the function as it was: four arrays, then the rows
    rng.uniform(-1, 1, (40, 3)); rng.uniform(0.5, 1.0, (40, 1)); rng.normal(size=(40, 3)); rng.uniform(0, 1, (40, 3))
    np.testing.assert_array_equal(a['lvis'], (rng.uniform(size=(40, 512)) < 0.7).astype(np.float32))


def test_render_integrate_clip_switch():
    inp = kc.shade_inputs(30, 256, 1, True)
    bright = inp['light'] * 8.0
    raw = kc.shade_reference(inp, torch.float64, grads=False, clip=False, light=bright)['rgb'][0]
    clipped = kc.shade_reference(inp, torch.float64, grads=False, clip=True, light=bright)['rgb'][0]
    np.testing.assert_array_equal(clipped, np.clip(raw, 0.0, 1.0))
    assert (raw > 1.0).any()


@pytest.mark.parametrize('n,B,car,bg,inv_s', [(1, 5, 0.3, (1.0, 1.0, 1.0), 64.0), (3, 7, 1.0, None, 512.0), (65, 64, 0.0, (1.0, 1.0, 1.0), math.exp(5.0)),
                                              (256, 16, 0.3, None, 2e6)])
def test_composite_case_conditions(n, B, car, bg, inv_s):
    inp = kc.composite_inputs(B, n, inv_s)
    names = list(kc.ADJOINT_SETS)
    f64, g64 = kc.composite_reference(inp, car, bg, torch.float64, names)
    f32, g32 = kc.composite_reference(inp, car, bg, torch.float32, names)
    assert kc.composite_margins_ok(inp, f64)
    np.testing.assert_array_equal(kc.branch_indicators(f32), kc.branch_indicators(f64))
    for g in list(g64.values()) + list(g32.values()):
        assert all(np.isfinite(t).all() for t in g)
    if not 1e-6 <= inv_s <= 1e6:
        assert all(not g[3].any() for g in g64.values())
    # the yardstick accepts the float32 reference itself and refuses a dropped term
    assert kc.yardstick(g32['all'][0], g32['all'][0], g64['all'][0])['ok']
    if inv_s < 1e6 and n > 1:
        assert not kc.yardstick(g32['weights'][0], g32['all'][0], g64['all'][0])['ok']


@pytest.mark.parametrize('N,L,n_sets,with_lvis', [(1, 256, 1, True), (12, 512, 2, True), (12, 1024, 2, False)])
def test_shade_case_conditions(N, L, n_sets, with_lvis):
    inp = kc.shade_inputs(N, L, n_sets, with_lvis)
    r64, r32 = kc.shade_reference(inp, torch.float64), kc.shade_reference(inp, torch.float32)
    n0 = sum(int((ms[2] == 0.0).sum()) for ms in inp['mats'])
    assert n0 == n_sets                                        # the rough = 0 edge is in every case
    assert kc.rough0_limit(inp, r64) <= n0 and kc.rough0_limit(inp, r32) <= n0
    E = kc.EDGES.index
    if N >= 10:
        dark = (inp['edge'] == E('all_behind')) | (inp['edge'] == E('zero_gsum'))
        for s in range(n_sets):
            assert all(not g[dark].any() for g in r64['g'][s])
        assert not r64['rgb'][0][inp['edge'] == E('all_behind')].any()
        assert r64['g_light'].any()


def test_upsample_oracles_agree_on_seven_rays_in_eight():
    worst = 0
    for n, m, s in kc.UPSAMPLE_GRID:
        c = kc.upsample_case(n, m, s)
        left_out = int((~c['agree'][:8]).sum())
        assert left_out <= 1, (n, m, s, left_out)
        worst = max(worst, left_out)
        assert np.isfinite(c['ref64']).all()
    assert worst <= 1


def test_merge_reference_is_stable():
    z, s, zn, sn = kc.merge_inputs(5, 64, 16)
    zs, ss = kc.merge_reference(z, s, zn, sn)
    assert (np.diff(zs, axis=1) >= 0).all() and (np.diff(zs, axis=1) == 0).any()
    old = np.isin(ss, s)
    for r in range(5):                                         # among equal depths: old before new, new ones in input order
        for i in range(zs.shape[1] - 1):
            if zs[r, i] == zs[r, i + 1]:
                assert old[r, i] or not old[r, i + 1]
                if not old[r, i] and not old[r, i + 1]:
                    assert list(sn[r]).index(ss[r, i]) < list(sn[r]).index(ss[r, i + 1])
