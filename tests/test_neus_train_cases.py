"""What tests/test_gpu_neus_train_kernels.py rests on, checked without a GPU: the statement of tests/neus_train_cases.py is the
oracle's (oracle/geo.py, pinned to the reference by the goldens), the screening leaves out few candidates and every kept point is
on the same side of every ReLU in both precisions, the references are finite and live, the engines the case table names are the ones
the host code selects -- and the comparison itself can fail (three mutations, each of which must break the bound)."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle import geo as og
from tests import neus_train_cases as nc
from tests.kernel_cases import yardstick

CASES = [(s, P) for s in nc.SHAPES for P in nc.POINTS]


@pytest.mark.parametrize('shape', list(nc.SHAPES))
def test_statement_is_the_oracles_in_float64(shape):
    """On wn_weight(p, l) of the oracle's parameters the statement equals og.sdf_forward / og.sdf_gradient / og.color_forward."""
    cfg = nc.cfg_of(shape)
    p_sdf, p_col = (og.to_torch(p, torch.float64) for p in nc.params_of(shape))
    nS, nCc = len(og.sdf_dims(cfg)) - 1, len(og.color_dims(cfg)) - 1
    ref = nc.reference(shape, 33)
    x, dirs = ref['x'].double(), ref['dirs'].double()
    st = nc.statement(shape, [og.wn_weight(p_sdf, l) for l in range(nS)], [p_sdf[f'lin{l}.bias'] for l in range(nS)],
                      [og.wn_weight(p_col, l) for l in range(nCc)], [p_col[f'lin{l}.bias'] for l in range(nCc)], x, dirs)
    out = og.sdf_forward(p_sdf, cfg, x)
    n = og.sdf_gradient(p_sdf, cfg, x)
    rgb = og.color_forward(p_col, cfg, x, n, dirs, out[:, 1:])
    for k, want in (('sdf', out[:, :1]), ('feat', out[:, 1:]), ('n', n), ('rgb', rgb)):
        assert st[k].dtype == np.float64 and np.abs(st[k] - want.numpy()).max() <= 1e-12, k
    s = nc.SHAPES[shape]
    assert [p.shape[1] for p in st['pre']] == [s.c_hidden] * s.c_layers and st['feat'].shape[1] == s.d_out - 1


@pytest.mark.parametrize('shape,P', CASES)
def test_screening_and_kept_points(shape, P):
    ref = nc.reference(shape, P)
    assert ref['x'].shape == (P, 3) and ref['dirs'].shape == (P, 3) and ref['n_candidates'] == 2 * P
    # a cap on what a case may leave out, not a measurement
    assert ref['n_rejected'] <= nc.REJECT_CAP * ref['n_candidates'], (ref['n_rejected'], ref['n_candidates'])
    assert np.abs(np.linalg.norm(ref['dirs'].double().numpy(), axis=1) - 1.0).max() <= 1e-6
    assert float(ref['x'].abs().max()) <= 1.0
    p32, p64 = (np.concatenate(ref[k]['pre'], 1).astype(np.float64) for k in ('f32', 'f64'))
    assert np.abs(p64).min() >= nc.MARGIN
    assert np.array_equal(p32 > 0.0, p64 > 0.0)
    # the float32 statement uses up at most a quarter of any pre-activation's margin (its distance from the kink, >= MARGIN): an
    # evaluation three times as far off as float32 torch -- what the yardstick admits -- is still on the same side of every ReLU
    assert (np.abs(p32 - p64) <= 0.25 * np.abs(p64)).all(), float((np.abs(p32 - p64) / np.abs(p64)).max())
    # and, where the absolute margin is what counts -- within 100 margins of the kink --, within a quarter of MARGIN itself (for every
    # pre-activation that cannot hold: float32 is 3e-6 off on activations of order 1)
    near = np.abs(p64) <= 100.0 * nc.MARGIN
    assert (np.abs(p32 - p64)[near] <= 0.25 * nc.MARGIN).all()


@pytest.mark.parametrize('shape,P', CASES)
def test_references_are_finite_and_live(shape, P):
    ref = nc.reference(shape, P)
    for key in ('f32', 'f64'):
        r = ref[key]
        for k in ('sdf', 'n', 'rgb'):
            assert np.isfinite(r[k]).all() and r[k].shape[0] == P, (key, k)
        assert set(r['grads']) == {'all', 'rgb'}
        for v, gs in r['grads'].items():
            assert list(gs) == nc.grad_names(shape)
            for k, g in gs.items():
                assert np.isfinite(g).all(), (key, v, k)
        for k, g in r['grads']['all'].items():
            assert np.any(g != 0.0), (key, k)
    # the float32 statement against itself passes the check it is the yardstick of
    assert nc.pooled_gradient_check(ref['f32']['grads']['all'], ref['f32']['grads']['all'], ref['f64']['grads']['all'])['ok']


@pytest.mark.parametrize('shape', list(nc.SHAPES))
def test_engines_of_the_table(shape, monkeypatch):
    """NeusTrainEngine from CPU modules: the constructor, forward_mode() and backward_mode() are host Python."""
    eng = nc.build_engine(shape)
    s = nc.SHAPES[shape]
    assert eng.E == 3 + 6 * s.multires and eng.X == 9 + 6 * s.multires_view and eng.F == s.d_out and eng.scale == s.scale
    assert eng.nL == s.n_layers and eng.nC == s.c_layers and eng.squeeze == s.squeeze_out
    assert eng.skip == (s.skip_in[0] if s.skip_in else -1)
    for engine in nc.SHAPE_ENGINES[shape]:
        nc.select(monkeypatch, engine)
        assert (eng.forward_mode(), eng.backward_mode()) == nc.MODES[engine], (shape, engine)
        ran, not_ran = nc.expected_entries(engine)
        assert len(ran) in (2, 3) and not set(ran) & set(not_ran) and set(ran) | set(not_ran) == set(nc.ALL_ENTRIES)


def test_case_table_is_the_documented_one():
    assert set(nc.SHAPE_ENGINES) == set(nc.SHAPES) and len(nc.GPU_CASES) == 20 and ('w288', 'default') in nc.GPU_CASES
    widths = {k: [s.d_hidden - (3 + 6 * s.multires) if l + 1 in s.skip_in else s.d_hidden for l in range(s.n_layers)] for k, s in nc.SHAPES.items()}
    assert 137 in widths['w200'] and 185 in widths['w224'] and 9 in widths['w48'] and 102 in widths['w129']
    assert nc.SHAPES['w200'].multires * 6 + 3 == 63 and nc.SHAPES['w200'].multires_view * 6 + 9 == 15
    assert nc.POINTS == (1, 33, 65, 161) and set(nc.POISON_POINTS) <= set(nc.POINTS)
    assert len({nc.seed_of(s, P) for s in nc.SHAPES for P in nc.POINTS}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------- the comparison can fail
def _outputs_ok(got, ref):
    return {k: yardstick(got[k], ref['f32'][k], ref['f64'][k])['ok'] for k in ('sdf', 'n', 'rgb')}


@pytest.mark.parametrize('shape', list(nc.SHAPES))
def test_one_wrong_gradient_entry_breaks_the_bound(shape):
    """One entry of one float64 gradient tensor moved by 1e-4 of the tensor's largest entry: the pooled bound rejects it, in every
    tensor of the case, and names that tensor alone."""
    ref = nc.reference(shape, 65)
    r32, r64 = ref['f32']['grads']['all'], ref['f64']['grads']['all']
    clean = nc.pooled_gradient_check(r64, r32, r64)
    assert clean['ok'] and nc.EPS8 <= clean['bound'] < 1e-4 / 3.0 and clean['rms_bound'] <= clean['bound']
    for k in nc.grad_names(shape):
        got = copy.copy(r64)
        g = got[k] = r64[k].copy()
        g.reshape(-1)[g.size // 2] += 1e-4 * np.abs(r64[k]).max()
        res = nc.pooled_gradient_check(got, r32, r64)
        assert not res['ok'] and res['bad'] == [k], (k, res['bad'])


@pytest.mark.parametrize('shape', [k for k, s in nc.SHAPES.items() if s.skip_in])
def test_dropping_the_skip_layers_sqrt2_breaks_the_bound(shape):
    """A copy of the statement without the 1/sqrt2 of the skip layer, in float32, in the kernel's place."""
    ref = nc.reference(shape, 65)
    adj = {'all': (ref['g_rgb'], ref['g_n'], ref['g_sdf'])}
    right = nc.statement(shape, *nc._leaves(shape, torch.float32, True), ref['x'], ref['dirs'], adj)
    wrong = nc.statement(shape, *nc._leaves(shape, torch.float32, True), ref['x'], ref['dirs'], adj, skip_div=False)
    assert all(_outputs_ok(right, ref).values())
    assert nc.pooled_gradient_check(right['grads']['all'], ref['f32']['grads']['all'], ref['f64']['grads']['all'])['ok']
    assert not any(_outputs_ok(wrong, ref).values())
    res = nc.pooled_gradient_check(wrong['grads']['all'], ref['f32']['grads']['all'], ref['f64']['grads']['all'])
    assert not res['ok'] and len(res['bad']) > len(nc.grad_names(shape)) // 2, res['bad']


def test_dropping_the_sdf_outputs_scale_breaks_the_bound():
    """A copy of the statement without the 1/scale of the sdf output (w224: scale 1.5), in float32, in the kernel's place."""
    shape = 'w224'
    assert nc.SHAPES[shape].scale != 1.0
    ref = nc.reference(shape, 65)
    adj = {'all': (ref['g_rgb'], ref['g_n'], ref['g_sdf'])}
    wrong = nc.statement(shape, *nc._leaves(shape, torch.float32, True), ref['x'], ref['dirs'], adj, sdf_div=False)
    ok = _outputs_ok(wrong, ref)
    assert not ok['sdf'] and not ok['n'] and not ok['rgb']
    res = nc.pooled_gradient_check(wrong['grads']['all'], ref['f32']['grads']['all'], ref['f64']['grads']['all'])
    assert not res['ok'] and f'dW{nc.SHAPES[shape].n_layers}' in res['bad']
    assert math.isclose(float(np.abs(wrong['sdf']).max() / np.abs(ref['f64']['sdf']).max()), 1.5, rel_tol=1e-5)
