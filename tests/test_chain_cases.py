"""CPU: the case table of tests/chain_cases.py before a GPU sees it.  For every case and both engines (where the builder takes the
program) the descriptor + pack that packing.ChainBuilder makes, run by the numpy emulators of tests/chain_model.py, equals the case's
plain float64 reference: row assignment, gather indices and descriptor fields at ragged shapes.  And the table reaches the paths of
the kernels that the reflectance model's own programs do not (MODEL_REACHES below says which those are)."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests.chain_model import emulate, emulate_f16s
from tests.decomp_util import make_config
from vqnerf_release_amd.decomp import packing as pk

N = 33
RUNS = [(c['name'], e) for c in cc.CASES for e in c['engines']]


def _emulated(case, built, x, mode):
    run = emulate if mode == 'f32' else emulate_f16s
    parts = [run(built['desc'], built['wbuf'].numpy(), x[p0:p0 + 32], built['widths']) for p0 in range(0, x.shape[0], 32)]
    return [np.concatenate([p[s] for p in parts], 0) for s in range(len(built['widths']))]


@pytest.mark.parametrize('name,mode', RUNS)
def test_emulated_program_equals_the_float64_reference(name, mode):
    """f32 layout: 1e-9, the bound of test_chain_packing.py for the same comparison; f16s: that file's 3e-6 of the output scale"""
    case = cc.BY_NAME[name]
    data = cc.make_data(case, 'real', N)
    built = cc.build(case, data, mode)
    want, _, _ = cc.reference(case, data)
    got = _emulated(case, built, data['x'], mode)
    assert len(got) == len(want)
    for s, g in enumerate(got):
        assert g.shape == want[s].shape == (N, built['widths'][s])
        atol = 1e-9 if mode == 'f32' else 3e-6 * max(1.0, np.abs(want[s]).max())
        np.testing.assert_allclose(g, want[s], rtol=0, atol=atol, err_msg=f'{name} {mode} slot {s}')


def test_integer_data_set_is_exact_where_the_device_test_asks_for_equality():
    """the bound sum |w| |x| + |b| of every slot compared for equality is below 2^24 (any order of summation is exact in float32), and
    the emulated f32 program reproduces the integers"""
    n_exact = 0
    for case in cc.CASES:
        data = cc.make_data(case, 'int', N)
        want, _, bounds = cc.reference(case, data, want_bounds=True)
        ex = cc.exact_slots(case)
        if not ex:
            continue
        got = _emulated(case, cc.build(case, data, 'f32'), data['x'], 'f32')
        for s in ex:
            assert bounds[s] < 2 ** 24, (case['name'], s, bounds[s])
            assert np.array_equal(want[s], np.round(want[s])) and np.array_equal(got[s], want[s]), (case['name'], s)
            n_exact += 1
    assert n_exact >= 8


def test_same_first_rows_at_every_point_count():
    for name in cc.BIG_CASES:
        case = cc.BY_NAME[name]
        for kind in ('int', 'real'):
            a, b = cc.make_data(case, kind, N), cc.make_data(case, kind, 4133)
            assert np.array_equal(a['x'], b['x'][:N], equal_nan=True)
            assert all(np.array_equal(a['params'][i][0], b['params'][i][0]) for i in a['params'])


# ------------------------------------------------------------------------------------------------------------------ coverage
def reached(plans):
    """what a set of f32 plans reaches of the kernel's paths"""
    r = dict(ng=set(), waves=set(), late_tiles=set(), small_out=set(), small_rows_below_waves=False, gemm_act=set(), small_act=set(),
             idle_waves=set(), uneven_tiles=set(), reload=False, n_layers=0, n_slots=0, idle_first=False)
    for plan in plans:
        r['waves'].add(plan.n_waves)
        r['n_layers'] = max(r['n_layers'], len(plan.layers))
        r['n_slots'] = max(r['n_slots'], plan.b.n_slots)
        gemm = [L for L in plan.layers if L['kind'] == 0]
        # a wave without a tile in the first GEMM layer that owns one (of >= 4 K rows: a look-ahead target) later
        r['idle_first'] |= any(L['tiles'] > gemm[0]['tiles'] and gemm[0]['tiles'] < plan.n_waves and sum(L['k_rows']) >= 4 for L in gemm[1:])
        for L in plan.layers:
            ng = sum(L['k_rows'])
            if L['kind'] == 2:
                r['reload'] = True
            elif L['kind'] == 0:
                r['ng'].add(ng if ng < 9 else '>=9')
                r['gemm_act'].add(L['act'] & 0xff)
                if L['act'] & pk.LATE_EPILOGUE:
                    r['late_tiles'].add(L['tiles'])
                if L['tiles'] < plan.n_waves:
                    r['idle_waves'].add(plan.n_waves)
                if L['tiles'] > plan.n_waves and L['tiles'] % plan.n_waves:
                    r['uneven_tiles'].add(plan.n_waves)
            else:
                r['small_out'].add(L['out'])
                r['small_act'].add(L['act'])
                r['small_rows_below_waves'] |= ng < plan.n_waves
    return r


# What the reflectance model's own programs (nfr_unit's builders at the shipped widths: encoder, the two head forms, encoder + heads)
# reach -- asserted below, so the listing cannot rot.  Everything the case table reaches beyond it is checked by these tests alone:
#   ng          the model: 8 (63 features), 16, 32 and 40 rows only         the table adds 1, 3, 4, 5
#   waves       4                                                          the table adds 8
#   late tiles  4 (the 128-wide head layer)                                the table adds 1, 2, 3
#   small out   1 and 3                                                    the table adds 2, 4
#   activations relu, none and sigmoid in GEMM layers, sigmoid in small    the table adds the softplus GEMM epilogue and
#               layers                                                     relu / softplus / none small layers
#   tiles       always a multiple of 4 per layer: no idle wave, no wave with one tile more than another
#   small rows  never fewer than the waves
#   idle first  no wave idles in the first GEMM layer and owns a tile later   the table: idle_then_busy
MODEL_REACHES = dict(ng={8, '>=9'}, waves={4}, late_tiles={4}, small_out={1, 3}, small_rows_below_waves=False, gemm_act={0, 1, 3},
                     small_act={3}, idle_waves=set(), uneven_tiles=set(), reload=True, n_layers=16, n_slots=4, idle_first=False)


def _model_plans():
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    model = get_model_class('vq_nfr')(make_config())
    model.build_nets(device='cpu', seed=5)
    fam = {suf: [h + '_' + suf for h in model.HEADS] for suf in ('main', 'vq')}
    plans = [model._enc_program()] + [model._head_program(n) for n in fam.values()] + [model._enc_heads_program(n) for n in fam.values()]
    b = pk.ChainBuilder('raw', model.z_dim)                     # the head form that fetches the input again (heads wider than 128)
    x = b.input
    y0 = b.dense('h/0', [x], 256, 'relu')
    y1 = b.dense('h/1', [y0], 256, 'relu')
    x = b.reload_input(keep=[y1])
    b.dense_small('h/2', [y1, x], 3, 'sigmoid', 0)
    return plans + [b.build()]


def test_the_table_reaches_what_the_model_does_not():
    table = reached([cc.build(c, cc.make_data(c, 'real', 1), 'f32')['plan'] for c in cc.CASES])
    assert table['ng'] >= {1, 3, 4, 5, 8, '>=9'}
    assert table['waves'] == {4, 8}
    assert table['late_tiles'] == {1, 2, 3, 4}
    assert table['small_out'] == {1, 2, 3, 4}
    assert table['gemm_act'] == table['small_act'] == {0, 1, 2, 3}
    assert table['small_rows_below_waves'] and table['reload'] and table['idle_first']
    assert table['idle_waves'] == {4, 8} and table['uneven_tiles'] == {4, 8}
    assert table['n_layers'] == pk.MAX_LAYERS and table['n_slots'] == pk.MAX_OUTS
    assert cc.build(cc.BY_NAME['eight_waves'], cc.make_data(cc.BY_NAME['eight_waves'], 'real', 1), 'f32')['plan'].n_waves == 8
    assert cc.build(cc.BY_NAME['eight_waves_uneven'], cc.make_data(cc.BY_NAME['eight_waves_uneven'], 'real', 1), 'f32')['plan'].n_waves == 8
    assert reached(_model_plans()) == MODEL_REACHES
