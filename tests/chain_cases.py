"""Case table of the Dense-stack chain kernels (csrc/mlp_chain.hip, csrc/mlp_chain_f16s.hip): small networks stated in words of
their own -- not through the descriptor -- with two renderings:

  reference(case, data, x, prec)   plain numpy matmuls, float64 (the model) or float32 (the yardstick of the tolerance rules);
                                   concatenation in Keras order, positional encoding as oracle.decomp.posenc, softplus
                                   log1p(exp(100 t)) / 100, exact sigmoid;
  build(case, data, mode)          the same network through packing.ChainBuilder -> plan, desc, wbuf, widths, leading dimensions.

A case: in_mode ('raw' | 'posenc'), in_feats, in_stride, n_freqs, engines, and `layers`, each one of
  dict(op='dense', name, src=[tensor names, Keras concat order], width, act, slot=None, ld=None, over=None)
  dict(op='small', src, width (1..4), act, slot, ld=None)
  dict(op='reload')                                       the input image again: 'x' names the new copy from here on
'x' is the input; which tensors the builder has to keep is derived from the later layers' `src`.

Two data sets per case, fixed seeds: 'int' (inputs, weights, biases small integers in [-2, 2]) and 'real' (inputs uniform in [-1, 1],
weights normal / sqrt(fan_in), biases uniform in [-0.5, 0.5]).  Everything is float32-representable; the reference reads it as is.

Three additions to the table as first planned.  `eight_waves_uneven` has a layer whose tile count is no multiple of 8 waves.  `sixteen_layers` hands layer 1 to slot 1 as well, because its slot 0 lies behind
softplus and sigmoid layers and the exact (integer) comparison needs an output before the first transcendental.  `idle_then_busy`
was added when skipping the idle-wave refill of the weight look-ahead (mlp_prims.h, end of gemm_tiles_chain) failed no test."""
import zlib

import numpy as np
import torch

from oracle import decomp as od
from tests import tile_vm_model as vm
from vqnerf_release_amd.decomp import packing as pk

ACT_ID = {'none': vm.NONE, 'relu': vm.RELU, 'softplus100': vm.SOFTPLUS, 'sigmoid': vm.SIGMOID}
EXACT_ACTS = ('none', 'relu')
BOTH, F32_ONLY = ('f32', 'f16s'), ('f32',)


def _dense(name, src, width, act, slot=None, ld=None, over=None):
    return dict(op='dense', name=name, src=list(src), width=width, act=act, slot=slot, ld=ld, over=over)


def _small(src, width, act, slot, ld=None):
    return dict(op='small', name=None, src=list(src), width=width, act=act, slot=slot, ld=ld)


def _case(name, in_mode, in_feats, in_stride, layers, n_freqs=0, engines=BOTH, int_range=2):
    return dict(name=name, in_mode=in_mode, in_feats=in_feats, in_stride=in_stride, n_freqs=n_freqs, layers=layers, engines=engines,
                int_range=int_range)


def _ragged(name, stride, ld):
    return _case(name, 'raw', 21, stride, [_dense('y0', ['x'], 40, 'relu'), _dense('y1', ['y0', 'x'], 17, 'none', slot=0, ld=ld)])


def _in_place(T):
    return _case(f'in_place_{T}', 'raw', 40, 40, [
        _dense('y0', ['x'], 128, 'relu'), _dense('y1', ['y0'], 32 * T, 'sigmoid', over='y0'), _small(['y1', 'x'], T, 'none', 0)],
        engines=F32_ONLY)


def _posenc(n_freqs):
    return _case(f'posenc_{n_freqs}', 'posenc', 3 + 6 * n_freqs, 3, [
        _dense('y0', ['x'], 40, 'softplus100'), _dense('y1', ['y0'], 8, 'none', slot=0)], n_freqs=n_freqs)


CYCLE = ('relu', 'none', 'softplus100', 'sigmoid')

CASES = [
    # ng = 1: no look-ahead target, clamped fetches, scalar store
    _case('one_row', 'raw', 3, 3, [_dense('y0', ['x'], 32, 'relu'), _dense('y1', ['y0'], 5, 'none', slot=0, ld=5)]),
    # ng 3 and 5 + 3; 2 tiles and 1 tile under 4 waves; both vector boundaries (21 of 24 in, 17 of 20 out)
    _ragged('ragged_k', 24, 20),
    # the scalar load and store paths
    _ragged('odd_stride', 23, 17),
    # 5 and 3 tiles over 4 waves; ng 8 and 20
    _case('tiles_5_3', 'raw', 64, 64, [_dense('y0', ['x'], 160, 'relu'), _dense('y1', ['y0'], 96, 'none', slot=0)]),
    # the late (in-place) epilogue with 1..4 tiles
    _in_place(1), _in_place(2), _in_place(3), _in_place(4),
    # the input dropped and fetched again for the last layer (the form of the reflectance heads that do not keep z resident)
    _case('reload', 'posenc', 27, 5, [
        _dense('y0', ['x'], 64, 'relu'), _dense('y1', ['y0'], 64, 'relu'), dict(op='reload'), _small(['y1', 'x'], 3, 'sigmoid', 0)],
        n_freqs=4),
    _posenc(0), _posenc(16),
    # all four slots; every activation in a GEMM epilogue; relu and softplus in act_rt (none: in_place, sigmoid: reload)
    _case('four_slots', 'raw', 24, 24, [
        _dense('y0', ['x'], 48, 'relu'),
        _dense('y1', ['y0'], 36, 'sigmoid', slot=0, ld=40),
        _dense('y2', ['y0', 'x'], 33, 'none', slot=1, ld=33),
        _dense('y3', ['y0'], 40, 'softplus100'),
        _small(['y3', 'x'], 4, 'softplus100', 2),
        _small(['y0'], 1, 'relu', 3)]),
    # 1 + 1 K rows: fewer than the waves
    _case('small_few_rows', 'raw', 8, 8, [_dense('y0', ['x'], 8, 'relu'), _small(['y0', 'x'], 2, 'none', 0)]),
    # 136 rows: an 8-wave program
    _case('eight_waves', 'posenc', 63, 3, [
        _dense('y0', ['x'], 512, 'relu'), _dense('y1', ['y0', 'x'], 512, 'relu'), _dense('y2', ['y1'], 33, 'none', slot=0),
        _small(['y2'], 2, 'none', 1)], n_freqs=10),
    # 12 tiles under 8 waves: waves 0..3 own two tiles, waves 4..7 one
    _case('eight_waves_uneven', 'posenc', 63, 3, [
        _dense('y0', ['x'], 512, 'relu'), _dense('y1', ['y0', 'x'], 384, 'relu'), _dense('y2', ['y1'], 33, 'none', slot=0)], n_freqs=10),
    # waves 1..3 own no tile in the FIRST GEMM layer and one each in the second: with nothing in flight yet, the fragments they owe
    # the second layer come from the idle-wave refill alone (in every other case of the table a wave that idles has either no later
    # tile or fragments left from an earlier layer that happen to be the right ones)
    _case('idle_then_busy', 'raw', 16, 16, [_dense('y0', ['x'], 32, 'relu'), _dense('y1', ['y0'], 128, 'none', slot=0)]),
    # n_layers == MAX_LAYERS
    _case('sixteen_layers', 'raw', 32, 32, [
        _dense(f'y{i}', ['x' if i == 0 else f'y{i - 1}'], 32, CYCLE[i % 4], slot={1: 1, 15: 0}.get(i)) for i in range(16)]),
]
BY_NAME = {c['name']: c for c in CASES}
MORE_POINT_COUNTS = ('ragged_k', 'tiles_5_3', 'four_slots', 'eight_waves')         # N in {1, 31, 32} besides 33
BIG_CASES = ('ragged_k', 'reload')                                                  # N_big: every workgroup takes >= 2 tiles


def n_big(n_cus):
    """launch.h gives at most two workgroups per CU: at this N every workgroup takes at least two tiles and the last tile is ragged"""
    return 32 * (4 * n_cus) + 5


def slots(case):
    """{slot: (layer index, width, ld)}"""
    return {L['slot']: (i, L['width'], L['ld'] or L['width']) for i, L in enumerate(case['layers']) if L.get('slot') is not None}


def raw_width(case):
    """columns of x the kernel may read"""
    return 3 if case['in_mode'] == 'posenc' else case['in_feats']


def fan_in(case, L):
    w = {'x': case['in_feats']}
    for M in case['layers']:
        if M['op'] == 'dense':
            w[M['name']] = M['width']
    return sum(w[s] for s in L['src'])


def make_data(case, kind, N):
    """-> dict(x [N, in_stride] float32 (NaN in the padding columns), params {layer index: (W [in, out], b [out])} float32).
    Weights are drawn before the points and the points row by row: the first rows are the same whatever N."""
    rng = np.random.default_rng(zlib.crc32(f'{case["name"]}/{kind}'.encode()))
    params = {}
    for i, L in enumerate(case['layers']):
        if L['op'] == 'reload':
            continue
        k, n = fan_in(case, L), L['width']
        if kind == 'int':
            r = case['int_range']
            W, b = rng.integers(-r, r + 1, (k, n)), rng.integers(-r, r + 1, (n,))
        else:
            W, b = rng.normal(size=(k, n)) / np.sqrt(k), rng.uniform(-0.5, 0.5, (n,))
        params[i] = (W.astype(np.float32), b.astype(np.float32))
    x = np.full((N, case['in_stride']), np.nan, np.float32)
    w = raw_width(case)
    r = case['int_range']
    x[:, :w] = rng.integers(-r, r + 1, (N, w)) if kind == 'int' else rng.uniform(-1, 1, (N, w))
    return dict(x=x, params=params)


def _posenc32(x, n_freqs):
    """float32 restatement: 2^k x is exact in float32, sin / cos rounded once"""
    outs = [x]
    for k in range(n_freqs):
        a = (x * np.float32(2.0 ** k)).astype(np.float32)
        outs += [np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)]
    return np.concatenate(outs, -1)


def _act(name, t, prec):
    if prec == 'f32':
        return vm.act(ACT_ID[name], t.astype(np.float32), 'f32')
    if name == 'relu':
        return np.maximum(t, 0)
    if name == 'softplus100':
        return np.logaddexp(0.0, 100.0 * t) / 100.0                   # log1p(exp(100 t)) / 100, without the overflow
    if name == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-np.maximum(t, -700.0)))
    return t


def reference(case, data, prec='f64', want_bounds=False):
    """-> (outs {slot: [N, width]}, tensors {name: values entering later layers}, bounds {slot: max of sum |w| |x| + |b|} | None).
    prec 'f32': every product, sum and activation in float32 (numpy's order of summation): the yardstick, not a model."""
    dt = np.float64 if prec == 'f64' else np.float32
    xin = data['x'][:, :raw_width(case)]
    if case['in_mode'] == 'posenc':
        feats = od.posenc(torch.tensor(xin, dtype=torch.float64), case['n_freqs']).numpy() if prec == 'f64' else _posenc32(xin, case['n_freqs'])
    else:
        feats = xin.astype(dt)
    T, mag = {'x': feats.astype(dt)}, {'x': np.abs(feats).astype(np.float64)}
    outs, bounds = {}, {}
    for i, L in enumerate(case['layers']):
        if L['op'] == 'reload':
            continue
        W, b = (a.astype(dt) for a in data['params'][i])
        K = np.concatenate([T[s] for s in L['src']], -1)
        y = _act(L['act'], (K @ W + b).astype(dt), prec).astype(dt)
        m = np.concatenate([mag[s] for s in L['src']], -1) @ np.abs(W).astype(np.float64) + np.abs(b).astype(np.float64)
        if L['op'] == 'dense':
            T[L['name']], mag[L['name']] = y, m
        if L['slot'] is not None:
            outs[L['slot']], bounds[L['slot']] = y, float(m.max())
    return (outs, T, bounds) if want_bounds else (outs, T, None)


def upstream(case, i):
    """indices of layer i and of every layer its value depends on; -> (set, True if the raw input feeds it unencoded)"""
    by_name = {L['name']: j for j, L in enumerate(case['layers']) if L.get('name')}
    seen, todo = set(), [i]
    while todo:
        j = todo.pop()
        if j in seen:
            continue
        seen.add(j)
        todo += [by_name[s] for s in case['layers'][j]['src'] if s != 'x']
    return seen


def exact_slots(case):
    """slots whose value is a sum of products of integers on the 'int' data set: every layer it depends on ends in relu or none, and
    the input is raw (a positional encoding of n_freqs = 0 is the raw point as well)"""
    if case['in_mode'] == 'posenc' and case['n_freqs'] > 0:
        return []
    return [s for s, (i, _, _) in sorted(slots(case).items())
            if all(case['layers'][j]['act'] in EXACT_ACTS for j in upstream(case, i))]


def gemm_inputs(case, slot):
    """names of the tensors that enter a GEMM layer (not a row-dot layer) on the way to `slot`"""
    names = set()
    for j in upstream(case, slots(case)[slot][0]):
        if case['layers'][j]['op'] == 'dense':
            names |= set(case['layers'][j]['src'])
    return names


def build(case, data, mode):
    """-> dict(plan, desc, wbuf (CPU float32), widths, lds) with widths / lds per slot 0..n-1"""
    b = pk.ChainBuilder(case['in_mode'], case['in_feats'], n_freqs=case['n_freqs'], in_stride=case['in_stride'], mode=mode)
    layers = case['layers']
    # names -> versions: a reload makes 'x' a new tensor
    ver, x_now = [], 'x#0'
    for L in layers:
        if L['op'] == 'reload':
            x_now = f'x#{int(x_now[2:]) + 1}'
            ver.append([])
        else:
            ver.append([x_now if s == 'x' else s for s in L['src']])
    regions = {'x#0': b.input}
    x_now = 'x#0'
    for i, L in enumerate(layers):
        later = {s for v in ver[i + 1:] for s in v}
        if L['op'] == 'reload':
            x_now = f'x#{int(x_now[2:]) + 1}'
            regions[x_now] = b.reload_input(keep=[regions[s] for s in later if s in regions])
            continue
        segs = [regions[s] for s in ver[i]]
        if L['op'] == 'small':
            b.dense_small(str(i), segs, L['width'], L['act'], L['slot'])
            continue
        over = regions[L['over']] if L['over'] else None
        assert L['over'] not in later
        keep = [regions[s] for s in sorted(later) if s in regions]
        regions[L['name']] = b.dense(str(i), segs, L['width'], L['act'], keep=keep, out_slot=L['slot'], over=over)
    plan = b.build()
    params = {str(i): (torch.from_numpy(W), torch.from_numpy(bb)) for i, (W, bb) in data['params'].items()}
    wbuf, desc = plan.pack(params)
    sl = slots(case)
    assert sorted(sl) == list(range(len(sl)))
    return dict(plan=plan, desc=desc, wbuf=wbuf, widths=[sl[s][1] for s in sorted(sl)], lds=[sl[s][2] for s in sorted(sl)])
