"""The Dense-stack chain kernels (vqn_mlp_chain_fwd, vqn_mlp_chain_fwd_f16s) program by program against the float64 reference of
tests/chain_cases.py, and the refusals of the three chain entry points.

Every case runs once per engine and point count (the launch count is asserted), on both data sets.  The input stands between finite
poison margins with NaN in the `in_stride - in_feats` padding columns; the outputs are NaN-prefilled [N, ld] buffers between guards:
  * written set -- exactly the elements [n < N, f < width] of every slot are no longer NaN; the `ld - width` tail still is;
  * integer data set, f32 engine -- for the slots that depend on relu / none layers of a raw input only, the bound sum |w| |x| + |b|
    through the layers is below 2^24 (asserted), so every partial sum is exact in float32 in any order: the output EQUALS the float64
    value.  f16s engine: the same, where besides every tensor entering a layer on the way is an integer below 2^11 (asserted from
    the reference): such a value is exact in one f16, the small-integer weights have zero low halves, the products accumulate in f32;
  * everything else -- per output feature, the rule of tests/test_gpu_tile_vm_ops.py for the same activation functions: the error
    against float64 is within 8 x the float32 restatement's own error, floor 4 * 2^-24 * max|model|.  f16s: 4 x the float32
    restatement's error + 2e-6 of the slot's scale (the bound test_gpu_decomp.py states for this engine).  No element is left out;
    every figure is recorded (profiles/observed_errors_chain_programs.json).  A run of N < 33 points uses the first N rows of the
    33-point data set: it takes a feature's two figures over those 33 points (see _compare) and must give the bits of the 33-point
    run's first N rows.  With a feature's figures taken over the one point of an N = 1 run the rule was missed four times on the
    f32 engine (kernel error / restatement error / bound: ragged_k 2.8e-8 / 1.5e-9 / 1.5e-8, tiles_5_3 7.7e-8 / 9.1e-10 / 1.5e-8,
    four_slots slot 1 3.4e-8 / 5.3e-11 / 1.4e-8, eight_waves integer data 2.0e-3 / 5.6e-5 / 4.5e-4 on values of 1e3..1e4) by the
    very bits that pass as row 0 of the 33-point runs: half an ulp of the sum's terms against four ulps of a sum that cancels;
  * launch-size independence -- the first 33 rows at N_big (every workgroup takes at least two tiles) are bit-identical to N = 33.
Refused calls get real allocations, large enough for the access a missing check would make."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import chain_cases as cc
from tests.gpu_util import launches, record_observed
from tests.test_gpu_wgrad_kernels import Guarded
from tests.tile_vm_model import own_error_bound
from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp import packing as pk

pytestmark = pytest.mark.gpu

VQN_EARG, VQN_ESHAPE = -1, -2
MARGIN, POISON = 64, 7.0e4                      # floats of a finite poison value before and behind the input
ENTRY = {'f32': 'vqn_mlp_chain_fwd', 'f16s': 'vqn_mlp_chain_fwd_f16s'}
OWN = '#float32_restatement_own_error'


def _n_big():
    return cc.n_big(torch.cuda.get_device_properties(0).multi_processor_count)


def _runs():
    out = []
    for c in cc.CASES:
        for mode in c['engines']:
            counts = [33] + ([1, 31, 32] if c['name'] in cc.MORE_POINT_COUNTS else []) + (['big'] if c['name'] in cc.BIG_CASES else [])
            out += [(c['name'], mode, n) for n in counts]
    return out


def _upload(x, shift=0):
    """x on the device between two margins of POISON, `shift` floats off the 16-byte grid -> (buffer, the [N, stride] view of x)"""
    buf = torch.full((x.size + 2 * MARGIN + shift,), POISON, dtype=torch.float32)
    buf[MARGIN + shift:MARGIN + shift + x.size] = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1)
    buf = buf.cuda()
    view = buf[MARGIN + shift:MARGIN + shift + x.size].view(x.shape)
    assert view.data_ptr() % 16 == 4 * (shift % 4)
    return buf, view


@functools.lru_cache(maxsize=None)
def _reference(name, kind, N):
    """(data, float64 outs, float32 outs, float64 tensors, bounds): computed once, shared, never written to"""
    case = cc.BY_NAME[name]
    data = cc.make_data(case, kind, N)
    o64, t64, bounds = cc.reference(case, data, want_bounds=True)
    o32, _, _ = cc.reference(case, data, prec='f32')
    return data, o64, o32, t64, bounds


@functools.lru_cache(maxsize=None)
def _built(name, kind, mode):
    case = cc.BY_NAME[name]
    b = cc.build(case, cc.make_data(case, kind, 1), mode)           # (the weights do not depend on N)
    b['wbuf_dev'] = b['wbuf'].cuda()
    return b


_RESULTS = {}


def _run(name, mode, kind, N, shift=0):
    """one launch through the package's entry -> the slots' [N, width] arrays; asserts the launch count, the guards, the written set"""
    data = _reference(name, kind, N)[0]
    built = _built(name, kind, mode)
    keep, x = _upload(data['x'], shift)
    outs = [Guarded(N * ld) for ld in built['lds']]
    with launches() as rec:
        _C.mlp_chain_fwd(built['desc'], built['wbuf_dev'], x, built['widths'], mode=mode,
                         outs=[g.view(N, ld) for g, ld in zip(outs, built['lds'])], lds=built['lds'])
    assert rec.counts == {ENTRY[mode]: 1}, rec.counts
    got = []
    for s, (g, w, ld) in enumerate(zip(outs, built['widths'], built['lds'])):
        assert g.intact(), f'{name} {mode}: written outside slot {s}'
        full = g.view(N, ld).cpu().numpy()
        nan = np.isnan(full)
        assert not nan[:, :w].any(), f'{name} {mode} slot {s}: {int(nan[:, :w].sum())} elements not written (or NaN read from the padding)'
        assert nan[:, w:].all(), f'{name} {mode} slot {s}: the ld - width tail was written'
        got.append(full[:, :w].copy())
    return got


def _f16_exact(case, slot, t64):
    """every tensor entering a layer on the way to `slot` is an integer below 2^11 in the reference: exact in one f16"""
    names = set()
    for j in cc.upstream(case, cc.slots(case)[slot][0]):
        names |= set(case['layers'][j]['src'])
    return all(np.array_equal(t64[n], np.round(t64[n])) and np.abs(t64[n]).max() < 2 ** 11 for n in names)


def _compare(test, name, mode, kind, N, got, label=None):
    """The yardstick of a run of fewer than 33 points is the case's 33-point data set, whose first N rows the run uses (asserted): per
    feature, the float32 restatement's own error and max|model| over those 33 points -- the bound the same element is held to in the
    N = 33 run.  A feature of ONE point has no statistic of its own: max|model| would be the one value, which cancellation can make
    arbitrarily small against the terms of its sum, and the restatement's error at one point can be zero by chance."""
    case = cc.BY_NAME[name]
    Ny = max(N, 33)
    data, o64, o32, t64, bounds = _reference(name, kind, Ny)
    assert np.array_equal(data['x'][:N], _reference(name, kind, N)[0]['x'], equal_nan=True)
    exact = cc.exact_slots(case) if kind == 'int' else []
    n_exact = 0
    for s, g in enumerate(got):
        v64, v32 = o64[s], o32[s]
        assert g.shape == v64[:N].shape
        if s in exact and (mode == 'f32' or _f16_exact(case, s, t64)):
            assert bounds[s] < 2 ** 24, f'{name} slot {s}: bound {bounds[s]} is no proof of exactness'
            bad = g.astype(np.float64) != v64[:N]
            assert not bad.any(), f'{name} {mode} {kind} N={label or N} slot {s}: {int(bad.sum())} of {bad.size} elements differ from the exact ' \
                                  f'value (first at {tuple(int(i[0]) for i in np.nonzero(bad))})'
            n_exact += 1
            continue
        worst = None
        scale = float(np.abs(v64).max())
        for f in range(v64.shape[1]):
            bound, own = own_error_bound(v64[:, f], v32[:, f])
            if mode == 'f16s':
                bound = 4 * own + 2e-6 * scale
            err = float(np.max(np.abs(g[:, f].astype(np.float64) - v64[:N, f])))
            rec = (err / bound if bound > 0 else (0.0 if err == 0 else np.inf), err, bound, own, f)
            worst = rec if worst is None or rec[0] > worst[0] else worst
        _, err, bound, own, f = worst
        key = f'{name}/{mode}/{kind}/N={label or N}/slot{s}'
        record_observed(test, key + OWN, own, bound)
        record_observed(test, key, err, bound)
        assert err <= bound, f'{key}: feature {f}: error {err:.3e} above {bound:.3e} (float32 restatement: {own:.3e})'
    return n_exact


@pytest.mark.parametrize('name,mode,n', _runs())
def test_program_against_the_float64_reference(name, mode, n):
    N = _n_big() if n == 'big' else n
    if n == 'big':
        assert (N + 31) // 32 >= 4 * torch.cuda.get_device_properties(0).multi_processor_count + 1 and N % 32
    case = cc.BY_NAME[name]
    for kind in ('int', 'real'):
        got = _run(name, mode, kind, N)
        _RESULTS[name, mode, kind, n] = [g[:33].copy() for g in got]
        n_exact = _compare('test_program_against_the_float64_reference', name, mode, kind, N, got, label=n)
        if kind == 'int' and mode == 'f32':
            assert n_exact == len(cc.exact_slots(case))
        if n != 33 and n != 'big':                                  # the same points as the first rows of the 33-point run: the same bits
            full = _RESULTS.get((name, mode, kind, 33)) or _run(name, mode, kind, 33)
            for s, (a, b) in enumerate(zip(got, full)):
                assert np.array_equal(a.view(np.int32), b[:n].view(np.int32)), f'{name} {mode} {kind} N={n} slot {s}: not the bits of N=33'
    if name.startswith('eight_waves'):
        assert _built(name, 'real', mode)['plan'].n_waves == 8


def test_integer_cases_are_exact_on_the_f16s_engine_too():
    """the condition of the f16s equality (integers below 2^11 on the whole way) holds for every slot that is exact on the f32 engine:
    the f16s runs above compare those for equality, not within a tolerance"""
    n = 0
    for case in cc.CASES:
        if 'f16s' in case['engines']:
            t64 = _reference(case['name'], 'int', 33)[3]
            for s in cc.exact_slots(case):
                assert _f16_exact(case, s, t64), (case['name'], s)
                n += 1
    assert n >= 7


@pytest.mark.parametrize('name', cc.BIG_CASES)
@pytest.mark.parametrize('mode', ('f32', 'f16s'))
def test_first_rows_do_not_depend_on_the_launch_size(name, mode):
    for kind in ('int', 'real'):
        small = _RESULTS.get((name, mode, kind, 33)) or _run(name, mode, kind, 33)
        big = _RESULTS.get((name, mode, kind, 'big')) or _run(name, mode, kind, _n_big())
        x33, xbig = _reference(name, kind, 33)[0]['x'], _reference(name, kind, _n_big())[0]['x']
        assert np.array_equal(x33, xbig[:33], equal_nan=True)
        for s, (a, b) in enumerate(zip(small, big)):
            assert np.array_equal(a[:33].view(np.int32), b[:33].view(np.int32)), f'{name} {mode} {kind} slot {s}'


@pytest.mark.parametrize('mode', ('f32', 'f16s'))
def test_unaligned_input_is_accepted_where_the_rows_are_read_by_scalars(mode):
    """in_stride % 4 != 0: `in` 4 bytes off the 16-byte grid is taken, and the result is still the reference's"""
    got = _run('odd_stride', mode, 'int', 33, shift=1)
    assert _compare('test_unaligned_input_is_accepted_where_the_rows_are_read_by_scalars', 'odd_stride', mode, 'int', 33, got) == 1
    got = _run('odd_stride', mode, 'real', 33, shift=1)
    _compare('test_unaligned_input_is_accepted_where_the_rows_are_read_by_scalars', 'odd_stride', mode, 'real', 33, got)


# ------------------------------------------------------------------------------------------------------------------- refusals
def _last_error():
    return _C.lib().vqn_last_error().decode()


class RawCall:
    """the C entry itself on the `four_slots` program (or `built`), every argument overridable; outputs with 4 floats to spare"""

    def __init__(self, mode, name='four_slots', built=None, N=33):
        case = cc.BY_NAME[name]
        self.mode, self.N = mode, N
        self.built = built or _built(name, 'real', mode)
        self.desc = np.ascontiguousarray(self.built['desc'], np.int32).copy()
        self.wbuf = self.built['wbuf_dev'] if 'wbuf_dev' in self.built else self.built['wbuf'].cuda()
        self.keep, self.x = _upload(cc.make_data(case, 'real', N)['x'])
        self.lds = list(self.built['lds'])
        self.outs = [Guarded(N * ld, spare=4) for ld in self.lds]
        self.ptrs = [g.ptr for g in self.outs]
        self.in_ptr = self.x.data_ptr()

    def __call__(self, N=None):
        args = []
        for i in range(4):
            args += [self.ptrs[i], self.lds[i]] if i < len(self.ptrs) else [None, 0]
        with launches() as rec:
            rc = getattr(_C.lib(), ENTRY[self.mode])(self.desc.ctypes.data, self.wbuf.data_ptr(), self.in_ptr, self.N if N is None else N,
                                                     *args, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, rec.counts

    def nothing_written(self):
        return all(bool(torch.isnan(g.full).all()) for g in self.outs)

    def refused(self, rc_want, words):
        rc, counts = self()
        assert rc == rc_want, f'return code {rc}: {_last_error()}'
        assert words in _last_error() and ENTRY[self.mode] + ':' in _last_error(), _last_error()
        assert counts == {} and self.nothing_written()


def _resident_over_program():
    """raw 32 -> 128 relu -> 128 sigmoid written over its K rows -> small: every row count is even, so under the f16s rules nothing
    but the in-place layer is wrong with it"""
    b = pk.ChainBuilder('raw', 32)
    x = b.input
    y0 = b.dense('0', [x], 128, 'relu', keep=[x])
    y1 = b.dense('1', [y0], 128, 'sigmoid', keep=[x], over=y0)
    b.dense_small('2', [y1, x], 2, 'none', 0)
    plan = b.build()
    rng = np.random.default_rng(11)
    params = {k: (torch.from_numpy(rng.normal(size=s).astype(np.float32)), torch.zeros(s[1]))
              for k, s in (('0', (32, 128)), ('1', (128, 128)), ('2', (160, 2)))}
    wbuf, desc = plan.pack(params)
    return dict(plan=plan, desc=desc, wbuf=wbuf, widths=[2], lds=[2])


@pytest.mark.parametrize('mode', ('f32', 'f16s'))
def test_chain_fwd_refusals(mode):
    call = RawCall(mode)
    rc, _ = call()
    assert rc == 0 and not call.nothing_written(), 'the unpatched call must run'
    # a written slot null
    call = RawCall(mode); call.ptrs[1] = None
    call.refused(VQN_EARG, 'an output the descriptor writes is null')
    # ld one below the width: a GEMM slot (33 wide), a small slot (4 wide)
    for slot in (1, 2):
        call = RawCall(mode); call.lds[slot] -= 1
        call.refused(VQN_EARG, "output leading dimension smaller than the layer's width")
    # a GEMM output with ld % 4 == 0, 4 bytes off
    call = RawCall(mode); assert call.lds[0] % 4 == 0; call.ptrs[0] += 4
    call.refused(VQN_EARG, 'outputs with ld % 4 == 0 must be 16-byte aligned')
    # in 4 bytes off with in_stride % 4 == 0
    call = RawCall(mode); assert call.desc[8] % 4 == 0; call.in_ptr += 4
    call.refused(VQN_EARG, 'in must be 16-byte aligned')
    # one field of the descriptor broken
    call = RawCall(mode); call.desc[7] = 5
    call.refused(VQN_ESHAPE, 'invalid chain descriptor (check 2)')
    call = RawCall(mode); call.desc[16 + 16 * 1 + 10] = 4                         # out_slot of layer 1 past the table
    call.refused(VQN_ESHAPE, 'invalid chain descriptor (check 13)')
    # N == 0: nothing to do, and no complaint about pointers nobody will follow
    call = RawCall(mode); call.in_ptr = None; call.ptrs = [None] * 4
    rc, counts = call(N=0)
    assert rc == 0 and counts == {} and call.nothing_written()


def test_in_place_program_is_refused_by_the_f16s_entry():
    built = _resident_over_program()
    ok = RawCall('f32', name='sixteen_layers', built=built)                         # (the case only sizes the input: 32 columns)
    rc, _ = ok()
    assert rc == 0 and not ok.nothing_written()
    RawCall('f16s', name='sixteen_layers', built=built).refused(VQN_ESHAPE, 'invalid chain descriptor (check 16)')


# ---- vqn_mlp_chain_vq_fwd
def _pack(b, shapes, seed):
    rng = np.random.default_rng(seed)
    params = {k: (torch.from_numpy((rng.normal(size=s) / np.sqrt(s[0])).astype(np.float32)), torch.zeros(s[1])) for k, s in shapes.items()}
    wbuf, desc = b.build().pack(params)
    return np.ascontiguousarray(desc, np.int32), wbuf.cuda()


def _program_a(extra=None):
    """posenc(1) 9 -> 256 relu to slot 0 (z); extra 'dense': a second layer reading x (slot 1); 'reload': the input again"""
    b = pk.ChainBuilder('posenc', 9, n_freqs=1)
    x = b.input
    shapes = {'z': (9, 256)}
    z = b.dense('z', [x], 256, 'relu', keep=[x] if extra else [], out_slot=0)
    if extra == 'dense':
        b.dense('e', [x], 32, 'relu', keep=[z], out_slot=1)
        shapes['e'] = (9, 32)
    elif extra == 'reload':
        b.reload_input(keep=[z])
    return _pack(b, shapes, 1)


def _program_b(small_first=False):
    b = pk.ChainBuilder('raw', 256)
    x = b.input
    if small_first:
        b.dense_small('s', [x], 3, 'sigmoid', 0)
        return _pack(b, {'s': (256, 3)}, 2)
    y = b.dense('h', [x], 32, 'relu')
    b.dense_small('s', [y], 3, 'sigmoid', 0)
    return _pack(b, {'h': (256, 32), 's': (32, 3)}, 2)


class VqCall:
    N, K = 33, 15

    def __init__(self, a=None, b=None, frag_K=15):
        self.da, self.wa = a or _program_a()
        self.db, self.wb = b or _program_b()
        self.da, self.db = self.da.copy(), self.db.copy()
        rng = np.random.default_rng(3)
        self.keep, self.x = _upload(rng.uniform(-1, 1, (self.N, 3)).astype(np.float32))
        self.frags = _C.vq_codebook_frags(torch.from_numpy(rng.uniform(0, 1, (256, frag_K)).astype(np.float32)).cuda())
        self.oa = [Guarded(self.N * 256), Guarded(self.N * 32)]
        self.ob = [Guarded(self.N * 3)]
        self.pa, self.lda = [self.oa[0].ptr, self.oa[1].ptr, None, None], [256, 32, 0, 0]
        self.pb, self.ldb = [self.ob[0].ptr, None, None, None], [3, 0, 0, 0]
        self.idx = torch.full((self.N,), -1, dtype=torch.int64, device='cuda')
        self.ste = Guarded(self.N * 256, spare=4)
        self.ste_ptr = self.ste.ptr
        self.loss = torch.full((1,), 1.0, device='cuda')
        self.counts = torch.full((80,), 7.0, device='cuda')
        self.ws = torch.zeros(4096, device='cuda')

    def __call__(self, N=None, K=None):
        N = self.N if N is None else N
        ptrs = lambda ps: (ctypes.c_void_p * 4)(*ps)
        i32 = lambda v: (ctypes.c_int32 * 4)(*v)
        with launches() as rec:
            rc = _C.lib().vqn_mlp_chain_vq_fwd(self.da.ctypes.data, self.wa.data_ptr(), self.db.ctypes.data, self.wb.data_ptr(), self.x.data_ptr(), N,
                                               ptrs(self.pa), i32(self.lda), ptrs(self.pb), i32(self.ldb), self.frags.data_ptr(),
                                               self.K if K is None else K, 1e-6, 1.0 / (256 * max(N, 1)), self.idx.data_ptr(), self.ste_ptr,
                                               self.loss.data_ptr(), self.counts.data_ptr(), self.ws.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, rec.counts

    def nothing_written(self):
        return all(bool(torch.isnan(g.full).all()) for g in self.oa + self.ob + [self.ste]) and bool((self.idx == -1).all()) \
            and float(self.loss) == 1.0

    def refused(self, rc_want, words, **kw):
        rc, counts = self(**kw)
        assert rc == rc_want, f'return code {rc}: {_last_error()}'
        assert words in _last_error() and 'vqn_mlp_chain_vq_fwd:' in _last_error(), _last_error()
        assert counts == {} and self.nothing_written()


def _layer(desc, l, field):
    return 16 + 16 * l + field


def test_chain_vq_fwd_refusals():
    call = VqCall(a=_program_a('dense'))
    rc, _ = call()
    assert rc == 0, _last_error()
    assert not bool(torch.isnan(call.oa[0].view(33, 256)).any()) and not bool(torch.isnan(call.ob[0].view(33, 3)).any())
    assert bool((call.idx >= 0).all()) and float(call.counts[:15].sum()) == 33.0

    VqCall(frag_K=64).refused(VQN_ESHAPE, 'K <= 64', K=65)              # (fragments as large as the entry takes)
    call = VqCall(); call.da[7] = 8
    call.refused(VQN_ESHAPE, 'both programs must be 4-wave programs')
    call = VqCall(a=_program_a('dense')); call.da[_layer(call.da, 0, 10)] = 2; call.pa[2] = call.pa[0]
    call.refused(VQN_ESHAPE, 'program A must leave a 256-feature z in LDS through output slot 0')
    call = VqCall(); call.db[2] = 255
    call.refused(VQN_ESHAPE, 'program B must take a raw 256-feature input')
    call = VqCall()                                                               # program B with the input image again at its end
    n = int(call.db[0]); call.db[0] = n + 1
    call.db[16 + 16 * n: 16 + 16 * n + 12] = [2, 0, 0, 0, 0, 0, 0, int(call.db[4]), 0, -1, -1, 0]
    call.refused(VQN_ESHAPE, 'program B must keep its input resident')
    VqCall(b=_program_b(small_first=True)).refused(VQN_ESHAPE, 'both programs must start with a GEMM layer')
    # a later layer of A over z (its own K rows are the input's: only z is at stake)
    call = VqCall(a=_program_a('dense'))
    z0 = int(call.da[_layer(call.da, 0, 7)])
    k0, k1 = int(call.da[_layer(call.da, 1, 3)]), int(call.da[_layer(call.da, 1, 3)]) + int(call.da[_layer(call.da, 1, 4)])
    assert k1 <= z0 or k0 >= z0 + 32
    call.da[_layer(call.da, 1, 7)] = z0
    call.refused(VQN_ESHAPE, 'a layer of program A overwrites z before the VQ step')
    # a reload of A over z
    call = VqCall(a=_program_a('reload'))
    assert call.da[_layer(call.da, 1, 0)] == 2
    call.da[_layer(call.da, 1, 7)] = int(call.da[_layer(call.da, 0, 7)])
    call.refused(VQN_ESHAPE, 'program A reloads its input over z')
    call = VqCall(); call.ste_ptr += 4
    call.refused(VQN_EARG, 'ste must be 16-byte aligned')


def test_chain_vq_fwd_of_no_points_gives_nan_loss_and_zero_counts():
    call = VqCall()
    rc, counts = call(N=0)
    assert rc == 0 and counts == {}
    assert bool(torch.isnan(call.loss).all()) and bool((call.counts[:15] == 0).all()) and bool((call.counts[15:] == 7).all())
    assert all(bool(torch.isnan(g.full).all()) for g in call.oa + call.ob + [call.ste]) and bool((call.idx == -1).all())
