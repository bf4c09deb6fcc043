"""The loss side of the reflectance training step, entry point by entry point: the ten of csrc/decomp_loss.hip and the four of
csrc/elementwise.hip, each called through its `_C` wrapper at its declared limits and compared element by element with the
references of tests/loss_kernel_cases.py -- float64 under the project's yardstick (kernel_cases.yardstick: as close to float64 as
the float32 statement is, max within 3x, rms within 2x, floor 8 float32 epsilons of the largest entry), or the statement's own bits
where the kernel promises them.  Every buffer a wrapper allocates starts as NaN, so an element no thread wrote shows, and every
test counts its launches.  CUs: torch.cuda.get_device_properties(0).multi_processor_count.

Observed figures, bounds and the float32 references' own errors: profiles/observed_errors_loss_kernels.json.  RAISED below names
the tensors that are held to a raised factor, each with its arithmetic reason."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import loss_kernel_cases as lc
from tests.gpu_util import launches
from vqnerf_release_amd import _C

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NAN = float('nan')

# Report key of ONE tensor of ONE case -> yardstick arguments, where a correct kernel passes the default factors.
# The code-separation kernels sum a pair's squared distance as one in-order chain of D fmaf, the float32 statement (torch) pairwise:
# ~sqrt(D) u against ~u, so the factor is 3 sqrt(D) (loss_kernel_cases.sim_chain_factor has the arithmetic).  Listed are exactly the
# tensors whose error exceeds the default bound -- both read the codebook from global memory (D K > 12288); the LDS-staged cases run
# the same chain and stay under the default bound, as does `dist` at (256, 49).
RAISED = {
    'D1028-K256/dist': lc.sim_chain_factor(1028),
    'D1028-K256/term': lc.sim_chain_factor(1028),
    'D1028-K256/g_cb': lc.sim_chain_factor(1028),
    'D256-K49/g_cb': lc.sim_chain_factor(256),
}


class _NanTorch:
    """Stands in for the `torch` that vqnerf_release_amd._C sees while a test runs: every floating-point buffer a wrapper allocates
    for a kernel's output is NaN before the launch."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*a, **k):
        t = torch.empty(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t

    @staticmethod
    def empty_like(*a, **k):
        t = torch.empty_like(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t


@pytest.fixture(autouse=True)
def nan_outputs(monkeypatch):
    monkeypatch.setattr(_C, 'torch', _NanTorch())


def CUs():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def check(rep, key, got, ref32, ref64):
    return rep.check(key, got, ref32, ref64, **RAISED.get(key, {}))


def same_bits(rep, key, got, want):
    rep.exact(key, lc.bits(got), lc.bits(want))


# ------------------------------------------------------------------------------------------- vqn_decomp_loss_fwd / _bwd
def _loss_case(rep, key, inp, nerf, w=lc.W, use_z=True, use_spec=True):
    r64, r32 = (lc.loss_reference(inp, nerf, dt, w, use_z, use_spec) for dt in (F64, F32))
    t = {k: dev(inp[k]) for k in ('rgb_pred', 'vq_rgb', 'rgb_gt', 'z', 'spec', 'rough', 'g_terms')}
    args = (t['rgb_pred'], t['vq_rgb'], t['rgb_gt'], t['z'] if use_z else None, t['spec'] if use_spec else None, t['rough'], nerf, w)
    with launches() as rec:
        terms = _C.decomp_loss_fwd(*args)
        grads = _C.decomp_loss_bwd(*args, t['g_terms'])
    assert rec.counts == {'vqn_decomp_loss_fwd': 1, 'vqn_decomp_loss_bwd': 1}, rec.counts
    terms = host(terms)
    N = terms.shape[0]
    for c, name in enumerate(lc.TERMS):                           # (lambert is ~3e-4 beside a loss of ~1.5: one bound per column)
        check(rep, f'{key}/{name}', terms[:, c], r32['terms'][:, c], r64['terms'][:, c])
    got = {}
    for name, g in zip(('g_pred', 'g_vq', 'g_z', 'g_spec'), grads):
        if r64[name] is None:
            assert g is None, name
            continue
        got[name] = host(g)
        check(rep, f'{key}/{name}', got[name], r32[name], r64[name])
    if 'g_spec' in got:                                           # non-zero at the first maximum only
        first = np.zeros((N, 3), bool)
        first[np.arange(N), np.argmax(inp['spec'], -1)] = True
        rep.exact(f'{key}/g_spec off the first maximum', got['g_spec'][~first], np.zeros(2 * N, np.float32))
    if N % 2:                                                     # the lone last point has no pair
        rep.exact(f'{key}/lone point chr_smooth', terms[N - 1, 3], np.float32(0))
        if 'g_z' in got:
            rep.exact(f'{key}/lone point g_z', got['g_z'][N - 1], np.zeros_like(got['g_z'][N - 1]))
    return terms, got


@pytest.mark.parametrize('nerf', [True, False], ids=['nerf', 'hw'])
@pytest.mark.parametrize('D', lc.LOSS_D)
def test_decomp_loss_terms_and_adjoints_vs_float64(D, nerf):
    """D = 256 has an unrolled branch of its own, every other D takes the generic loop (ragged against the 64 lanes at 4, 60, 252,
    260); odd N ends in a point without a pair; every term column has an upstream gradient of its own."""
    rep = lc.Report('test_decomp_loss_terms_and_adjoints_vs_float64')
    for N in lc.LOSS_N:
        _loss_case(rep, f'N{N}-D{D}-{"nerf" if nerf else "hw"}', lc.loss_inputs(N, D), nerf)
    rep.finish()


def test_decomp_loss_second_grid_pass():
    """N = 2 * 4 * 16 CUs + 3: two pairs more than one pass of the capped grid holds, the last of them a lone point."""
    rep = lc.Report('test_decomp_loss_second_grid_pass')
    N = 2 * 4 * 16 * CUs() + 3
    _loss_case(rep, f'N{N}-D64-nerf', lc.loss_inputs(N, 64), True)
    rep.finish()


@pytest.mark.parametrize('N,D', [(9, 256), (3, 60)])
def test_decomp_loss_absent_inputs_and_zero_weights(N, D):
    rep = lc.Report('test_decomp_loss_absent_inputs_and_zero_weights')
    inp = lc.loss_inputs(N, D)
    for name, kw in (('no_z', dict(use_z=False)), ('no_spec', dict(use_spec=False)), ('w_smooth0', dict(w=dict(lc.W, smooth=0.0))),
                     ('w_lambert0', dict(w=dict(lc.W, lambert=0.0)))):
        terms, got = _loss_case(rep, f'N{N}-D{D}-{name}', inp, True, **kw)
        col = 3 if name in ('no_z', 'w_smooth0') else 4
        rep.exact(f'{name}/term column', terms[:, col], np.zeros(N, np.float32))
        if name == 'w_smooth0':
            rep.exact(f'{name}/g_z', got['g_z'], np.zeros((N, D), np.float32))
        if name == 'w_lambert0':
            rep.exact(f'{name}/g_spec', got['g_spec'], np.zeros((N, 3), np.float32))
    rep.finish()


# --------------------------------------------------------------------------- vqn_sim_smooth_fwd / _bwd, vqn_codebook_prep
def _sim_run(cb_t):
    with launches() as rec:
        out = _C.sim_smooth_fwd(cb_t, lc.SIM_W)
        g_cb = _C.sim_smooth_bwd(cb_t, out, dev(np.float32(lc.SIM_G)), lc.SIM_W)
    assert rec.counts == {'vqn_sim_smooth_fwd': 1, 'vqn_sim_smooth_bwd': 1}, rec.counts
    return host(out), host(g_cb)


@pytest.mark.parametrize('D,K', lc.SIM_CASES)
def test_sim_smooth_vs_float64(D, K):
    """(252, 15): the staged copy with the D % 16 tail; (256, 33) and (256, 48): staged, more than one pair per thread, 48 at the
    12288-float boundary; (256, 49): one column past it, read from global memory; (33, 5), (7, 2): odd sizes, the scalar staging copy;
    (1028, 256): the K limit, 128 pairs per thread, the backward's 1024-block cap."""
    rep = lc.Report('test_sim_smooth_vs_float64')
    cb = lc.sim_inputs(D, K)
    r64, r32 = lc.sim_reference(cb, F64), lc.sim_reference(cb, F32)
    out, g_cb = _sim_run(dev(cb))
    key = f'D{D}-K{K}'
    check(rep, f'{key}/dist', out[1:2], r32['dist'], r64['dist'])
    check(rep, f'{key}/term', out[0:1], r32['term'], r64['term'])
    rep.exact(f'{key}/pair', out[2:4], np.array(r64['pair'], np.float32))
    check(rep, f'{key}/g_cb', g_cb, r32['g_cb'], r64['g_cb'])
    rep.exact(f'{key}/g_cb outside the pair', np.delete(g_cb, r64['pair'], axis=1), np.zeros((D, K - 2), np.float32))
    rep.finish()


def test_sim_smooth_unaligned_codebook_takes_the_scalar_copy():
    """(256, 15) on a view that starts 4 bytes into its buffer: the same bits as on the aligned tensor."""
    rep = lc.Report('test_sim_smooth_unaligned_codebook_takes_the_scalar_copy')
    D, K = lc.SIM_UNALIGNED
    cb = lc.sim_inputs(D, K)
    buf = torch.zeros(D * K + 1, device='cuda')
    view = buf[1:].view(D, K)
    view.copy_(dev(cb))
    aligned = dev(cb)
    assert view.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0 and view.is_contiguous()
    out_a, g_a = _sim_run(aligned)
    out_u, g_u = _sim_run(view)
    same_bits(rep, 'out', out_u, out_a)
    same_bits(rep, 'g_cb', g_u, g_a)
    r64, r32 = lc.sim_reference(cb, F64), lc.sim_reference(cb, F32)
    key = f'unaligned-D{D}-K{K}'
    check(rep, f'{key}/dist', out_u[1:2], r32['dist'], r64['dist'])
    check(rep, f'{key}/term', out_u[0:1], r32['term'], r64['term'])
    rep.exact(f'{key}/pair', out_u[2:4], np.array(r64['pair'], np.float32))
    check(rep, f'{key}/g_cb', g_u, r32['g_cb'], r64['g_cb'])
    rep.exact(f'{key}/g_cb outside the pair', np.delete(g_u, r64['pair'], axis=1), np.zeros((D, K - 2), np.float32))
    rep.finish()


@pytest.mark.parametrize('same_thread', [True, False], ids=['one_thread', 'two_threads'])
def test_sim_smooth_reports_the_smaller_pair_index_on_a_tie(same_thread):
    cb, _, pairs, want = lc.sim_tie_case(same_thread)
    out, g_cb = _sim_run(dev(cb))
    assert out[1] == np.float32(1.0 / 64.0), out
    assert (int(out[2]), int(out[3])) == want, (out, pairs)
    assert not np.delete(g_cb, want, axis=1).any() and np.isfinite(g_cb).all()


def test_sim_smooth_nan_entry_gives_a_nan_term():
    cb = lc.sim_inputs(256, 15)
    cb[100, 7] = NAN
    with launches() as rec:
        out = host(_C.sim_smooth_fwd(dev(cb), lc.SIM_W))
    assert rec.counts == {'vqn_sim_smooth_fwd': 1}
    assert np.isnan(out[0]) and np.isnan(out[1]) and 7 in (int(out[2]), int(out[3])), out


@pytest.mark.parametrize('D', lc.PREP_D)
def test_codebook_prep_both_forms_vs_float64(D):
    """D = 515: every thread walks its column in up to three steps of 256; K = 70: more workgroups than the shipped 64 codes."""
    rep = lc.Report('test_codebook_prep_both_forms_vs_float64')
    for K in lc.PREP_K:
        raw, gy = lc.prep_inputs(D, K)
        (cb64, g64, s64), (cb32, g32, _) = lc.prep_reference(raw, gy, F64), lc.prep_reference(raw, gy, F32)
        over = s64 > lc.PREP_EPS
        with launches() as rec:
            cb = _C.codebook_prep(dev(raw))
            g = _C.codebook_prep(dev(raw), dev(gy))
        assert rec.counts == {'vqn_codebook_prep': 2}, rec.counts
        for cols, name in ((over, 'columns_over_eps'), (~over, 'columns_under_eps')):      # (a clamped column's entries of g_raw are
            if cols.any():                                                               #  ~1000 x larger: bounded on their own)
                check(rep, f'D{D}-K{K}/codebook/{name}', host(cb)[:, cols], cb32[:, cols], cb64[:, cols])
                check(rep, f'D{D}-K{K}/g_raw/{name}', host(g)[:, cols], g32[:, cols], g64[:, cols])
    rep.finish()


# ------------------------------------------------------------------------------------------------------ vqn_vq_ema_update
@pytest.mark.parametrize('K', lc.EMA_K)
def test_ema_update_four_calls(K):
    """K > 256: every thread of the one workgroup takes several codes; K = 1024: the declared limit.  Counters exact, `hidden` the
    numpy float32 statement's bits, `average` and `update` against float64, unused codes keep their codebook column to the bit."""
    rep = lc.Report('test_ema_update_four_calls')
    for D in lc.EMA_D:
        inp = lc.ema_inputs(K, D)
        r64, r32, hid = lc.ema_reference(inp, F64), lc.ema_reference(inp, F32), lc.ema_hidden_f32(inp)
        state = lambda shape: SimpleNamespace(hidden=torch.zeros(shape, device='cuda'), average=torch.full(shape, NAN, device='cuda'),
                                              counter=torch.zeros((), dtype=torch.int64, device='cuda'))
        ema_cs, ema_dw = state((K,)), state((D, K))
        cb = dev(inp['cb'])
        for c, call in enumerate(inp['calls']):
            with launches() as rec:
                update = host(_C.vq_ema_update(dev(call['counts']), dev(call['dw']), cb, lc.EMA_DECAY, lc.EMA_EPS, ema_cs, ema_dw))
            assert rec.counts == {'vqn_vq_ema_update': 1}, rec.counts
            assert int(ema_cs.counter) == int(ema_dw.counter) == c + 1 == r64[c]['counter']
            key = f'K{K}-D{D}-call{c + 1}'
            same_bits(rep, f'{key}/hidden_cs', host(ema_cs.hidden), hid[c][0])
            same_bits(rep, f'{key}/hidden_dw', host(ema_dw.hidden), hid[c][1])
            check(rep, f'{key}/average_cs', host(ema_cs.average), r32[c]['average_cs'], r64[c]['average_cs'])
            check(rep, f'{key}/average_dw', host(ema_dw.average), r32[c]['average_dw'], r64[c]['average_dw'])
            check(rep, f'{key}/update', update, r32[c]['update'], r64[c]['update'])
            unused = call['counts'] == 0
            same_bits(rep, f'{key}/unused columns', update[:, unused], inp['cb'][:, unused])
    rep.finish()


# ------------------------------------------------------------------------------ vqn_l2_normalize_rows_bwd, vqn_vq_train_bwd
@pytest.mark.parametrize('D', lc.ROW_D)
def test_row_backwards_vs_float64_and_the_two_kernel_sequence(D):
    """D = 252, 260, 1020: the last group of 64 float4 lanes is ragged; D = 4: one lane.  Rows over and under the eps clamp are
    bounded separately (the clamped rows' entries are ~1000 x larger).  vqn_vq_train_bwd == vqn_l2_normalize_rows_bwd after
    vqn_vq_ste_loss_bwd at g_loss * c, bit for bit."""
    rep = lc.Report('test_row_backwards_vs_float64_and_the_two_kernel_sequence')
    for N in lc.ROW_N:
        inp = lc.row_inputs(N, D)
        over = lc.row_sums(inp['x']) > lc.ROW_EPS
        t = {k: dev(v) for k, v in inp.items()}
        gl = dev(np.float32(lc.ROW_GL))

        def both(key, got, r32, r64):
            check(rep, f'{key}/rows_over_eps', got[over], r32[over], r64[over])
            if not over.all():
                check(rep, f'{key}/rows_under_eps', got[~over], r32[~over], r64[~over])

        with launches() as rec:
            got = host(_C.l2_normalize_rows_bwd(t['x'], t['g'], lc.ROW_EPS))
            fused, seq = {}, {}
            for c in (1.0, 0.1):
                glc = dev(np.float32(lc.ROW_GL) * np.float32(c))                  # g_loss * c as autograd's own multiplication rounds it
                for ste in (True, False):
                    gs = t['gs'] if ste else None
                    fused[c, ste] = host(_C.vq_train_bwd(t['x'], t['xn'], t['q'], gs, gl, lc.ROW_EPS, loss_post=c))
                    seq[c, ste] = host(_C.l2_normalize_rows_bwd(t['x'], _C.vq_ste_loss_bwd(t['xn'], t['q'], gs, glc), lc.ROW_EPS))
        assert rec.counts == {'vqn_l2_normalize_rows_bwd': 5, 'vqn_vq_train_bwd': 4, 'vqn_vq_ste_loss_bwd': 4}, rec.counts
        both(f'N{N}-D{D}/l2_bwd', got, lc.l2_bwd_reference(inp['x'], inp['g'], F32), lc.l2_bwd_reference(inp['x'], inp['g'], F64))
        for (c, ste), g in fused.items():
            key = f'N{N}-D{D}-c{c:g}-{"ste" if ste else "noste"}'
            both(f'{key}/train_bwd', g, lc.train_bwd_reference(inp, c, ste, F32), lc.train_bwd_reference(inp, c, ste, F64))
            same_bits(rep, f'{key}/train_bwd == sequence', g, seq[c, ste])
    rep.finish()


@pytest.mark.parametrize('numel', [4, 1028, 4 * 256 * 4096 + 4], ids=['4', '1028', 'past_the_block_cap'])
def test_ste_loss_bwd_is_the_numpy_statement(numel):
    rep = lc.Report('test_ste_loss_bwd_is_the_numpy_statement')
    rng = np.random.default_rng(numel)
    x, q, gs = (rng.normal(size=numel).astype(np.float32) for _ in range(3))
    with launches() as rec:
        with_gs = host(_C.vq_ste_loss_bwd(dev(x), dev(q), dev(gs), dev(np.float32(lc.ROW_GL))))
        without = host(_C.vq_ste_loss_bwd(dev(x), dev(q), None, dev(np.float32(lc.ROW_GL))))
    assert rec.counts == {'vqn_vq_ste_loss_bwd': 2}, rec.counts
    same_bits(rep, 'with g_ste', with_gs, lc.ste_loss_bwd_f32(x, q, gs, lc.ROW_GL))
    same_bits(rep, 'without g_ste', without, lc.ste_loss_bwd_f32(x, q, None, lc.ROW_GL))
    rep.finish()


# ------------------------------------------------------------------------------------------------ csrc/elementwise.hip
def _n(n):
    return 256 * 16 * CUs() + 7 if n < 0 else n


@pytest.mark.parametrize('n', [1, 257, -1], ids=['1', '257', 'past_the_grid_cap'])
@pytest.mark.parametrize('kc', [1, 3])
def test_ks_split_is_the_numpy_statement(kc, n):
    rep = lc.Report('test_ks_split_is_the_numpy_statement')
    n = _n(n)
    rng = np.random.default_rng(kc + n)
    bc, ga, gs = (rng.uniform(-1, 1, (n, 3)).astype(np.float32) for _ in range(3))
    ks = rng.uniform(0, 1, (n, kc)).astype(np.float32)
    with launches() as rec:
        albedo, spec = _C.ks_split_fwd(dev(bc), dev(ks))
        bwd = {k: _C.ks_split_bwd(dev(bc), dev(ks), dev(a), dev(s)) for k, (a, s) in dict(both=(ga, gs), no_albedo=(None, gs), no_spec=(ga, None)).items()}
    assert rec.counts == {'vqn_ks_split_fwd': 1, 'vqn_ks_split_bwd': 3}, rec.counts
    want_a, want_s = lc.ks_split_fwd_f32(bc, ks)
    same_bits(rep, 'albedo', host(albedo), want_a)
    same_bits(rep, 'spec', host(spec), want_s)
    for k, (a, s) in dict(both=(ga, gs), no_albedo=(None, gs), no_spec=(ga, None)).items():
        want_bc, want_ks = lc.ks_split_bwd_f32(bc, ks, a, s)
        same_bits(rep, f'{k}/g_basecolor', host(bwd[k][0]), want_bc)
        same_bits(rep, f'{k}/g_ks', host(bwd[k][1]), want_ks)
    rep.finish()


@pytest.mark.parametrize('with_sim', [True, False], ids=['sim', 'no_sim'])
def test_loss_total_all_flag_combinations(with_sim):
    rep = lc.Report('test_loss_total_all_flag_combinations')
    n = 257
    rng = np.random.default_rng(n)
    terms = rng.normal(size=(n, 5)).astype(np.float32)
    vqloss, sim = np.float32(0.37), np.float32(0.0123) if with_sim else None
    with launches() as rec:
        for flags in np.ndindex(2, 2, 2):
            got = host(_C.loss_total(dev(terms), dev(vqloss), dev(sim), *flags))
            same_bits(rep, f'flags{flags}', got, lc.loss_total_f32(terms, vqloss, sim, *flags))
    assert rec.counts == {'vqn_loss_total': 8}, rec.counts
    rep.finish()


def test_clip_preserve_is_the_numpy_statement():
    """on, inside and outside the bounds, NaN and +-inf (x + (clip - x) is NaN at +-inf, as in the statement), and one size past the
    grid cap"""
    rep = lc.Report('test_clip_preserve_is_the_numpy_statement')
    rng = np.random.default_rng(5)
    special = np.array([0.0, 1.0, 0.5, 1e-8, -1e-8, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, -0.25, 1.5, 3e38, -3e38, NAN, np.inf, -np.inf], np.float32)
    big = np.concatenate([special, rng.uniform(-0.5, 1.5, 256 * 16 * CUs() + 5).astype(np.float32)])
    with launches() as rec:
        got01 = host(_C.clip_preserve(dev(special), 0.0, 1.0))
        got_big = host(_C.clip_preserve(dev(big), 0.0, 1.0))
        got_other = host(_C.clip_preserve(dev(big[:1000]), -0.125, 0.75))
    assert rec.counts == {'vqn_clip_preserve': 3}, rec.counts
    assert np.isnan(got01[-3:]).all() and np.array_equal(got01[:3], special[:3]) and got01[7] == 0.0 and got01[8] == 1.0
    same_bits(rep, 'special', got01, lc.clip_preserve_f32(special, 0.0, 1.0))
    same_bits(rep, 'past the grid cap', got_big, lc.clip_preserve_f32(big, 0.0, 1.0))
    same_bits(rep, 'other bounds', got_other, lc.clip_preserve_f32(big[:1000], -0.125, 0.75))
    rep.finish()


# ----------------------------------------------------------------------------------------------------------- refusals
def test_unsupported_shapes_are_refused_before_any_launch():
    """Each call returns its error code and leaves the (NaN-filled, fully sized) output buffers untouched.  The calls go to the
    library directly (the wrappers would allocate the outputs out of sight), so `launches()`, which counts in `_C._call`, does not
    see them: a buffer that is still all NaN after a synchronise is the evidence that nothing was launched on it."""
    lib = _C.lib()
    assert bool(torch.isnan(_C.torch.empty((2, 3), dtype=torch.float32, device='cuda')).all())      # (the wrappers' own buffers, see nan_outputs)
    stream = torch.cuda.current_stream().cuda_stream
    nan = lambda *shape: torch.full(shape, NAN, device='cuda')
    ones = lambda *shape: torch.ones(shape, device='cuda')
    p = lambda t: None if t is None else t.data_ptr()
    f = ctypes.c_float
    outs = []

    def refused(rc, code, what, *out):
        assert rc == code and what.encode() in lib.vqn_last_error(), (rc, lib.vqn_last_error())
        outs.extend(out)

    for K in (1, 257):
        cb, out4, g_cb = ones(4, K), nan(4), nan(4, K)
        refused(lib.vqn_sim_smooth_fwd(p(cb), 4, K, f(0.3), p(out4), stream), -2, 'vqn_sim_smooth_fwd', out4)
        refused(lib.vqn_sim_smooth_bwd(p(cb), p(ones(4)), p(ones(1)), 4, K, f(0.3), p(g_cb), stream), -2, 'vqn_sim_smooth_bwd', g_cb)
    K = 1025
    cnt = torch.zeros(2, dtype=torch.int64, device='cuda')
    avg_cs, avg_dw, update = nan(K), nan(2, K), nan(2, K)
    refused(lib.vqn_vq_ema_update(p(ones(K)), p(ones(2, K)), p(ones(2, K)), 2, K, 0.999, f(1e-5), p(ones(K)), p(avg_cs), p(cnt[0:]),
                                  p(ones(2, K)), p(avg_dw), p(cnt[1:]), p(update), stream), -2, 'vqn_vq_ema_update', avg_cs, avg_dw, update)
    for D in (6, 1028):
        gx, gz = nan(3, D), nan(3, D)
        refused(lib.vqn_l2_normalize_rows_bwd(p(ones(3, D)), p(ones(3, D)), 3, D, f(1e-6), p(gx), stream), -2, 'vqn_l2_normalize_rows_bwd', gx)
        refused(lib.vqn_vq_train_bwd(p(ones(3, D)), p(ones(3, D)), p(ones(3, D)), None, p(ones(1)), f(1.0), 3, D, f(1e-6), p(gz), stream), -2,
                'vqn_vq_train_bwd', gz)
    g_pred, g_vq, g_z = nan(2, 3), nan(2, 3), nan(2, 64)
    w = [f(lc.W[k]) for k in ('rgb', 'chr', 'smooth', 'alpha', 'thres', 'lambert')]
    refused(lib.vqn_decomp_loss_bwd(p(ones(2, 3)), p(ones(2, 3)), p(ones(2, 3)), None, None, None, 2, 64, 1, *w, p(ones(2, 5)), p(g_pred), p(g_vq),
                                    p(g_z), None, stream), -1, 'g_z without z', g_pred, g_vq, g_z)
    alb, spec, g_bc, g_ks = nan(5, 3), nan(5, 3), nan(5, 3), nan(5, 2)
    refused(lib.vqn_ks_split_fwd(p(ones(5, 3)), p(ones(5, 2)), 2, 5, p(alb), p(spec), stream), -1, 'ks_channels', alb, spec)
    refused(lib.vqn_ks_split_bwd(p(ones(5, 3)), p(ones(5, 2)), 2, 5, p(ones(5, 3)), p(ones(5, 3)), p(g_bc), p(g_ks), stream), -1, 'ks_channels',
            g_bc, g_ks)
    torch.cuda.synchronize()
    assert int(cnt.sum()) == 0
    assert len(outs) == 18 and all(bool(torch.isnan(o).all()) for o in outs)
