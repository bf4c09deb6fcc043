"""The weight-gradient kernels on their own, window by window: vqn_wgrad_partials / _x3 / _batched, vqn_wgrad_thin_batched,
vqn_reduce_partials, vqn_wgrad_finalize and the planners of vqnerf_release_amd/wgrad.py (WgradBatch, WgradPerWeight) that cut a
weight into their windows.

Three kinds of comparison (cases, operands and references: tests/wgrad_cases.py, checked on the CPU by tests/test_wgrad_cases.py):
  * exact -- integer operands in [-8, 8] (one bf16 piece each): every partial sum is an integer below 2^24, so any summation order
    gives the same float32 and the kernel output must EQUAL the float64 contraction;
  * poison -- the operand tensors are wider than the window and NaN outside it, workspaces and destinations are NaN with 64-float
    guards: a correct kernel never reads the one and never writes past the documented extent of the other;
  * accuracy -- real-valued operands over eight decades of scale against the float64 contraction, held to the project's yardstick
    (tests/kernel_cases.yardstick: 3x max / 2x rms of the float32 torch.matmul's own error, floor 8 eps), and bit for bit between
    the single-problem and the batched entry (vqnerf_hip.h: "the same kernels, hence the same partial blocks bit for bit")."""
import math

import numpy as np
import pytest
import torch

from tests import wgrad_cases as wc
from tests.gpu_util import launches, record_observed
from tests.kernel_cases import yardstick
from vqnerf_release_amd import _C

pytestmark = pytest.mark.gpu

NAN = float('nan')
# key suffix of the figures that are NOT kernel measurements: the error of torch.matmul in float32 on the CPU against float64, recorded
# next to the bound it produces (3x max / 2x rms of itself) -- the pair of figures a changed factor would have to be justified by
REF32 = '#float32_matmul_own_error'


class Guarded:
    """`used` floats a kernel may write and `spare` floats it may not, NaN-filled, between two NaN guards of 64 floats."""

    def __init__(self, used, spare=0, fill=None):
        total, self.off = wc.guarded_layout(used, spare)
        self.used = used
        self.full = torch.full((total,), NAN, device='cuda')
        if fill is not None:
            self.full[self.off:self.off + used] = fill.reshape(-1)
        self.ptr = self.full.data_ptr() + 4 * self.off
        assert self.ptr % 16 == 0

    def view(self, *shape):
        assert math.prod(shape) <= self.used
        return self.full[self.off:self.off + math.prod(shape)].view(*shape)

    def intact(self):
        return wc.untouched(self.full, self.used)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_partials(A, B, win, npt, n_split, rowsum, x3, batched):
    """one problem through the single-problem (batched=False) or the batched entry -> (n, ws [n, rows, cols], rs [n, rows] | None);
    asserts the entry ran once, the returned count, and that nothing outside the n blocks was written."""
    a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt = win
    rows, cols = a_nt * 32, b_nt * 32
    n_exp = wc.n_blocks(npt, n_split)
    wsg = Guarded(n_exp * rows * cols, spare=(n_split - n_exp) * rows * cols)
    rsg = Guarded(n_exp * rows, spare=(n_split - n_exp) * rows) if rowsum else None
    with launches() as rec:
        if batched:
            n = _C.wgrad_partials_batched([A], [a_tiles], [a_t0], [a_nt], [B], [b_tiles], [b_t0], [b_nt], npt, n_split, [wsg.ptr],
                                          [rsg.ptr if rowsum else None], x3)
        else:
            n = _C.wgrad_partials(A, a_tiles, a_t0, a_nt, B, b_tiles, b_t0, b_nt, npt, n_split, wsg.ptr, rsg.ptr if rowsum else None, x3=x3)
    assert rec.counts.get('vqn_wgrad_partials_x3' if x3 else 'vqn_wgrad_partials') == 1, rec.counts
    assert n == n_exp
    assert wsg.intact() and (rsg is None or rsg.intact()), 'written outside the partial blocks'
    return n, wsg.view(n, rows, cols), (rsg.view(n, rows) if rowsum else None)


# ----------------------------------------------------------------------------------------------------------- partial blocks
@pytest.mark.parametrize('case', [c for c, _ in wc.PARTIAL_CASES], ids=wc.case_id)
def test_partial_blocks_are_exact_and_read_only_their_window(case):
    """Every case through vqn_wgrad_partials and vqn_wgrad_partials_x3, each as a single call and as a batched call of one problem:
    block s must equal the integer contraction over point tiles s, s + n, ... of the window (rows, columns, split, tile range: any
    slip changes an integer), with the tiles around the window poisoned and the workspaces guarded."""
    a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt, npt, n_split, rowsum = case
    ref = wc.exact_partial_case(case)
    Ap, Bp, want_ws, want_rs = ref['Ap'].cuda(), ref['Bp'].cuda(), ref['ws'].cuda(), ref['rs'].cuda()
    got = {}
    for x3 in (False, True):
        for batched in (False, True):
            n, ws, rs = _run_partials(Ap, Bp, case[:6], npt, n_split, rowsum, x3, batched)
            assert n == ref['n']
            bad = int((ws != want_ws).sum())
            assert bad == 0, f'x3={x3} batched={batched}: {bad} of {ws.numel()} elements differ from the integer contraction'
            if rowsum:
                assert torch.equal(rs, want_rs), f'x3={x3} batched={batched}: row sums'
            got[x3, batched] = ws
    if wc.partial_class(a_nt, b_nt, True, npt) < 3:              # the x3 entry hands this shape to the f32 kernel
        assert torch.equal(got[True, False], got[False, False]) and torch.equal(got[True, True], got[False, True])


@pytest.mark.parametrize('x3,case', wc.ACCURACY_CASES, ids=lambda v: wc.case_id(v) if isinstance(v, tuple) else ('x3' if v else 'f32'))
def test_partial_blocks_meet_the_float32_yardstick_and_are_the_same_through_both_entries(x3, case):
    """One real-valued case per kernel class.  Single call and batched call: the same blocks BIT FOR BIT (at 1025 point tiles that is
    the narrow kernel against wgrad_x3_lds_body<false, 2> with an idle second tile).  Their sum against the float64 contraction:
    within the yardstick of torch.matmul in float32; the exact-split kernels also within max(2 x the f32 kernel's error, 2e-7) of
    the sum of the terms' magnitudes (the relation test_bf16x3_weight_gradient_contraction_matches_the_f32_one holds whole tensors to).
    Row sums: within the rounding bound gamma_K of a float32 sum of the K points, in whatever order."""
    a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt, npt, n_split, rowsum = case
    name = 'test_partial_blocks_meet_the_float32_yardstick'
    key = ('x3-' if x3 else 'f32-') + wc.case_id(case)
    assert wc.partial_class(a_nt, b_nt, x3, npt) >= (3 if x3 else 0)
    A, B = wc.real_operands(npt, a_tiles, b_tiles, seed=100 * a_nt + b_nt)
    Ap, Bp = wc.poisoned(A, a_t0, a_nt).cuda(), wc.poisoned(B, b_t0, b_nt).cuda()
    n, ws, rs = _run_partials(Ap, Bp, case[:6], npt, n_split, True, x3, False)
    nb, wsb, rsb = _run_partials(Ap, Bp, case[:6], npt, n_split, True, x3, True)
    assert torch.equal(_bits(ws), _bits(wsb)) and torch.equal(_bits(rs), _bits(rsb)), 'single and batched entry differ'
    Aw, Bw = wc.window_rows(A, a_t0, a_nt), wc.window_rows(B, b_t0, b_nt)
    ref64 = Aw @ Bw.T
    ref32 = torch.matmul(Aw.float(), Bw.float().T)
    hip = ws.double().sum(0).cpu()
    r = yardstick(hip.numpy(), ref32.numpy(), ref64.numpy())
    record_observed(name, key, r['e_hip'], r['bound'])
    record_observed(name, key + REF32, r['e_ref'], r['bound'])
    record_observed(name, key + '#rms', r['rms_hip'], r['rms_bound'])
    record_observed(name, key + '#rms' + REF32, r['rms_ref'], r['rms_bound'])
    problems = [] if r['ok'] else [f'yardstick: {r}']
    if x3:
        _, ws32, _ = _run_partials(Ap, Bp, case[:6], npt, n_split, True, False, False)
        scale = float((Aw.abs() @ Bw.abs().T).max())
        e32 = float((ws32.double().sum(0).cpu() - ref64).abs().max()) / scale
        ex3 = float((hip - ref64).abs().max()) / scale
        record_observed(name, key + '#x3_vs_f32_kernel', ex3, max(2.0 * e32, 2e-7))
        if not ex3 <= max(2.0 * e32, 2e-7):
            problems.append(f'ex3 {ex3:.3e} > max(2 x e32 {e32:.3e}, 2e-7)')
    K = 32 * npt
    rs_err = (rs.double().sum(0).cpu() - Aw.sum(1)).abs()
    rs_bound = K * wc.U / (1.0 - K * wc.U) * Aw.abs().sum(1)
    record_observed(name, key + '#rowsum/bound', float((rs_err / rs_bound).max()), 1.0)
    if not bool((rs_err <= rs_bound).all()):
        problems.append('row sums outside the rounding bound')
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('x3,npt,n_split', [(False, 7, 4), (True, 7, 4), (True, 1025, 64)], ids=['f32-7', 'x3-7', 'x3-1025'])
def test_batched_call_of_forty_problems_equals_forty_single_calls(x3, npt, n_split):
    """One vqn_wgrad_partials_batched call of 40 windows into two shared operands: 26 of one class (more than WG_MAX = 24: its table
    is flushed in the middle of the loop), 14 of every other class reachable, interleaved, every third without row sums.  Integer
    operands: each problem's blocks exact and torch.equal to its single call.  Real operands: bit-equal to the single call."""
    probs, _ = wc.batched_problems(x3, npt)
    ref = wc.batched_reference(npt, n_split)
    n_exp = ref['n']
    want_ws, want_rs = ref['ws'].cuda(), ref['rs'].cuda()
    real = wc.real_operands(npt, wc.BATCH_A_TILES, wc.BATCH_B_TILES, seed=npt)
    for kind, (A, B) in (('int', (ref['A'].cuda(), ref['B'].cuda())), ('real', (real[0].cuda(), real[1].cuda()))):
        wsg = [Guarded(n_exp * a_nt * 32 * b_nt * 32, spare=32) for _, a_nt, _, b_nt, _ in probs]
        rsg = [Guarded(n_exp * a_nt * 32, spare=32) if rs else None for _, a_nt, _, _, rs in probs]
        col = lambda j: [p[j] for p in probs]
        with launches() as rec:
            n = _C.wgrad_partials_batched([A] * 40, [wc.BATCH_A_TILES] * 40, col(0), col(1), [B] * 40, [wc.BATCH_B_TILES] * 40, col(2), col(3),
                                          npt, n_split, [g.ptr for g in wsg], [None if g is None else g.ptr for g in rsg], x3)
        assert n == n_exp and rec.counts.get('vqn_wgrad_partials_x3' if x3 else 'vqn_wgrad_partials') == 1
        for i, (a_t0, a_nt, b_t0, b_nt, rowsum) in enumerate(probs):
            tag = f'{kind} problem {i} {probs[i]} class {wc.CLASS_NAMES[wc.partial_class(a_nt, b_nt, x3, npt)]}'
            rows, cols = a_nt * 32, b_nt * 32
            ws = wsg[i].view(n, rows, cols)
            assert wsg[i].intact() and (rsg[i] is None or rsg[i].intact()), tag + ': written outside its blocks'
            n1, ws1, rs1 = _run_partials(A, B, (wc.BATCH_A_TILES, a_t0, a_nt, wc.BATCH_B_TILES, b_t0, b_nt), npt, n_split, rowsum, x3, False)
            assert torch.equal(_bits(ws), _bits(ws1)), tag + ': not the single call\'s blocks'
            if rowsum:
                assert torch.equal(_bits(rsg[i].view(n, rows)), _bits(rs1)), tag + ': not the single call\'s row sums'
            if kind == 'int':
                assert torch.equal(ws, want_ws[:, 32 * a_t0:32 * a_t0 + rows, 32 * b_t0:32 * b_t0 + cols]), tag + ': not exact'
                if rowsum:
                    assert torch.equal(rsg[i].view(n, rows), want_rs[:, 32 * a_t0:32 * a_t0 + rows]), tag + ': row sums not exact'
            else:
                assert bool(torch.isfinite(ws).all())


# ----------------------------------------------------------------------------------------------------------- thin kernel
def _run_thin(problems, npt, n_split):
    """problems: (A, a_tiles, a_t0, a_row0, a_rows, B, b_tiles, b_t0, b_nt, rowsum) -> (n, [ws [n, 32 b_nt, 8]], [rs [n, 32] | None])"""
    n_exp = wc.n_blocks(npt, n_split)
    wsg = [Guarded(n_exp * 32 * p[8] * 8, spare=(n_split - n_exp) * 32 * p[8] * 8) for p in problems]
    rsg = [Guarded(n_exp * 32, spare=(n_split - n_exp) * 32) if p[9] else None for p in problems]
    col = lambda j: [p[j] for p in problems]
    with launches() as rec:
        n = _C.wgrad_thin_batched(col(0), col(1), col(2), col(3), col(4), col(5), col(6), col(7), col(8), npt, n_split,
                                  [g.ptr for g in wsg], [None if g is None else g.ptr for g in rsg])
    assert rec.counts.get('vqn_wgrad_thin_batched') == 1, rec.counts
    assert n == n_exp
    for i, (w, r) in enumerate(zip(wsg, rsg)):
        assert w.intact() and (r is None or r.intact()), f'problem {i}: written outside its blocks'
    return n, [w.view(n, 32 * p[8], 8) for w, p in zip(wsg, problems)], [None if r is None else r.view(n, 32) for r in rsg]


@pytest.mark.parametrize('case', wc.THIN_CASES, ids=wc.case_id)
def test_thin_blocks_are_exact_transposed_and_read_only_their_rows(case):
    a_tiles, a_t0, a_row0, a_rows, b_tiles, b_t0, b_nt, npt, n_split = case
    A, B = wc.int_operand(npt, a_tiles, 5), wc.int_operand(npt, b_tiles, 6)
    wc.assert_headroom(A, B, n_points=32 * npt, what='thin')
    n_ref, want_ws, want_rs = wc.thin_reference(A, a_t0, a_row0, a_rows, B, b_t0, b_nt, npt, n_split)
    Ap, Bp = wc.poisoned(A, a_t0, 1, a_row0, a_rows).cuda(), wc.poisoned(B, b_t0, b_nt).cuda()
    n, (ws,), (rs,) = _run_thin([(Ap, a_tiles, a_t0, a_row0, a_rows, Bp, b_tiles, b_t0, b_nt, True)], npt, n_split)
    assert n == n_ref == min(n_split, npt)
    assert torch.equal(ws, wc.exact32(want_ws).cuda()), 'blocks [n][32 b_nt][8]'
    assert torch.equal(rs, wc.exact32(want_rs).cuda()), 'row sums [n][32]'
    assert not ws[:, :, a_rows:].any() and not rs[:, a_rows:].any()          # exactly zero (already implied: the reference has zeros there)
    _, (ws0,), (rs0,) = _run_thin([(Ap, a_tiles, a_t0, a_row0, a_rows, Bp, b_tiles, b_t0, b_nt, False)], npt, n_split)
    assert rs0 is None and torch.equal(ws0, ws)                              # NULL row-sum workspace


def test_thin_call_of_twenty_five_problems():
    """More than TH_MAX = 24 problems in one call (a second launch for the 25th), windows into shared operands, some without row sums."""
    npt, n_split = 7, 3
    A, B = wc.int_operand(npt, 3, 5), wc.int_operand(npt, 9, 6)
    wc.assert_headroom(A, B, n_points=32 * npt, what='thin batch')
    Ad, Bd = A.cuda(), B.cuda()
    probs = wc.thin_batch_problems()
    n, ws, rs = _run_thin([(Ad, 3, a_t0, a_row0, a_rows, Bd, 9, b_t0, b_nt, rowsum) for a_t0, a_row0, a_rows, b_t0, b_nt, rowsum in probs], npt, n_split)
    for i, (a_t0, a_row0, a_rows, b_t0, b_nt, rowsum) in enumerate(probs):
        _, want_ws, want_rs = wc.thin_reference(A, a_t0, a_row0, a_rows, B, b_t0, b_nt, npt, n_split)
        assert torch.equal(ws[i], wc.exact32(want_ws).cuda()), f'problem {i} {probs[i]}'
        assert (rs[i] is None) == (not rowsum)
        if rowsum:
            assert torch.equal(rs[i], wc.exact32(want_rs).cuda()), f'problem {i} {probs[i]}: row sums'


def test_thin_blocks_meet_the_float32_yardstick():
    """3 rows against 12 feature tiles (two problems: b_nt 8 and 4) over 64 point tiles, real-valued: summed blocks against float64."""
    c = wc.THIN_ACCURACY
    npt, n_split, a_rows = c['n_point_tiles'], c['n_split'], c['a_rows']
    A, B = wc.real_operands(npt, c['a_tiles'], c['b_tiles'], seed=12)
    Ap = wc.poisoned(A, c['a_t0'], 1, c['a_row0'], a_rows).cuda()
    probs = [(Ap, c['a_tiles'], c['a_t0'], c['a_row0'], a_rows, wc.poisoned(B, b0, bn).cuda(), c['b_tiles'], b0, bn, True) for b0, bn in c['blocks']]
    n, ws, rs = _run_thin(probs, npt, n_split)
    for w in ws:
        assert not w[:, :, a_rows:].any()
    hip = torch.cat([w.double().sum(0)[:, :a_rows] for w in ws], 0).cpu()    # [384, 3]
    Aw, Bw = wc.window_rows(A, c['a_t0'], 1)[c['a_row0']:c['a_row0'] + a_rows], wc.window_rows(B, 0, c['b_tiles'])
    ref64, ref32 = Bw @ Aw.T, torch.matmul(Bw.float(), Aw.float().T)
    r = yardstick(hip.numpy(), ref32.numpy(), ref64.numpy())
    name = 'test_thin_blocks_meet_the_float32_yardstick'
    record_observed(name, 'blocks', r['e_hip'], r['bound'])
    record_observed(name, 'blocks' + REF32, r['e_ref'], r['bound'])
    record_observed(name, 'blocks#rms', r['rms_hip'], r['rms_bound'])
    record_observed(name, 'blocks#rms' + REF32, r['rms_ref'], r['rms_bound'])
    K = 32 * npt
    rs_err = (rs[0].double().sum(0)[:a_rows].cpu() - Aw.sum(1)).abs()
    rs_bound = K * wc.U / (1.0 - K * wc.U) * Aw.abs().sum(1)
    record_observed(name, 'rowsum/bound', float((rs_err / rs_bound).max()), 1.0)
    assert torch.equal(_bits(rs[0]), _bits(rs[1])) and not rs[0][:, a_rows:].any()
    assert r['ok'] and bool((rs_err <= rs_bound).all()), r


# ----------------------------------------------------------------------------------------------------------- ordered sums
def _partials(rng, n, rows, cols, integer=False):
    if integer:
        return rng.integers(-8, 9, size=(n, rows, cols)).astype(np.float32)
    return (rng.normal(size=(n, rows, cols)) * np.exp(rng.normal(size=(n, 1, 1)) * 2.0)).astype(np.float32)


@pytest.mark.parametrize('rows,cols', wc.REDUCE_BLOCKS)
@pytest.mark.parametrize('n', wc.REDUCE_N)
def test_reduce_partials_sums_in_the_documented_order(n, rows, cols):
    """Bit-equal to the numpy float32 restatement of the order (16 groups of ceil(n / 16) consecutive blocks, group sums in group
    order, then `out`), within the rounding bound of the float64 sum, into a window of a wider matrix whose other columns stay."""
    rng = np.random.default_rng(1000 * n + rows)
    ws = _partials(rng, n, rows, cols)
    out_ld = cols + 8
    out0 = rng.normal(size=(rows, out_ld)).astype(np.float32)
    ws_d = torch.tensor(ws).cuda()
    for accumulate in (0, 1):
        out = Guarded(rows * out_ld, fill=torch.tensor(out0).cuda())
        with launches() as rec:
            _C.reduce_partials(ws_d, n, rows, cols, out.view(rows, out_ld), out_ld, accumulate)
        assert rec.counts.get('vqn_reduce_partials') == 1 and out.intact()
        got = out.view(rows, out_ld).cpu().numpy()
        want = out0.copy()
        want[:, :cols] = wc.reduce_restatement(ws, out0[:, :cols] if accumulate else None)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f'accumulate={accumulate}: {(got != want).sum()} elements differ'
        s, bound = wc.reduce_bound(ws, out0[:, :cols] if accumulate else None)
        assert (np.abs(got[:, :cols].astype(np.float64) - s) <= bound).all()


def _finalize_image(like, tmp, transposed, rows_valid, col_first, cols_valid):
    """the destination matrix of a finalize entry: NaN but for the valid window of tmp, transposed or not (see the test below)"""
    want = torch.full_like(like, NAN)
    if transposed:
        want[3 + col_first:3 + cols_valid, 2:2 + rows_valid] = tmp[:rows_valid, col_first:cols_valid].T
    else:
        want[2:2 + rows_valid, 3 + col_first:3 + cols_valid] = tmp[:rows_valid, col_first:cols_valid]
    return want


def test_finalize_of_forty_five_entries_is_reduce_scale_transpose_slice():
    """One vqn_wgrad_finalize call of 45 entries (more than FIN_MAX = 40) of mixed sizes: every written element bit-equal to
    vqn_reduce_partials (+ vqn_reduce_partials(accumulate = 1) for ws2), a torch float32 multiply by scale and a torch transpose /
    slice -- and to the numpy restatement of the same --, every other element of the NaN-filled destinations still NaN."""
    ents = wc.finalize_entries()
    rng = np.random.default_rng(5)
    ws, ws2, big, dst, sr, sc, host = [], [], [], [], [], [], []
    for e in ents:
        R, C = e['src_rows'], e['src_cols']
        w = _partials(rng, e['n'], R, C, e['integer'])
        w2 = None if e['n2'] is None else _partials(rng, e['n2'], R, C, e['integer'])
        host.append((w, w2))
        ws.append(torch.tensor(w).cuda())
        ws2.append(None if w2 is None else torch.tensor(w2).cuda())
        if e['transposed']:                                      # element (r, c) at m[3 + c, 2 + r]
            m = torch.full((C + 7, R + 5), NAN, device='cuda')
            dst.append(m[3:, 2:]); sr.append(1); sc.append(m.stride(0))
        else:                                                    # element (r, c) at m[2 + r, 3 + c]
            m = torch.full((R + 5, C + 7), NAN, device='cuda')
            dst.append(m[2:, 3:]); sr.append(m.stride(0)); sc.append(1)
        big.append(m)
    col = lambda k: [e[k] for e in ents]
    with launches() as rec:
        _C.wgrad_finalize(ws, col('n'), ws2, [e['n2'] or 0 for e in ents], col('src_rows'), col('src_cols'), col('rows_valid'), col('col_first'),
                          col('cols_valid'), dst, sr, sc, col('scale'))
    assert rec.counts.get('vqn_wgrad_finalize') == 1, rec.counts
    for i, e in enumerate(ents):
        R, C, rv, c0, cv = e['src_rows'], e['src_cols'], e['rows_valid'], e['col_first'], e['cols_valid']
        tmp = torch.full((R, C), NAN, device='cuda')
        _C.reduce_partials(ws[i], e['n'], R, C, tmp, C, 0)
        if ws2[i] is not None:
            _C.reduce_partials(ws2[i], e['n2'], R, C, tmp, C, 1)
        tmp = tmp * e['scale']
        w, w2 = host[i]
        res = wc.reduce_restatement(w)
        if w2 is not None:
            res = wc.reduce_restatement(w2, res)
        res = res * np.float32(e['scale'])
        assert res.dtype == np.float32 and np.array_equal(tmp.cpu().numpy().view(np.int32), res.view(np.int32)), f'entry {i}: the sequence itself'
        want = _finalize_image(big[i], tmp, e['transposed'], rv, c0, cv)
        assert torch.equal(_bits(big[i]), _bits(want)), f'entry {i} {e}: {int((_bits(big[i]) != _bits(want)).sum())} elements differ'
        if e['integer']:
            exact = w.astype(np.float64).sum(0) + (0.0 if w2 is None else w2.astype(np.float64).sum(0))
            assert np.array_equal(tmp.cpu().numpy().astype(np.float64), exact * e['scale']), f'entry {i}: integer partials'


# ----------------------------------------------------------------------------------------------------------- the planner
def _int_rows(N, F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-wc.INT_MAX, wc.INT_MAX + 1, (N, F), generator=g).to(torch.float32)


class _Dst:
    """A [rows, cols] result inside a larger NaN matrix, row-major or transposed, and a bias inside a larger NaN vector."""

    def __init__(self, rows, cols, transposed, pad):
        r0, c0 = pad
        self.rows, self.cols, self.transposed, self.r0, self.c0 = rows, cols, transposed, r0, c0
        if transposed:
            self.m = torch.full((cols + 2 * c0 + 1, rows + 2 * r0 + 3), NAN, device='cuda')
            self.dst, self.sr, self.sc = self.m[c0:, r0:], 1, self.m.stride(0)
        else:
            self.m = torch.full((rows + 2 * r0 + 1, cols + 2 * c0 + 3), NAN, device='cuda')
            self.dst, self.sr, self.sc = self.m[r0:, c0:], self.m.stride(0), 1
        self.b = torch.full((rows + 13,), NAN, device='cuda')
        self.bias = self.b[3:]

    def check(self, want, want_bias, col_first=0, tag='', scale=1.0):
        """want [rows, cols] float64 integers (times the float32 `scale`, one rounding); columns below col_first and everything
        around the window must still be NaN"""
        exp = torch.full_like(self.m, NAN)
        w = wc.exact32(want).cuda()
        if scale != 1.0:
            w = w * torch.tensor(scale, dtype=torch.float32, device='cuda')
        if self.transposed:
            exp[self.c0 + col_first:self.c0 + self.cols, self.r0:self.r0 + self.rows] = w[:, col_first:].T
        else:
            exp[self.r0:self.r0 + self.rows, self.c0 + col_first:self.c0 + self.cols] = w[:, col_first:]
        assert torch.equal(_bits(self.m), _bits(exp)), f'{tag}: {int((_bits(self.m) != _bits(exp)).sum())} elements of the destination differ'
        expb = torch.full_like(self.b, NAN)
        if want_bias is not None:
            expb[3:3 + self.rows] = wc.exact32(want_bias).cuda()
        assert torch.equal(_bits(self.b), _bits(expb)), f'{tag}: bias'


def _plan_case(which, npt):
    from vqnerf_release_amd.decomp.train_programs import to_tfmt
    from vqnerf_release_amd.wgrad import WgradBatch
    N = 32 * npt - 5                                             # the last point tile is zero padded
    T = lambda rows, tiles=None: to_tfmt(rows.cuda(), tiles)
    P = lambda a, b: a.double().T @ b.double()                   # the product of the rows: integers, exact in float64
    if which == 'transposed_257x295':
        a, b = _int_rows(N, 257, 1), _int_rows(N, 295, 2)
        wc.assert_headroom(a, b, n_points=N, what=which)
        d = _Dst(257, 295, True, (2, 4))
        wb = WgradBatch(64)
        wb.contract(T(a), T(b), 257, 295, d.dst, d.sr, d.sc, bias_dst=d.bias)
        with launches() as rec:
            wb.flush()
        d.check(P(a, b), a.double().sum(0), tag=which)
    elif which == 'two_terms_scaled_col_first':
        a, b, a2, b2 = _int_rows(N, 70, 3), _int_rows(N, 295, 4), _int_rows(N, 70, 5), _int_rows(N, 295, 6)
        wc.assert_headroom(a, b, a2, b2, n_points=2 * N, what=which)
        d = _Dst(70, 295, False, (1, 5))
        wb = WgradBatch(64)
        wb.contract(T(a), T(b), 70, 295, d.dst, d.sr, d.sc, bias_dst=d.bias, A2=T(a2), B2=T(b2), scale=0.5, col_first=39)
        with launches() as rec:
            wb.flush()
        want = 0.5 * (P(a, b) + P(a2, b2))
        d.check(want, a.double().sum(0), col_first=39, tag=which)
        assert bool(torch.isnan(d.dst[:70, :39]).all())
    elif which == 'col_first_skips_a_block':
        # col_first past the first 8-tile block: that block gets no problem and no entry, its columns stay NaN -- and the row sums, which
        # otherwise ride with block 0, still reach the bias
        a, b = _int_rows(N, 70, 11), _int_rows(N, 295, 12)
        wc.assert_headroom(a, b, n_points=N, what=which)
        d = _Dst(70, 295, False, (1, 5))
        wb = WgradBatch(64)
        wb.contract(T(a), T(b), 70, 295, d.dst, d.sr, d.sc, bias_dst=d.bias, col_first=260)
        assert len(wb.p) == 1 and wb.p[0][6] == 8, wb.p             # one problem: B tiles 8..9
        with launches() as rec:
            wb.flush()
        d.check(P(a, b), a.double().sum(0), col_first=260, tag=which)
        assert bool(torch.isnan(d.dst[:70, :260]).all())
    elif which == 'thin_3x384':
        a, b = _int_rows(N, 3, 7), _int_rows(N, 384, 8)
        wc.assert_headroom(a, b, n_points=N, what=which)
        d = _Dst(3, 384, False, (2, 4))
        wb = WgradBatch(64, thin=True)
        At = T(a)
        assert At.shape[1] == 1
        At[:, 0, 3:] = NAN                                       # the thin kernel reads rows 0..2 of the tile only
        wb.contract(At, T(b), 3, 384, d.dst, d.sr, d.sc, bias_dst=d.bias)
        with launches() as rec:
            wb.flush()
        assert rec.ran('vqn_wgrad_thin_batched') and not rec.ran('vqn_wgrad_partials')
        d.check(P(a, b), a.double().sum(0), tag=which)
    elif which == 'thin_rows_three_targets':
        a, b = _int_rows(N, 9, 9), _int_rows(N, 300, 10)
        wc.assert_headroom(a, b, n_points=N, what=which)
        At = T(a)
        At[:, 0, :4] = NAN
        At[:, 0, 9:] = NAN
        ds = [(0, 1, _Dst(1, 300, False, (2, 4))), (1, 3, _Dst(3, 300, True, (3, 2))), (4, 1, _Dst(1, 300, False, (5, 9)))]
        wb = WgradBatch(64, thin=True)
        wb.contract_thin_rows(At, 4, 5, T(b), 300, [(off, k, d.dst, d.sr, d.sc, d.bias) for off, k, d in ds])
        with launches() as rec:
            wb.flush()
        assert rec.ran('vqn_wgrad_thin_batched') and not rec.ran('vqn_wgrad_partials')
        want, want_b = P(a[:, 4:9], b), a[:, 4:9].double().sum(0)
        for off, k, d in ds:
            d.check(want[off:off + k], want_b[off:off + k], tag=f'{which} target ({off}, {k})')
    else:
        raise AssertionError(which)
    assert rec.ran('vqn_wgrad_finalize')
    return rec


PLAN_CASES = ('transposed_257x295', 'two_terms_scaled_col_first', 'col_first_skips_a_block', 'thin_3x384', 'thin_rows_three_targets')


@pytest.mark.parametrize('mode', ['f32', 'bf16x3'])
@pytest.mark.parametrize('which', PLAN_CASES)
def test_wgradbatch_plan_is_the_matrix_product(which, mode):
    """WgradBatch's windows (8-tile blocking, col_first clipped per block, the thin path's negative pointer offsets) against the
    integer product of the rows the operands were packed from; 3 point tiles, n_split = 64."""
    from vqnerf_release_amd import wgrad as tp
    old = tp.wgrad_mode()
    try:
        tp.wgrad_mode(mode)
        rec = _plan_case(which, 3)
        if not which.startswith('thin'):
            assert rec.ran(tp.WGRAD_ENTRY[mode]) and set(n for n in rec.names if n.startswith('vqn_wgrad_partials')) == {tp.WGRAD_ENTRY[mode]}
    finally:
        tp.wgrad_mode(old)


def test_wgradbatch_plan_at_1025_point_tiles():
    """The 257 x 295 weight again at 1025 point tiles under 'bf16x3': its 8 + 1 by 8 + 2 tile blocks run the full, the guarded and
    (the 1-tile row block) the narrow exact-split kernel."""
    from vqnerf_release_amd import wgrad as tp
    old = tp.wgrad_mode()
    try:
        tp.wgrad_mode('bf16x3')
        _plan_case('transposed_257x295', 1025)
    finally:
        tp.wgrad_mode(old)


# ----------------------------------------------------------------------------------------------------------- the two executors
def _run_executor(make, npt):
    """One contraction list through the executor make() returns; every destination checked against the integer product of the rows
    (and NaN around it) -> (launches record, destinations).  257 result rows = an 8-tile row window and one of a single valid row;
    295 / 39 columns = two / one column windows."""
    from vqnerf_release_amd.decomp.train_programs import to_tfmt
    N = 32 * npt - 5                                             # the last point tile is zero padded
    P = lambda a, b: a.double().T @ b.double()
    a, a2 = _int_rows(N, 257, 21), _int_rows(N, 257, 22)
    b295, b39, b39_2 = _int_rows(N, 295, 23), _int_rows(N, 39, 24), _int_rows(N, 39, 25)
    wc.assert_headroom(a, a2, b295, b39, b39_2, n_points=2 * N, what='executors')
    A, A2, B295, B39, B39_2 = [to_tfmt(t.cuda()) for t in (a, a2, b295, b39, b39_2)]
    s2 = float(np.float32(1.0 / math.sqrt(2.0)))
    dt = _Dst(257, 295, True, (2, 4))                            # transposed (the Keras layout), with its bias
    ds = _Dst(257, 39, False, (1, 5))                            # two terms, scaled, into a column slice of a wider matrix
    dc = _Dst(257, 39, False, (3, 2))                            # without its first column
    with launches() as rec:
        ex = make()
        ex.contract(A, B295, 257, 295, dt.dst, dt.sr, dt.sc, bias_dst=dt.bias)
        ex.contract(A, B39, 257, 39, ds.dst, ds.sr, ds.sc, A2=A2, B2=B39_2, scale=s2)
        ex.contract(A2, B39, 257, 39, dc.dst, dc.sr, dc.sc, bias_dst=dc.bias, col_first=1)
        ex.flush()
    dt.check(P(a, b295), a.double().sum(0), tag='transposed')
    ds.check(P(a, b39) + P(a2, b39_2), None, scale=s2, tag='two terms, scaled')
    dc.check(P(a2, b39), a2.double().sum(0), col_first=1, tag='col_first')
    return rec, (dt, ds, dc)


@pytest.mark.parametrize('mode', ['f32', 'bf16x3'])
def test_both_executors_write_the_same_bits_and_nothing_else(mode):
    """WgradBatch and WgradPerWeight given the same contractions (3 point tiles in 2 uneven blocks): every destination and bias equal
    bit for bit, NaN everywhere else; one vqn_wgrad_finalize for the batch, one vqn_wgrad_partials + vqn_reduce_partials per window and
    operand pair (4 + 2 * 2 + 2) for the per-weight form."""
    from vqnerf_release_amd import wgrad
    old = wgrad.wgrad_mode()
    try:
        wgrad.wgrad_mode(mode)
        rec_b, dst_b = _run_executor(lambda: wgrad.WgradBatch(2), 3)
        rec_p, dst_p = _run_executor(lambda: wgrad.WgradPerWeight(2), 3)
    finally:
        wgrad.wgrad_mode(old)
    entry = wgrad.WGRAD_ENTRY[mode]
    partial_entries = lambda rec: set(n for n in rec.names if n.startswith('vqn_wgrad_partials'))
    assert rec_b.counts.get('vqn_wgrad_finalize') == 1 and not rec_b.ran('vqn_reduce_partials') and partial_entries(rec_b) == {entry}, rec_b.counts
    assert rec_p.counts.get('vqn_reduce_partials') == 10 and rec_p.counts.get(entry) == 10 and partial_entries(rec_p) == {entry} \
        and not rec_p.ran('vqn_wgrad_finalize'), rec_p.counts
    for x, y in zip(dst_b, dst_p):
        assert torch.equal(_bits(x.m), _bits(y.m)) and torch.equal(_bits(x.b), _bits(y.b))
