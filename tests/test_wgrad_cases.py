"""What tests/test_gpu_wgrad_kernels.py rests on, checked without a GPU: the case tables reach the kernel classes they name, the
integer operands leave float32 its 2^24 headroom in every case, the references cut the point tiles the way the kernels' split
does, and the float32 restatement of vqn_reduce_partials' order is a correctly rounded-ish sum (within the plain rounding bound of
the float64 one)."""
import numpy as np
import pytest
import torch

from tests import wgrad_cases as wc


def test_case_tables_reach_the_classes_they_name():
    seen = {False: set(), True: set()}
    for case, cls in wc.PARTIAL_CASES:
        a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt, npt, n_split, _ = case
        assert 0 <= a_t0 and a_t0 + a_nt <= a_tiles and 0 <= b_t0 and b_t0 + b_nt <= b_tiles and 1 <= a_nt <= 8 and 1 <= b_nt <= 8
        assert wc.partial_class(a_nt, b_nt, False, npt) == cls['f32'] and wc.partial_class(a_nt, b_nt, True, npt) == cls['x3'], case
        seen[False].add(cls['f32']); seen[True].add(cls['x3'])
    assert seen[False] == {0, 1, 2} and seen[True] == {0, 1, 3, 4, 5}
    assert {wc.partial_class(c[2], c[5], x3, c[6]) for x3, c in wc.ACCURACY_CASES} == {0, 1, 2, 3, 4, 5}
    # windows inside wider tensors, NULL row sums, n_split above and below the tile count, unequal and odd tile counts per workgroup
    cases = [c for c, _ in wc.PARTIAL_CASES]
    assert any(c[1] > 0 and c[4] > 0 and c[0] > c[1] + c[2] for c in cases) and any(not c[8] for c in cases)
    assert any(c[7] > c[6] for c in cases) and any(c[6] % c[7] for c in cases if c[7] <= c[6])
    assert {c[2] for c in cases} >= {5, 7, 8} and any(c[5] < 8 and c[2] > 4 for c in cases)
    for a_tiles, a_t0, a_row0, a_rows, b_tiles, b_t0, b_nt, npt, n_split in wc.THIN_CASES:
        assert a_t0 < a_tiles and a_row0 + a_rows <= 32 and 1 <= a_rows <= 8 and b_t0 + b_nt <= b_tiles
    assert {c[3] for c in wc.THIN_CASES} >= {1, 8} and any(c[2] > 0 for c in wc.THIN_CASES)


@pytest.mark.parametrize('x3,npt', [(False, 7), (True, 7), (True, 1025)])
def test_batched_problem_lists_overflow_one_class_and_interleave_the_rest(x3, npt):
    probs, major = wc.batched_problems(x3, npt)
    assert len(probs) == wc.BATCH_COUNT
    cls = [wc.partial_class(p[1], p[3], x3, npt) for p in probs]
    reachable = {wc.partial_class(a, b, x3, npt) for a in range(1, 9) for b in range(1, 9)}
    assert set(cls) == reachable and cls.count(major) == wc.BATCH_MAJOR > wc.WG_MAX
    for c in reachable - {major}:
        assert cls.count(c) >= 2
    # the table of the major class fills up (its 24th problem) while problems of every other class are still to come and already queued
    full_at = [i for i, c in enumerate(cls) if c == major][wc.WG_MAX - 1]
    assert all(any(x == c for x in cls[:full_at]) for c in reachable - {major})
    assert major in cls[full_at + 1:] and any(x != major for x in cls[full_at + 1:])
    assert max(len(list(g)) for g in _runs(cls)) <= 3
    for a_t0, a_nt, b_t0, b_nt, rs in probs:
        assert a_t0 + a_nt <= wc.BATCH_A_TILES and b_t0 + b_nt <= wc.BATCH_B_TILES
    assert any(not p[4] for p in probs) and any(p[4] for p in probs)
    assert len({p[:4] for p in probs}) > 30                       # windows, not one window forty times
    assert wc.batched_problems(x3, npt)[0] == probs               # deterministic
    if major == 5:                                                # the narrow kernel inside a full table: every a_nt it takes, wide B too
        narrow = [p for p, c in zip(probs, cls) if c == 5]
        assert {p[1] for p in narrow} == {1, 2, 3, 4} and max(p[3] for p in narrow) == 8 and min(p[3] for p in narrow) <= 2


def _runs(xs):
    run = []
    for x in xs:
        if run and run[-1] != x:
            yield run
            run = []
        run.append(x)
    yield run


def test_thin_and_finalize_tables():
    probs = wc.thin_batch_problems()
    assert len(probs) == 25 > wc.TH_MAX and any(not p[5] for p in probs) and {p[2] for p in probs} >= {1, 8}
    for a_t0, a_row0, a_rows, b_t0, b_nt, rs in probs:
        assert a_t0 < 3 and a_row0 + a_rows <= 32 and b_t0 + b_nt <= 9
    ents = wc.finalize_entries()
    assert len(ents) == 45 > wc.FIN_MAX
    assert {(e['src_rows'], e['src_cols']) for e in ents} == {(1, 32), (96, 8), (64, 96), (256, 256)}
    assert {e['n'] for e in ents} == set(wc.REDUCE_N)
    assert any(e['n2'] is not None and e['n2'] != e['n'] for e in ents)
    assert {e['scale'] for e in ents} == {1.0, 0.5, float(np.float32(2.0 ** -0.5))}
    assert any(e['rows_valid'] < e['src_rows'] for e in ents) and any(e['cols_valid'] < e['src_cols'] for e in ents)
    assert any(e['col_first'] > 0 for e in ents) and {e['transposed'] for e in ents} == {True, False}
    assert any(e['integer'] and e['n2'] is not None for e in ents)
    for e in ents:
        assert 1 <= e['rows_valid'] <= e['src_rows'] and 0 <= e['col_first'] < e['cols_valid'] <= e['src_cols'] and e['src_cols'] % 4 == 0
    # consecutive entries differ in size: a block -> entry lookup off by one entry reads a block of another shape
    assert sum((a['src_rows'], a['src_cols']) != (b['src_rows'], b['src_cols']) for a, b in zip(ents, ents[1:])) >= 30


def test_integer_operands_leave_float32_its_headroom_in_every_case():
    worst = 0.0
    for case, _ in wc.PARTIAL_CASES:
        a_tiles, _, _, b_tiles, _, _, npt, _, _ = case
        A, B = wc.int_operand(npt, a_tiles, 1), wc.int_operand(npt, b_tiles, 2)
        worst = max(worst, wc.assert_headroom(A, B, n_points=32 * npt, what=wc.case_id(case)))
    for npt in (7, 1025):
        A, B = wc.int_operand(npt, wc.BATCH_A_TILES, 3), wc.int_operand(npt, wc.BATCH_B_TILES, 4)
        worst = max(worst, wc.assert_headroom(A, B, n_points=32 * npt, what='batched'))
    for c in wc.THIN_CASES:
        wc.assert_headroom(wc.int_operand(c[7], c[0], 5), wc.int_operand(c[7], c[4], 6), n_points=32 * c[7], what='thin')
    assert 2.0e6 < worst < 2 ** 24                                # 64 x 32,800 at the 1025-tile cases
    A = wc.int_operand(3, 2, 1)
    assert A.min() == -8 and A.max() == 8 and torch.equal(A.to(torch.bfloat16).to(torch.float32), A)      # one bf16 piece each
    with pytest.raises(AssertionError):
        wc.assert_headroom(A * 1024.0, A, n_points=96)
    with pytest.raises(AssertionError):
        wc.assert_headroom(A + 0.5, A, n_points=96)


def test_block_references_are_the_plain_contraction_cut_by_the_split():
    case = (6, 1, 5, 5, 2, 3, 5, 2, True)
    ref = wc.exact_partial_case(case)
    A, B = ref['A'], ref['B']
    assert ref['n'] == 2 and ref['ws'].shape == (2, 160, 96) and ref['rs'].shape == (2, 160)
    # element by element, straight from the layout [point tile][feature tile][feature][point]
    rows_a = torch.stack([A[p // 32, 1 + o // 32, o % 32, p % 32] for o in (0, 37, 159) for p in range(160)]).reshape(3, 160).to(torch.int64)
    rows_b = torch.stack([B[p // 32, 2 + i // 32, i % 32, p % 32] for i in (0, 95) for p in range(160)]).reshape(2, 160).to(torch.int64)
    tile = torch.arange(160) // 32
    for s in (0, 1):
        mine = (tile % 2 == s).to(torch.int64)                    # block s of 2: tiles s, s + 2, ...
        want = (rows_a * mine) @ rows_b.T
        got = ref['ws'][s][[0, 37, 159]][:, [0, 95]]
        assert torch.equal(got.to(torch.int64), want)
        assert torch.equal(ref['rs'][s][[0, 37, 159]].to(torch.int64), (rows_a * mine).sum(1))
    assert wc.block_tiles(0, 2, 5) == [0, 2, 4] and wc.block_tiles(1, 2, 5) == [1, 3] and wc.n_blocks(1, 64) == 1
    # the poisoned copies agree with the clean ones inside the window and nowhere else
    assert torch.equal(ref['Ap'][:, 1:6], A[:, 1:6]) and bool(torch.isnan(ref['Ap'][:, 0]).all()) and bool(torch.isnan(ref['Bp'][:, :2]).all())
    P = wc.poisoned(A, 2, 1, row0=4, rows=5)
    assert torch.equal(P[:, 2, 4:9], A[:, 2, 4:9]) and int(torch.isfinite(P).sum()) == 5 * 5 * 32
    # thin: transposed blocks, zero columns
    n, ws, rs = wc.thin_reference(A, 2, 4, 5, B, 2, 3, 5, 2)
    assert n == 2 and ws.shape == (2, 96, 8) and rs.shape == (2, 32) and not ws[:, :, 5:].any() and not rs[:, 5:].any()
    full = wc.partials_reference(A, 2, 1, B, 2, 3, 5, 2)
    assert torch.equal(ws[:, :, :5], full[1][:, 4:9].transpose(1, 2)) and torch.equal(rs[:, :5], full[2][:, 4:9])
    # the shared reference of the batched calls holds every problem's blocks as a slice
    b = wc.batched_reference(7, 4)
    n, ws, rs = wc.partials_reference(b['A'], 3, 2, b['B'], 5, 4, 7, 4)
    assert n == b['n'] == 4 and torch.equal(ws.float(), b['ws'][:, 96:160, 160:288]) and torch.equal(rs.float(), b['rs'][:, 96:160])


def test_guard_helper():
    total, off = wc.guarded_layout(10, spare=6)
    buf = torch.full((total,), float('nan'))
    buf[off:off + 10] = 1.0
    assert wc.untouched(buf, 10)
    for bad in (off - 1, off + 10, total - 1, 0):
        b2 = buf.clone(); b2[bad] = 0.0
        assert not wc.untouched(b2, 10)


@pytest.mark.parametrize('n', wc.REDUCE_N)
def test_reduce_restatement_is_an_ordered_float32_sum_within_the_rounding_bound(n):
    rng = np.random.default_rng(n)
    ws = (rng.normal(size=(n, 5, 12)) * np.exp(rng.normal(size=(n, 1, 1)) * 3.0)).astype(np.float32)
    out = rng.normal(size=(5, 12)).astype(np.float32)
    for o in (None, out):
        got = wc.reduce_restatement(ws, o)
        s, bound = wc.reduce_bound(ws, o)
        assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - s) <= bound).all()
    # the order is the documented one, not another: element by element with Python's float32 scalars
    per = (n + 15) >> 4
    t = np.float32(0.0)
    for g in range(16):
        acc = np.float32(0.0)
        for s_ in range(g * per, min(n, g * per + per)):
            acc = np.float32(acc + ws[s_, 3, 7])
        t = acc if g == 0 else np.float32(t + acc)
    assert wc.reduce_restatement(ws)[3, 7] == t and wc.reduce_restatement(ws, out)[3, 7] == np.float32(t + out[3, 7])
    # integers: exact
    wi = rng.integers(-8, 9, size=(n, 5, 12)).astype(np.float32)
    assert np.array_equal(wc.reduce_restatement(wi).astype(np.float64), wi.astype(np.float64).sum(0))
