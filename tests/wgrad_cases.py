"""Cases, operands and references of the direct weight-gradient kernel tests (tests/test_gpu_wgrad_kernels.py).  Nothing here
touches a GPU: the case tables, the integer operands whose contraction is exact in float32 whatever the summation order, the
poisoned copies, the per-block references and the float32 restatement of vqn_reduce_partials' documented order are all checked
on the CPU too (tests/test_wgrad_cases.py).

The tile format (TFMT) of every operand: [point tiles][feature tiles][32 features][32 points]."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24                # unit roundoff of float32
GUARD = 64                    # floats of NaN before and after every workspace / destination
INT_MAX = 8                   # integer operands are drawn from [-INT_MAX, INT_MAX]: one bf16 piece each
WG_MAX, TH_MAX, FIN_MAX = 24, 24, 40          # problems / entries per launch of the batched kernels (csrc/wgrad_batch.h, wgrad_thin.hip, wgrad_finalize.hip)
X3_SMALL_FROM = 1024          # csrc/wgrad_batch.h WG_X3_SMALL_FROM: point tiles from which a_nt <= 4 problems stay on the exact-split kernels

CLASS_NAMES = ('f32<1,4,6>', 'f32<1,8,4>', 'f32<2,8,D>', 'x3 full', 'x3 guarded', 'x3 narrow')


def partial_class(a_nt, b_nt, x3, n_point_tiles):
    """wgrad_class of csrc/wgrad_batch.h, restated: the kernel class all three entries file a problem under; the single-problem x3
    entry has no narrow kernel: class 5 is the guarded kernel with one idle output tile per wave there."""
    f32 = (not x3) or (a_nt <= 4 and n_point_tiles < X3_SMALL_FROM)
    if f32:
        return 0 if (a_nt <= 4 and b_nt <= 4) else (1 if a_nt <= 4 else 2)
    return 3 if (a_nt == 8 and b_nt == 8) else (5 if a_nt <= 4 else 4)


# ------------------------------------------------------------------------------------------------------------- case tables
# (a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt, n_point_tiles, n_split, rowsum) -- and the class each entry must reach with it
PARTIAL_CASES = [
    ((3, 1, 2, 5, 2, 3, 7, 3, True), dict(f32=0, x3=0)),          # workgroups of 3 / 2 / 2 tiles: n_q = 12 / 8 against the ring depth 6
    ((4, 0, 4, 4, 0, 4, 1, 64, True), dict(f32=0, x3=0)),         # grid 1, n_split > tiles
    ((4, 1, 3, 9, 1, 8, 5, 2, False), dict(f32=1, x3=1)),         # NULL row sums
    ((9, 1, 8, 8, 0, 8, 6, 4, True), dict(f32=2, x3=3)),
    ((6, 1, 5, 3, 0, 3, 7, 7, True), dict(f32=2, x3=4)),          # a_nt = 5: only wave 0 owns a second tile; one tile per workgroup
    ((10, 2, 8, 9, 1, 8, 7, 2, True), dict(f32=2, x3=3)),         # workgroups of 4 and 3 tiles: n_q = 6 leaves a tail of 2 against R = 4
    ((8, 0, 8, 8, 0, 8, 3, 64, False), dict(f32=2, x3=3)),
    ((6, 1, 5, 5, 2, 3, 5, 2, True), dict(f32=2, x3=4)),
    ((8, 0, 8, 4, 1, 3, 2, 1, True), dict(f32=2, x3=4)),
    ((7, 0, 7, 8, 0, 8, 9, 4, False), dict(f32=2, x3=4)),
    # windows with feature tiles on BOTH sides (a look-ahead fetch clamped one tile too far reads the poison behind the window)
    ((5, 1, 3, 6, 2, 3, 4, 3, True), dict(f32=0, x3=0)),
    ((10, 1, 8, 10, 1, 8, 5, 2, True), dict(f32=2, x3=3)),
    ((8, 1, 6, 6, 1, 4, 5, 2, True), dict(f32=2, x3=4)),
    ((4, 0, 4, 8, 0, 8, 1025, 64, True), dict(f32=1, x3=5)),      # workgroups of 17 or 16 tiles
    ((3, 1, 2, 5, 2, 3, 1025, 64, True), dict(f32=0, x3=5)),
    ((2, 1, 1, 2, 1, 1, 1025, 64, False), dict(f32=0, x3=5)),
]
# one real-valued case per class for the accuracy yardstick: (entry is x3, case)
ACCURACY_CASES = [
    (False, (3, 1, 2, 5, 2, 3, 7, 3, True)),
    (False, (4, 1, 3, 9, 1, 8, 5, 2, True)),
    (False, (6, 1, 5, 3, 0, 3, 7, 7, True)),
    (True, (10, 2, 8, 9, 1, 8, 7, 2, True)),
    (True, (6, 1, 5, 5, 2, 3, 5, 2, True)),
    (True, (3, 1, 2, 5, 2, 3, 1025, 64, True)),
]

# (a_tiles, a_t0, a_row0, a_rows, b_tiles, b_t0, b_nt, n_point_tiles, n_split): shapes paired with the splits, not crossed
THIN_CASES = [
    (1, 0, 0, 3, 9, 1, 8, 1, 64),
    (3, 2, 29, 3, 4, 0, 1, 2, 1),
    (1, 0, 5, 8, 8, 0, 8, 7, 3),
    (2, 1, 0, 1, 5, 2, 3, 64, 32),
]
THIN_ACCURACY = dict(a_tiles=1, a_t0=0, a_row0=0, a_rows=3, b_tiles=12, blocks=((0, 8), (8, 4)), n_point_tiles=64, n_split=32)

REDUCE_N = (1, 2, 15, 16, 17, 33, 64)
REDUCE_BLOCKS = ((5, 12), (32, 256))

BATCH_A_TILES, BATCH_B_TILES, BATCH_COUNT, BATCH_MAJOR = 10, 9, 40, 26


def case_id(c):
    return '-'.join('rs' if x is True else ('null' if x is False else str(x)) for x in c)


def _window(rng, nt_lo, nt_hi, tiles):
    nt = int(rng.integers(nt_lo, nt_hi + 1))
    return int(rng.integers(0, tiles - nt + 1)), nt


def batched_problems(x3, n_point_tiles):
    """The 40 windows (a_t0, a_nt, b_t0, b_nt, rowsum) of one vqn_wgrad_partials_batched call into operands of BATCH_A_TILES /
    BATCH_B_TILES feature tiles: 26 problems of the cheapest class reachable (more than WG_MAX: flushed in the middle of the loop),
    the other 14 dealt round-robin over every other reachable class, interleaved with them in submission order; every third problem
    has no row-sum workspace.  -> (problems, major class)."""
    rng = np.random.default_rng(17 + 2 * n_point_tiles + int(bool(x3)))
    shapes = {0: ((1, 4), (1, 4)), 1: ((1, 4), (5, 8)), 2: ((5, 8), (1, 8)), 3: ((8, 8), (8, 8)), 4: ((5, 8), (1, 8)), 5: ((1, 4), (1, 8))}
    reachable = sorted({partial_class(a, b, x3, n_point_tiles) for a in range(1, 9) for b in range(1, 9)})
    major = 5 if 5 in reachable else 0                      # the classes of at most four A tiles: the smallest workspaces
    others = [c for c in reachable if c != major]
    probs, k_other = [], 0
    for k in range(BATCH_COUNT):
        n_other = BATCH_COUNT - BATCH_MAJOR
        if (k * n_other) // BATCH_COUNT != ((k + 1) * n_other) // BATCH_COUNT:
            cls = others[k_other % len(others)]
            k_other += 1
        else:
            cls = major
        for _ in range(1000):
            (a_lo, a_hi), (b_lo, b_hi) = shapes[cls]
            a_t0, a_nt = _window(rng, a_lo, a_hi, BATCH_A_TILES)
            b_t0, b_nt = _window(rng, b_lo, b_hi, BATCH_B_TILES)
            if partial_class(a_nt, b_nt, x3, n_point_tiles) == cls:
                break
        else:
            raise AssertionError(f'no window of class {cls}')
        probs.append((a_t0, a_nt, b_t0, b_nt, k % 3 != 2))
    return probs, major


def thin_batch_problems():
    """25 (> TH_MAX) thin problems (a_t0, a_row0, a_rows, b_t0, b_nt, rowsum) into operands of 3 / 9 feature tiles."""
    rng = np.random.default_rng(29)
    probs = []
    for k in range(25):
        a_rows = (1, 3, 8, 2, 5)[k % 5]
        b_t0, b_nt = _window(rng, 1, 8, 9)
        probs.append((int(rng.integers(0, 3)), int(rng.integers(0, 32 - a_rows + 1)), a_rows, b_t0, b_nt, k % 4 != 1))
    return probs


# ------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=8)
def int_operand(n_point_tiles, tiles, seed):
    """TFMT tensor of integers in [-8, 8] as float32 (shared and cached: treat as read-only)."""
    g = torch.Generator().manual_seed(1000003 * seed + 31 * n_point_tiles + tiles)
    return torch.randint(-INT_MAX, INT_MAX + 1, (n_point_tiles, tiles, 32, 32), generator=g).to(torch.float32)


def real_operands(n_point_tiles, a_tiles, b_tiles, seed):
    """The recipe of test_bf16x3_weight_gradient_contraction_matches_the_f32_one: A = randn exp(4 randn per point) 1e-6 (eight
    decades of operand scale), B = randn."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((n_point_tiles, a_tiles, 32, 32), generator=g) * torch.exp(torch.randn((n_point_tiles, 1, 1, 32), generator=g) * 4.0) * 1e-6
    B = torch.randn((n_point_tiles, b_tiles, 32, 32), generator=g)
    return A, B


def poisoned(T, t0, nt, row0=None, rows=None):
    """A copy of T with NaN in every feature tile outside [t0, t0 + nt) -- and, for the thin kernel's A operand, in every row of
    tile t0 outside [row0, row0 + rows)."""
    P = torch.full_like(T, float('nan'))
    P[:, t0:t0 + nt] = T[:, t0:t0 + nt]
    if row0 is not None:
        assert nt == 1
        P[:, t0, :row0] = float('nan')
        P[:, t0, row0 + rows:] = float('nan')
    return P


def window_rows(T, t0, nt, tiles=None):
    """float64 [nt * 32 features, points] of the feature tiles [t0, t0 + nt) of the point tiles `tiles` (default: all, in order)."""
    W = T[:, t0:t0 + nt] if tiles is None else T[tiles, t0:t0 + nt]
    return W.permute(1, 2, 0, 3).reshape(nt * 32, -1).to(torch.float64)


def assert_headroom(*operands, n_points, what=''):
    """Every product of two of the integer operands' entries summed over n_points points, and every sum of one operand's entries,
    stays below 2^24: all partial sums are integers float32 holds exactly, so any summation order gives the same float32 result.
    Judged from the operands alone: max|a| max|b| n_points."""
    m = [float(T.abs().max()) for T in operands]
    for T in operands:
        assert torch.equal(T, T.round()) and bool(torch.isfinite(T).all()), f'{what}: operands are not integers'
    bound = max(m) ** 2 * n_points
    assert bound < 2 ** 24, f'{what}: sums up to {bound:.3g} do not fit float32 exactly'
    return bound


def n_blocks(n_point_tiles, n_split):
    return min(n_split, n_point_tiles)


def block_tiles(s, n, n_point_tiles):
    """point tiles summed into partial block s of n: s, s + n, s + 2 n, ..."""
    return list(range(s, n_point_tiles, n))


def partials_reference(A, a_t0, a_nt, B, b_t0, b_nt, n_point_tiles, n_split):
    """-> (n, blocks [n, 32 a_nt, 32 b_nt], row sums [n, 32 a_nt]) in float64: block s = sum over its point tiles of A[o][p] B[i][p]."""
    n = n_blocks(n_point_tiles, n_split)
    ws = torch.empty((n, a_nt * 32, b_nt * 32), dtype=torch.float64)
    rs = torch.empty((n, a_nt * 32), dtype=torch.float64)
    for s in range(n):
        t = block_tiles(s, n, n_point_tiles)
        Aw, Bw = window_rows(A, a_t0, a_nt, t), window_rows(B, b_t0, b_nt, t)
        ws[s] = Aw @ Bw.T
        rs[s] = Aw.sum(1)
    return n, ws, rs


def thin_reference(A, a_t0, a_row0, a_rows, B, b_t0, b_nt, n_point_tiles, n_split):
    """-> (n, blocks [n, 32 b_nt, 8] TRANSPOSED with columns >= a_rows zero, row sums [n, 32] with entries >= a_rows zero), float64."""
    n = n_blocks(n_point_tiles, n_split)
    ws = torch.zeros((n, b_nt * 32, 8), dtype=torch.float64)
    rs = torch.zeros((n, 32), dtype=torch.float64)
    for s in range(n):
        t = block_tiles(s, n, n_point_tiles)
        Aw = window_rows(A, a_t0, 1, t)[a_row0:a_row0 + a_rows]
        ws[s, :, :a_rows] = window_rows(B, b_t0, b_nt, t) @ Aw.T
        rs[s, :a_rows] = Aw.sum(1)
    return n, ws, rs


@functools.lru_cache(maxsize=4)
def exact_partial_case(case):
    """Integer operands of one PARTIAL_CASES tuple and its reference: dict(A, B (clean), Ap, Bp (poisoned), n, ws, rs (float32: the
    exact values)).  Cached: shared by the tests of a case, read-only."""
    a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt, npt, n_split, _ = case
    A, B = int_operand(npt, a_tiles, 1), int_operand(npt, b_tiles, 2)
    assert_headroom(A, B, n_points=32 * npt, what=case_id(case))
    n, ws, rs = partials_reference(A, a_t0, a_nt, B, b_t0, b_nt, npt, n_split)
    return dict(A=A, B=B, Ap=poisoned(A, a_t0, a_nt), Bp=poisoned(B, b_t0, b_nt), n=n, ws=exact32(ws), rs=exact32(rs))


def exact32(x64):
    """float64 integers -> float32, asserting that nothing is lost"""
    x32 = x64.to(torch.float32)
    assert torch.equal(x32.to(torch.float64), x64) and float(x64.abs().max()) < 2 ** 24
    return x32


@functools.lru_cache(maxsize=2)
def batched_reference(n_point_tiles, n_split):
    """The shared integer operands of the batched calls and ALL their partial blocks at once ([n, 320, 288] float32, exact): problem
    (a_t0, a_nt, b_t0, b_nt) owns the slice [:, 32 a_t0 : 32 (a_t0 + a_nt), 32 b_t0 : 32 (b_t0 + b_nt)]."""
    A, B = int_operand(n_point_tiles, BATCH_A_TILES, 3), int_operand(n_point_tiles, BATCH_B_TILES, 4)
    assert_headroom(A, B, n_points=32 * n_point_tiles, what='batched')
    n, ws, rs = partials_reference(A, 0, BATCH_A_TILES, B, 0, BATCH_B_TILES, n_point_tiles, n_split)
    return dict(A=A, B=B, n=n, ws=exact32(ws), rs=exact32(rs))


# ------------------------------------------------------------------------------------------------------------- guarded buffers
def guarded_layout(used, spare=0):
    """A buffer of `used` floats the kernel may write and `spare` it may not, between two guards: -> (total floats, offset of the
    buffer).  Everything but [offset, offset + used) must still be NaN afterwards."""
    return GUARD + used + spare + GUARD, GUARD


def untouched(full, used):
    """full: the flat NaN-filled allocation of guarded_layout after the kernel ran -> True if all of it outside the `used` floats
    behind the front guard is still NaN."""
    return bool(torch.isnan(full[:GUARD]).all()) and bool(torch.isnan(full[GUARD + used:]).all())


# ------------------------------------------------------------------------------------------------------------- ordered sums
def reduce_restatement(ws, out=None):
    """vqn_reduce_partials' documented order in numpy float32: 16 groups of ceil(n / 16) consecutive blocks, each summed in block
    order from zero; the 16 group sums added in group order; then, accumulating, `out` added.  ws [n, ...] float32."""
    ws = np.asarray(ws, np.float32)
    n = ws.shape[0]
    per = (n + 15) >> 4
    t = None
    for g in range(16):
        acc = np.zeros(ws.shape[1:], np.float32)
        for s in range(g * per, min(n, g * per + per)):
            acc = acc + ws[s]
        t = acc if g == 0 else t + acc
    if out is not None:
        t = t + np.asarray(out, np.float32)
    assert t.dtype == np.float32
    return t


def reduce_bound(ws, out=None):
    """(float64 sum, rounding bound): n float32 additions (n - 1 between the blocks -- the zeros the groups start from add nothing --
    and one for `out`) lose at most gamma_n <= (n + 1) 2^-24 of the sum of the terms' magnitudes."""
    ws64 = np.asarray(ws, np.float64)
    s, m = ws64.sum(0), np.abs(ws64).sum(0)
    if out is not None:
        s, m = s + np.asarray(out, np.float64), m + np.abs(np.asarray(out, np.float64))
    return s, (ws64.shape[0] + 1) * U * m


def finalize_entries():
    """The 45 (> FIN_MAX) entries of the vqn_wgrad_finalize call: dicts of src_rows, src_cols, n, n2 (None: no ws2), scale,
    rows_valid, col_first, cols_valid, transposed, integer (integer partials: exact under scale 0.5).  Sizes mixed, so that the
    block -> entry lookup of the kernel matters; the 256 x 256 ones are few and of small n (memory)."""
    sizes = ((1, 32), (96, 8), (64, 96), (256, 256))
    scales = (1.0, 0.5, float(np.float32(1.0 / math.sqrt(2.0))))
    ents = []
    for k in range(45):
        rows, cols = sizes[(k + k // 4) % 4]
        n = REDUCE_N[k % 7]
        if (rows, cols) == (256, 256) and n > 17:
            n = REDUCE_N[k % 5]
        n2 = REDUCE_N[(k + 3) % 7 if rows < 256 else (k + 1) % 4] if k % 3 == 0 else None
        scale = scales[(k + k // 3) % 3]
        clip = k % 4
        rows_valid = rows if (clip & 1) == 0 or rows == 1 else rows - (1 + k % 3)
        cols_valid = cols if (clip & 2) == 0 else cols - (1 + k % 5)
        col_first = 0 if k % 3 != 1 else min(cols_valid - 1, 1 + (k % 7))
        ents.append(dict(src_rows=rows, src_cols=cols, n=n, n2=n2, scale=scale, rows_valid=rows_valid, col_first=col_first,
                         cols_valid=cols_valid, transposed=k % 2 == 1, integer=scale == 0.5))
    return ents
