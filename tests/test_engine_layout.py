"""CPU: the three engine layouts of vqnerf_release_amd/geo/packing.py (`LAYOUTS`) against their plain definition -- the formulas of
that module's docstring written out as literal loops over (tile, step, lane, slot) -- on a two-segment K with ragged tails:
33 output rows (two tiles, one row in the second), a 40-feature segment and a 27-feature one at column base 40.  The steps of
the two segments (f32: 5 + 4 rows, f16s and x3: 3 + 2 steps) are no whole A block for f16s (blocks of 4) and x3 (blocks of 2), so
the padding steps are part of the case."""
import numpy as np
import pytest

from vqnerf_release_amd.geo import packing

N_OUT, FEATS, N_COLS = 33, (40, 27), 67


def _phi(i):
    return 2 * (i & 3) + 8 * (i >> 3) + ((i >> 2) & 1)


def _feature(name, s, h, j):
    return 32 * (s >> 2) + 2 * (4 * (s & 3) + j) + h if name == 'f32' else 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)


@pytest.mark.parametrize('name', ['f32', 'f16s', 'x3'])
def test_layout_matches_its_definition(name):
    lay = packing.LAYOUTS[name]
    rows_per_step, step_feats, block, slots = {'f32': (1, 8, 1, 4), 'f16s': (2, 16, 4, 8), 'x3': (3, 16, 2, 8)}[name]
    assert lay.rows_per_tile == rows_per_step * 32 // step_feats and lay.block_steps == block
    steps = [-(-f // step_feats) for f in FEATS]
    assert [lay.rows_for(f) for f in FEATS] == [rows_per_step * s for s in steps]
    segs = [(lay.rows_for(FEATS[0]), FEATS[0], 0), (lay.rows_for(FEATS[1]), FEATS[1], FEATS[0])]
    # column of the matrix held by (step of the concatenated K, lane half, slot); None = padding
    col = {}
    s_all = 0
    for (rows, n_valid, base), n_steps in zip(segs, steps):
        kf = lay.k_features(rows)
        assert kf.shape == (n_steps, 64, slots)
        for s in range(n_steps):
            for lane in range(64):
                for j in range(slots):
                    f = _feature(name, s, lane >> 5, j)
                    assert kf[s, lane, j] == f
                    col[s_all, lane >> 5, j] = base + f if f < n_valid else None
            s_all += 1
    padded = -(-s_all // block) * block
    assert padded > s_all or name == 'f32'
    zero = N_OUT * N_COLS
    g = lay.gemm_index(N_OUT, N_COLS, segs)
    assert g.shape == (2, padded, 64, slots) and g.dtype == np.int64
    for t in range(2):
        for s in range(padded):
            for lane in range(64):
                row = 32 * t + (_phi(lane & 31) if name == 'f32' else lane & 31)
                for j in range(slots):
                    c = col.get((s, lane >> 5, j))
                    assert g[t, s, lane, j] == (row * N_COLS + c if (row < N_OUT and c is not None) else zero), (t, s, lane, j)
    r = lay.rowdot_index(N_OUT, N_COLS, segs)
    assert r.shape == (N_OUT, s_all, 2, slots) and r.dtype == np.int64
    for o in range(N_OUT):
        for s in range(s_all):
            for h in range(2):
                for j in range(slots):
                    c = col[s, h, j]
                    assert r[o, s, h, j] == (o * N_COLS + c if c is not None else zero), (o, s, h, j)
    b = lay.bias_index(N_OUT)
    assert b.shape == (2, 2, 16) and b.dtype == np.int64
    for t in range(2):
        for h in range(2):
            for reg in range(16):
                f = 32 * t + (2 * reg + h if name == 'f32' else (reg & 3) + 8 * (reg >> 2) + 4 * h)
                assert b[t, h, reg] == (f if f < N_OUT else N_OUT)


def test_default_segment_and_column_function_escape():
    """no segments = the whole tiles of all columns; (rows, col_fn) = any other column map"""
    for lay in packing.LAYOUTS.values():
        whole = [(lay.rows_per_tile * 2, 40, 0)]
        assert lay.tile_seg(40) == whole[0]
        assert (lay.gemm_index(33, 40) == lay.gemm_index(33, 40, whole)).all()
        assert (lay.rowdot_index(3, 40) == lay.rowdot_index(3, 40, whole)).all()
        fn = lambda f: np.where(f < 40, f, -1)
        assert (lay.gemm_index(33, 40, [(whole[0][0], fn)]) == lay.gemm_index(33, 40, whole)).all()
