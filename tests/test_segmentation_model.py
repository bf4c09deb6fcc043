"""CPU: known answers of the float64 statement of the segmentation scores (tests/segmentation_model.py), the statement against
scikit-learn where that is installed, and the three C-ABI rows of csrc/segmentation_metrics.hip against their header.

The bound of the scikit-learn comparison, 1e-14 absolute, is derived, not observed.  A macro score is the mean of m <= 65 correctly
rounded quotients in [0, 1]: each quotient is off by at most u = 2^-53, the i-th partial sum is at most i and rounded once (at most
i u), so the sum is off by at most (m + m (m + 1) / 2) u and the mean, after its own rounding, by at most (2 + (m + 1) / 2) u
<= 35 u = 3.9e-15 for m = 65, whatever the order of the additions.  Two such evaluations (the statement's order and numpy's) differ
by at most twice that, 7.8e-15 < 1e-14.  Purity and micro F1 are one quotient of exact integers: no error at all."""
import math

import numpy as np
import pytest

from tests import segmentation_model as S

SKLEARN_BOUND = 1e-14


def _scores_of(gt, pd, n_gt, n_pd, keep=None):
    return S.evaluate_labels(np.asarray(gt), np.asarray(pd), n_gt, n_pd, keep)


def test_perfect_segmentation_under_a_permutation_scores_one():
    gt = np.array([0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 3])
    perm = np.array([2, 3, 0, 1])
    r = _scores_of(gt, perm[gt], 3, 3)
    assert [r[k] for k in S.KEYS] == [1.0] * 5
    assert r['label_map'] == [2, 3, 0, 1] and r['total'] == 11 and r['invalid'] == 0 and (r['rows'], r['cols']) == (4, 4)


def test_two_clusters_on_one_class_and_a_class_nothing_maps_to():
    # gt 1: 5 pixels in cluster 1, 3 in cluster 2; gt 2: 2 in cluster 1, 1 in cluster 2 -> both clusters are read as class 1
    gt = [1] * 8 + [2] * 3
    pd = [1] * 5 + [2] * 3 + [1] * 2 + [2] * 1
    r = _scores_of(gt, pd, 2, 2)
    assert r['contingency'].tolist() == [[0, 0, 0], [0, 5, 3], [0, 2, 1]]
    assert r['label_map'] == [-1, 1, 1] and (r['rows'], r['cols']) == (2, 2)
    assert r['purity'] == 8.0 / 11.0 and r['f1-micro'] == 8.0 / 11.0
    assert r['p-macro'] == (8.0 / 11.0 + 0.0) / 2.0              # class 2: precision 0 (nothing predicted), it still counts
    assert r['r-macro'] == (1.0 + 0.0) / 2.0
    assert r['f1-macro'] == (16.0 / 19.0 + 0.0) / 2.0


def test_an_argmax_tie_picks_the_lowest_row():
    gt = [2, 2, 1, 1, 3]
    pd = [1, 1, 1, 1, 2]
    r = _scores_of(gt, pd, 3, 2)
    assert r['label_map'] == [-1, 1, 3]
    gt0 = [2, 2, 0, 0]                                           # class 0 is a class like any other
    assert _scores_of(gt0, [1, 1, 1, 1], 2, 1)['label_map'] == [-1, 0]


@pytest.mark.parametrize('seed', range(8))
def test_f1_micro_equals_purity_exactly(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 3000))
    gt = rng.integers(0, 22, n) * (rng.random(n) < 0.7)
    pd = rng.integers(0, 22, n) * (rng.random(n) < 0.6)
    r = _scores_of(gt, pd, 21, 21)
    assert r['f1-micro'] == r['purity'] and 0.0 < r['purity'] <= 1.0
    assert int(r['contingency'].sum()) == n == r['total']


def test_the_two_palettes_differ_at_half_intensity():
    assert S.GT_PALETTE.shape == (21, 3) and S.PD_PALETTE.shape == (21, 3)
    assert (S.GT_PALETTE == 127).sum() == (S.PD_PALETTE == 128).sum() == 21 and not (S.GT_PALETTE == 128).any() and not (S.PD_PALETTE == 127).any()
    px = np.array([[128, 0, 0], [127, 0, 0], [255, 0, 0], [1, 2, 3], [0, 255, 127], [0, 255, 128]], np.uint8)
    assert S.palette_labels(px, S.GT_PALETTE).tolist() == [0, 7, 1, 0, 21, 0]
    assert S.palette_labels(px, S.PD_PALETTE).tolist() == [7, 0, 1, 0, 0, 21]
    twice = np.array([[9, 9, 9], [9, 9, 9], [1, 1, 1]], np.uint8)             # a repeated row: the first one names the label
    assert S.palette_labels(np.array([[9, 9, 9], [1, 1, 1]], np.uint8), twice).tolist() == [1, 3]
    r = S.evaluate_rgb(px, px, None)
    assert r['contingency'][0, 7] == 1 and r['contingency'][7, 0] == 1 and r['contingency'][1, 1] == 1 and r['contingency'][0, 0] == 1
    assert r['contingency'].shape == (22, 22) and r['total'] == 6


def test_a_pixel_at_the_threshold_is_not_counted():
    thres = 0.8
    above = np.nextafter(np.float32(thres), np.float32(2))
    alpha = np.array([thres, above, 0.0, 1.0, np.float32(thres)], np.float32)
    assert S.counted(alpha, thres).tolist() == [False, True, False, True, False]
    px = np.tile(np.array([[255, 0, 0]], np.uint8), (5, 1))
    r = S.evaluate_rgb(px, px, alpha, thres)
    assert r['total'] == 2 and r['contingency'][1, 1] == 2


def test_no_counted_pixel_gives_nan():
    r = _scores_of([1, 2], [1, 2], 2, 2, keep=[0, 0])
    assert r['total'] == 0 and all(math.isnan(r[k]) for k in S.KEYS) and r['label_map'] == [-1, -1, -1] and (r['rows'], r['cols']) == (0, 0)
    r = _scores_of([], [], 2, 2)
    assert all(math.isnan(r[k]) for k in S.KEYS)


def test_labels_out_of_range_are_invalid_and_stay_out_of_the_table():
    r = _scores_of([0, 1, 3, -1, 2, 1], [0, 1, 0, 0, 5, 1], 2, 4)
    assert r['invalid'] == 3 and r['total'] == 3 and r['contingency'][1, 1] == 2 and r['contingency'][0, 0] == 1


def _resort(arr):
    """the reference's `resort`: the labels that occur, renumbered 0, 1, ... in ascending order"""
    return np.unique(arr, return_inverse=True)[1].reshape(-1)


@pytest.mark.parametrize('seed', range(40))
def test_statement_against_scikit_learn(seed):
    metrics = pytest.importorskip('sklearn.metrics')
    cluster = pytest.importorskip('sklearn.metrics.cluster')
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 4001)) if seed > 3 else (1, 2, 3999, 4000)[seed]
    k_gt, k_pd = int(rng.integers(1, 23)), int(rng.integers(1, 23))
    w_gt, w_pd = rng.random(k_gt) ** 4 + 1e-3, rng.random(k_pd) ** 4 + 1e-3              # skewed class frequencies
    gt = rng.choice(rng.permutation(22)[:k_gt], n, p=w_gt / w_gt.sum())
    pd = np.where(rng.random(n) < 0.6, (gt * 7 + 3) % 22, rng.choice(rng.permutation(22)[:k_pd], n, p=w_pd / w_pd.sum()))
    mine = _scores_of(gt, pd, 21, 21)
    # cluster_eval.py: correspond, then the five scores
    g, p = _resort(gt), _resort(pd)
    coo = np.asarray(cluster.contingency_matrix(g, p))
    rows, cols = np.flatnonzero(mine['contingency'].sum(1)), np.flatnonzero(mine['contingency'].sum(0))
    np.testing.assert_array_equal(mine['contingency'][np.ix_(rows, cols)], coo)
    label_map = np.argmax(coo, axis=0)
    assert [mine['label_map'][c] for c in cols] == [int(rows[i]) for i in label_map]
    replaced = label_map[p]
    want = {'purity': np.sum(np.max(coo, axis=0)) / np.sum(coo), 'f1-micro': metrics.f1_score(g, replaced, average='micro'),
            'f1-macro': metrics.f1_score(g, replaced, average='macro'),
            'p-macro': metrics.precision_score(g, replaced, average='macro', zero_division=0),
            'r-macro': metrics.recall_score(g, replaced, average='macro')}
    for k in S.KEYS:
        assert abs(mine[k] - float(want[k])) <= SKLEARN_BOUND, (k, mine[k], want[k])


def test_the_three_prototypes_equal_their_abi_rows():
    from tests import abi_headers
    from vqnerf_release_amd import _C
    declared, table = abi_headers.prototypes('vqn_eval.h'), _C.ABI_BY_HEADER['vqn_eval.h']
    names = ('vqn_seg_scratch_bytes', 'vqn_seg_contingency_rgb', 'vqn_seg_contingency_labels')
    for name in names:
        assert declared[name] == table[name], name
    assert table['vqn_seg_scratch_bytes'] == ('l', 'lii')
    assert table['vqn_seg_contingency_rgb'][1].endswith('p') and table['vqn_seg_contingency_labels'][0] == 'i'


def test_the_package_palettes_are_the_statement_s():
    from vqnerf_release_amd.decomp.nerfactor.util import segmentation
    np.testing.assert_array_equal(segmentation.GT_PALETTE, S.GT_PALETTE)
    np.testing.assert_array_equal(segmentation.PD_PALETTE, S.PD_PALETTE)
    assert segmentation.GT_PALETTE[6].tolist() == [127, 0, 0] and segmentation.PD_PALETTE[6].tolist() == [128, 0, 0]
    assert segmentation.KEYS == S.KEYS == ('purity', 'f1-micro', 'f1-macro', 'p-macro', 'r-macro')
