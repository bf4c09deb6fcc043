"""CPU: the float64 statement of mean-shift clustering (tests/meanshift_model.py) against sklearn.cluster.MeanShift and against
answers known by hand, the rows of the binding table, and the argument checks of the device wrapper
(decomp/nerfactor/util/meanshift.py) that raise before anything is launched."""
import numpy as np
import pytest
import torch

from tests import meanshift_model as M

# (n, D, k, sigma, seed), bandwidth: 3 .. 14 clusters found
SKLEARN_CASES = [((700, 3, 4, 0.06, 1), 0.3), ((1000, 7, 8, 0.07, 2), 0.2), ((1500, 8, 3, 0.1, 3), 0.5), ((2000, 7, 12, 0.05, 4), 0.2),
                 ((1200, 3, 6, 0.04, 5), 0.2), ((900, 8, 5, 0.08, 6), 0.3)]


@pytest.mark.parametrize('which', range(len(SKLEARN_CASES)))
def test_statement_matches_sklearn(which):
    cluster = pytest.importorskip('sklearn.cluster')
    spec, b = SKLEARN_CASES[which]
    X = M.blobs(*spec)
    ref = cluster.MeanShift(bandwidth=b, cluster_all=True).fit(X)
    got = M.fit(X, b)
    assert got['centres'].shape == ref.cluster_centers_.shape
    worst = np.abs(got['centres'] - ref.cluster_centers_).max()
    print(f'[statement vs sklearn] {spec} b={b}: K={len(got["centres"])} n_iter={got["n_iter"]} centres differ by {worst:.2e} {got["margins"]}')
    assert worst <= 1e-14
    assert got['n_iter'] == ref.n_iter_
    np.testing.assert_array_equal(got['labels'], ref.labels_)
    fresh = np.random.default_rng(100 + spec[4]).random((5000, spec[1]))
    np.testing.assert_array_equal(M.assign(fresh, got['centres'])[0], ref.predict(fresh))


def test_blobs_stay_in_the_unit_cube():
    X = M.blobs(517, 1, 3, 0.05, 14)
    assert X.shape == (517, 1) and X.min() >= 0 and X.max() <= 1 and X.dtype == np.float64


def test_two_far_pairs_give_their_midpoints():
    X = np.array([[0.1, 0.1], [0.2, 0.1], [0.8, 0.9], [0.8, 0.7]])
    got = M.fit(X, 0.25)
    assert got['counts'].tolist() == [2, 2, 2, 2] and got['distinct'] == 2 and got['n_iter'] == 1
    # equal counts: descending by the coordinates
    np.testing.assert_array_equal(got['centres'], np.array([[(0.8 + 0.8) / 2, (0.9 + 0.7) / 2], [(0.1 + 0.2) / 2, (0.1 + 0.1) / 2]]))
    assert got['labels'].tolist() == [1, 1, 0, 0]


def test_a_seed_beyond_the_bandwidth_is_dropped_and_all_dropped_raises():
    X = np.array([[0.1, 0.1], [0.2, 0.1], [0.8, 0.9]])
    seeds = np.array([[0.15, 0.1], [0.5, 0.5], [0.8, 0.9]])
    means, counts, iters, _ = M.seek(X, seeds, 0.2)
    assert counts.tolist() == [2, 0, 1] and iters.tolist() == [0, 0, 0]
    np.testing.assert_array_equal(means[1], seeds[1])                        # a dropped seed stays where it was
    got = M.fit(X, 0.2, seeds=seeds)
    np.testing.assert_array_equal(got['centres'], np.array([[(0.1 + 0.2) / 2, 0.1], [0.8, 0.9]]))
    with pytest.raises(ValueError, match='bandwidth'):
        M.fit(X, 0.2, seeds=np.array([[0.5, 0.5], [0.5, 0.1]]))


def test_max_iter_zero_is_one_mean_step():
    X = M.blobs(300, 3, 2, 0.1, 7)
    means, counts, iters, _ = M.seek(X, X, 0.3, max_iter=0)
    assert (iters == 0).all() and (counts > 0).all()
    near = M.dist2(X[None, :, :], X[:, None, :]) <= 0.3 * 0.3
    np.testing.assert_array_equal(means, np.stack([X[r].mean(axis=0) for r in near]))
    one = M.seek(X, X, 0.3, max_iter=1)[2]
    assert set(one.tolist()) <= {0, 1} and one.max() == 1


def test_a_bandwidth_beyond_the_diameter_gives_the_data_mean():
    X = M.blobs(200, 7, 5, 0.1, 8)
    got = M.fit(X, 4.0)
    assert len(got['centres']) == 1 and got['distinct'] == 1 and (got['counts'] == 200).all() and (got['labels'] == 0).all()
    np.testing.assert_array_equal(got['centres'][0], X.mean(axis=0))
    assert got['n_iter'] == 1 and got['margins']['label_gap'] == np.inf      # the second step does not move: the same 200 neighbours


def test_duplicate_points_count_as_often_as_they_occur():
    X = np.array([[0.25, 0.5]] * 3 + [[0.75, 0.5]] * 2 + [[0.5, 0.5]])
    got = M.fit(X, 0.1)
    assert got['counts'].tolist() == [3, 3, 3, 2, 2, 1] and got['distinct'] == 3
    np.testing.assert_array_equal(got['centres'], np.array([[0.25, 0.5], [0.75, 0.5], [0.5, 0.5]]))
    assert got['labels'].tolist() == [0, 0, 0, 1, 1, 2] and got['n_iter'] == 0
    lab, dist, gap = M.assign(np.array([[0.5, 0.5], [0.375, 0.5], [0.0, 0.5]]), got['centres'], b=0.2)
    assert lab.tolist() == [2, 0, -1] and gap == 0.0                         # 0.375 is as far from 0.25 as from 0.5: the lowest index


def test_binding_table_has_the_mean_shift_rows():
    from vqnerf_release_amd import _C
    table = _C.ABI_BY_HEADER['vqn_eval.h']
    assert table['vqn_meanshift_seek'] == ('i', 'plplidipppp') and table['vqn_meanshift_merge_scratch_bytes'] == ('l', 'li')
    assert table['vqn_meanshift_merge'] == ('i', 'pplidplppp') and table['vqn_meanshift_assign'] == ('i', 'plpiidppp')
    assert (_C.MEANSHIFT_POINTS_PER_TILE, _C.MEANSHIFT_SEEDS_PER_GROUP, _C.MEANSHIFT_MAX_DIM) == (256, 64, 8)


def test_wrapper_refuses_bad_arguments_before_any_launch():
    from vqnerf_release_amd.decomp.nerfactor.util import meanshift
    x = np.zeros((10, 3))
    for bad in (0.0, -0.2, float('nan')):
        with pytest.raises(ValueError, match='bandwidth'):
            meanshift.MeanShift(bad).fit(x)
    with pytest.raises(ValueError, match='max_iter'):
        meanshift.MeanShift(0.2, max_iter=-1).fit(x)
    with pytest.raises(ValueError, match='at most 8'):
        meanshift.MeanShift(0.2).fit(np.zeros((10, 9)))
    with pytest.raises(ValueError, match='empty'):
        meanshift.MeanShift(0.2).fit(np.zeros((0, 3)))
    with pytest.raises(ValueError, match='empty'):
        meanshift.MeanShift(0.2).fit(torch.zeros((0, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=r'\[n, D\]'):
        meanshift.MeanShift(0.2).fit(np.zeros(10))
    with pytest.raises(ValueError, match='features per point'):
        meanshift.MeanShift(0.2, seeds=np.zeros((4, 2))).fit(x)
    with pytest.raises(ValueError, match='float32, float64 or uint8'):
        meanshift.MeanShift(0.2).fit(np.zeros((10, 3), np.int32))
    model = meanshift.MeanShift(0.2)
    with pytest.raises(ValueError, match='before fit'):
        model.predict(x)
    model.cluster_centers_ = torch.zeros((2, 3), dtype=torch.float64)        # as after a fit on three features
    with pytest.raises(ValueError, match='fitted on 3'):
        model.predict(np.zeros((10, 5)))
    with pytest.raises(ValueError, match='empty'):
        model.predict(np.zeros((0, 3)))
    assert meanshift._UNIT8.dtype == np.float64 and meanshift._UNIT8[51] == 51 / 255. and meanshift._UNIT8[255] == 1.0
