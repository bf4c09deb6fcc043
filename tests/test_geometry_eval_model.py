"""CPU: the NumPy statement of the geometry scores (tests/geometry_eval_model.py) -- its float32 brute-force nearest neighbour against
scipy's k-d tree in float64, its sampler against closed forms, and known answers of its scores."""
import math

import numpy as np
import pytest

from tests import geometry_eval_model as gm


def kd_inputs():
    """the inputs of the k-d tree comparison, which the GPU tests share"""
    rng = np.random.default_rng(0)
    ref = rng.random((3000, 3), dtype=np.float32)
    query = rng.random((4096, 3), dtype=np.float32)
    return query, ref


def test_nearest_equals_a_float64_kd_tree():
    spatial = pytest.importorskip('scipy.spatial')
    query, ref = kd_inputs()
    d2, idx = gm.nearest(query, ref)
    dist, want = spatial.cKDTree(ref.astype(np.float64)).query(query.astype(np.float64), k=2)
    gap = (dist[:, 1] ** 2 - dist[:, 0] ** 2) / dist[:, 1] ** 2
    assert gap.min() > 1e-5                                   # no query whose two best are close enough for float32 to swap them
    assert np.array_equal(idx, want[:, 0])
    rel = np.abs(d2.astype(np.float64) - dist[:, 0] ** 2) / dist[:, 0] ** 2
    print(f'largest relative d2 difference {rel.max():.3e}')
    assert rel.max() <= 6 * 2.0 ** -24                        # three differences, three products, two sums


def test_nearest_ties_go_to_the_lowest_index_and_the_cap_is_strict():
    ref = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 3]], np.float32)
    query = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    d2, idx = gm.nearest(query, ref)
    assert idx.tolist() == [0, 0, 0] and d2.tolist() == [1.0, 0.0, 2.0]
    d2, idx = gm.nearest(query, ref, max_d2=np.float32(1.0))
    assert idx.tolist() == [0, 0, -1] and d2.tolist() == [1.0, 0.0, np.inf]      # d2 = max_d2 stays: the rule is d2 > max_d2


def test_sampler():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [3, 0, 0], [0, 2, 0], [5, 5, 5], [5, 5, 5]], np.float32)
    t = np.array([[0, 1, 2], [6, 7, 6], [3, 4, 5]], np.int32)                    # areas 0.5, 0 (degenerate), 3
    areas = gm.tri_areas(v, t)
    assert areas.tolist() == [0.5, 0.0, 3.0]
    cum = np.cumsum(areas)
    u = np.stack([(np.arange(1000, dtype=np.float32) + 0.5) / 1000, np.full(1000, 0.25, np.float32), np.full(1000, 0.5, np.float32)], 1)
    p, n, f = gm.sample_surface(v, t, cum, u)
    assert (f != 1).all() and (f == 0).sum() == 143 and (f == 2).sum() == 857     # u0 * 3.5 < 0.5 for the first 143 of 1000
    assert np.array_equal(n, np.tile(np.float32([0, 0, 1]), (1000, 1)))
    # s = 0.5: a = 0.5, b = c = 0.25
    assert np.array_equal(p[0], np.float32([0.25, 0.25, 0])) and np.array_equal(p[-1], np.float32([0.75, 0.5, 0]))
    # x exactly on a boundary of the prefix sum goes to the next face with area; a degenerate face has a zero normal
    t2 = np.array([[0, 1, 2], [6, 7, 6], [0, 1, 2]], np.int32)                   # cum = 0.5, 0.5, 1
    _, _, f1 = gm.sample_surface(v, t2, np.cumsum(gm.tri_areas(v, t2)), np.float32([[0.5, 0, 0], [0.49999997, 0, 0]]))
    assert f1.tolist() == [2, 0]
    _, n2, _ = gm.sample_surface(v, t[1:2], np.array([0.0]), np.float32([[0.3, 0.3, 0.3]]))
    assert np.array_equal(n2, np.zeros((1, 3), np.float32))


def _plane(k=20, z=0.0, normal=1.0):
    g = (np.arange(k, dtype=np.float32) / np.float32(k))
    x, y = np.meshgrid(g, g, indexing='ij')
    pts = np.stack([x.ravel(), y.ravel(), np.full(k * k, z, np.float32)], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, normal]), (k * k, 1))
    return pts, nrm


def test_a_cloud_against_itself():
    pts = np.random.default_rng(1).random((500, 3), dtype=np.float32)
    s = gm.surface_scores(pts, None, pts, None, thresholds=(1e-6, 0.1))
    assert s['accuracy'] == 0.0 and s['completeness'] == 0.0 and s['chamfer'] == 0.0 and s['chamfer_l2'] == 0.0
    assert s['precision'] == [1.0, 1.0] and s['recall'] == [1.0, 1.0] and s['fscore'] == [1.0, 1.0]
    assert s['accuracy_max'] == 0.0 and s['n_pred'] == 500 and s['n_gt_valid'] == 500 and math.isnan(s['normal_consistency'])


def test_a_plane_against_its_shifted_copy():
    delta = 0.0625                                            # exact in float32; the nearest point is the one straight above
    a, an = _plane(20, 0.0)
    b, bn = _plane(20, delta)
    s = gm.surface_scores(a, an, b, bn, thresholds=(0.03, delta, 0.07))
    assert s['accuracy'] == delta and s['completeness'] == delta and s['chamfer'] == delta and s['chamfer_l2'] == delta * delta
    assert s['precision'] == [0.0, 0.0, 1.0] and s['recall'] == [0.0, 0.0, 1.0] and s['fscore'] == [0.0, 0.0, 1.0]
    assert s['accuracy_max'] == delta and s['normal_consistency'] == 1.0


def test_flipped_normals_are_consistent():
    a, an = _plane(12, 0.0, 1.0)
    s = gm.surface_scores(a, an, a, -an)
    assert s['normal_consistency'] == 1.0
    an[:5] = 0                                                # zero normals leave the normal sum, on either side
    r = gm.reduce(*gm.nearest(a, a), (), an, -an)
    assert r['pairs'] == len(a) - 5 and r['sum_dot'] == float(len(a) - 5)


def test_a_cap_below_the_distance_leaves_no_valid_query():
    a, an = _plane(10, 0.0)
    b, bn = _plane(10, 0.25)
    s = gm.surface_scores(a, an, b, bn, thresholds=(0.5,), max_dist=0.125)
    assert s['n_pred'] == 100 and s['n_gt'] == 100 and s['n_pred_valid'] == 0 and s['n_gt_valid'] == 0 and s['n_pred_far'] == 100
    for k in ('accuracy', 'completeness', 'chamfer', 'chamfer_l2', 'normal_consistency'):
        assert math.isnan(s[k]), k
    assert math.isnan(s['precision'][0]) and math.isnan(s['fscore'][0]) and s['accuracy_max'] == 0.0


def test_the_reduction_counts_and_sums():
    d2 = np.float32([0.0, 4.0, np.inf, 0.25, 9.0])
    idx = np.int32([0, 1, -1, 2, 0])
    r = gm.reduce(d2, idx, (0.5, 2.0, 2.5))
    assert r['n'] == 5 and r['n_valid'] == 4 and r['count'] == [1, 2, 3]          # d = 0, 2, 0.5, 3; d < tau is strict
    assert r['sum_d'] == 5.5 and r['sum_d2'] == 13.25 and r['max_d'] == 3.0
    s = gm.scores(r, r, (0.5, 2.0, 2.5))
    assert s['accuracy'] == 5.5 / 4 and s['precision'] == [0.25, 0.5, 0.75] and s['fscore'] == [0.25, 0.5, 0.75]
    zero = gm.reduce(np.float32([1.0]), np.int32([0]), (0.5,))
    assert gm.scores(zero, zero, (0.5,))['fscore'] == [0.0]                         # P + R = 0
