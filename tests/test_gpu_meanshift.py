"""GPU: mean-shift clustering of csrc/meanshift.hip (decomp/nerfactor/util/meanshift.py, decomp/meanshift.py) against its float64
statement tests/meanshift_model.py.

Neighbour counts, completed iterations, n_iter_, K, labels_, predict, the number of distinct means and the order of the centres must
EQUAL the statement's.  That comparison is valid only while device and statement take the same discrete decisions, so every case
first asserts, from the statement's own record, that no decision was close: |d2 - b^2| >= 1e-10 for every (seed, iteration, point) and
every pair the merge compares, |shift - 1e-3 b| >= 1e-10 for every step, and >= 1e-9 between a point's nearest and second nearest
centre.  These are conditions on the INPUTS (another seed is picked when one misses them), not tolerances: the device's mean differs
from the statement's by at most about n 2^-53 per coordinate, which moves d2 by ~1e-12.

Means and centres are held to 2 n 2^-53 absolute, n the number of points: a sequential float64 sum of c <= n values in [0, 1] is
within (c - 1) 2^-53 c of exact, dividing by c leaves less than n 2^-53, and the statement's own pairwise sum and the two final
divisions add less than that again.  Observed on an MI355X: profiles/observed_errors_meanshift.json.

Sizes are written in the kernels' constants: T points per staged tile and G seeds per workgroup of the seek kernel, SPAN points per
workgroup pass and CEN resident centres of the assign kernel."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import meanshift_model as M
from tests import segmentation_model as S
from tests.gpu_util import launches, record_observed

pytestmark = pytest.mark.gpu

ONE_FIT = {'vqn_meanshift_seek': 1, 'vqn_meanshift_merge': 1, 'vqn_meanshift_assign': 1}


def _consts():
    from vqnerf_release_amd import _C
    return _C.MEANSHIFT_POINTS_PER_TILE, _C.MEANSHIFT_SEEDS_PER_GROUP, _C.MEANSHIFT_ASSIGN_SPAN, _C.MEANSHIFT_ASSIGN_CENTRES


def _dev():
    return torch.device('cuda:0')


def _bound(n):
    return 2.0 * n * 2.0 ** -53


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case(spec, b, max_iter=300, cluster_all=True, n_seeds=None, seed_kind='points'):
    """(n, D, k, sigma, seed) -> (X, seeds or None, the statement's fit or the ValueError it raises)
    seed_kind: 'points' the first n_seeds samples, 'cube' uniform in [0, 1]^D (some have no neighbour), 'far' beyond every point"""
    X = M.blobs(*spec)
    seeds = None
    if n_seeds is not None:
        rng = np.random.default_rng(1000 + spec[4])
        seeds = {'points': lambda: X[:n_seeds].copy(), 'cube': lambda: rng.random((n_seeds, spec[1])),
                 'far': lambda: 3.0 + rng.random((n_seeds, spec[1]))}[seed_kind]()
    try:
        ref = M.fit(X, b, max_iter, cluster_all, seeds)
        _frozen(*[v for v in ref.values() if isinstance(v, np.ndarray)])
    except ValueError as e:
        ref = e
    _frozen(X, seeds)
    return X, seeds, ref


def _assert_margins(ref, case):
    m = ref['margins']
    print(f'[margins] {case}: {m} n_iter={ref["n_iter"]} K={len(ref["centres"])} distinct={ref["distinct"]}')
    assert m['distance'] >= 1e-10 and m['shift'] >= 1e-10 and m['merge'] >= 1e-10 and m['label_gap'] >= 1e-9, (case, m)


def _check_fit(test, case, X, seeds, ref, b, max_iter=300, cluster_all=True, x_dev=None):
    """fits on the device (x_dev: what is handed to fit, default X as a float64 device tensor) and holds everything to `ref`"""
    from vqnerf_release_amd.decomp.nerfactor.util import meanshift
    _assert_margins(ref, case)
    n = X.shape[0]
    model = meanshift.MeanShift(b, max_iter=max_iter, cluster_all=cluster_all, seeds=None if seeds is None else seeds.copy())
    with launches() as rec:
        model.fit(torch.tensor(X, device=_dev()) if x_dev is None else x_dev)
    assert rec.counts == ONE_FIT, (case, rec.counts)                         # every seed to convergence in ONE seek launch
    counts, iters, means = model.counts_.cpu().numpy(), model.iters_.cpu().numpy(), model.means_.cpu().numpy()
    np.testing.assert_array_equal(counts, ref['counts'], err_msg=case)
    np.testing.assert_array_equal(iters, ref['iters'], err_msg=case)
    assert model.n_iter_ == ref['n_iter'], case
    found = counts > 0
    assert len(np.unique(means[found], axis=0)) == ref['distinct'], case     # equal neighbour sets: bit-identical means
    start = X if seeds is None else seeds
    np.testing.assert_array_equal(means[~found], start[~found], err_msg=case)           # a dropped seed stays where it was
    centres = model.cluster_centers_.cpu().numpy()
    assert model.cluster_centers_.dtype == torch.float64 and model.cluster_centers_.is_cuda
    assert centres.shape == ref['centres'].shape, (case, centres.shape, ref['centres'].shape)        # K
    worst = max(float(np.abs(means - ref['means']).max()), float(np.abs(centres - ref['centres']).max()))          # row by row: the order
    record_observed(test, case, worst, _bound(n))
    assert worst <= _bound(n), (case, worst)
    np.testing.assert_array_equal(model.labels_.cpu().numpy(), ref['labels'], err_msg=case)
    assert model.labels_.dtype == torch.int32
    return model


def _check_predict(model, ref, D, n, case, seed=0):
    fresh = np.random.default_rng(77 + seed).random((n, D))
    want, _, gap = M.assign(fresh, ref['centres'])
    assert gap >= 1e-9, (case, gap)
    with launches() as rec:
        got = model.predict(fresh)                                           # numpy in
    assert rec.counts == {'vqn_meanshift_assign': 1}
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=case)


# the full fits whose margins the statement was measured on: every sample a seed; D = 3, 8, 1, 7; n is no multiple of T or G
FULL = [((1031, 3, 4, 0.06, 12), 0.3), ((2053, 8, 3, 0.1, 13), 0.5), ((517, 1, 3, 0.05, 14), 0.2), ((4099, 7, 8, 0.07, 3), 0.2)]


@pytest.mark.parametrize('which', range(len(FULL)))
def test_full_fit_matches_the_statement(which):
    T, G, SPAN, CEN = _consts()
    spec, b = FULL[which]
    X, seeds, ref = _case(spec, b)
    case = f'{spec} b={b}'
    model = _check_fit('test_full_fit_matches_the_statement', case, X, seeds, ref, b)
    assert len(ref['centres']) == (3, 3, 2, 9)[which] and ref['n_iter'] == (9, 4, 13, 10)[which]
    if which == 3:
        assert ref['distinct'] == 58                                         # 58 distinct means merge into the 9 centres
    _check_predict(model, ref, spec[1], 19 * SPAN + 136, case, seed=which)   # no multiple of the assign kernel's span


@pytest.mark.parametrize('which', range(5))
def test_point_counts_around_the_staged_tile(which):
    T, G, SPAN, CEN = _consts()
    n = [1, T - 1, T, T + 1, 2 * T + 3][which]
    spec, b = (n, 3, 3, 0.06, 20 + which), 0.3
    X, seeds, ref = _case(spec, b)
    model = _check_fit('test_point_counts_around_the_staged_tile', f'n={n}', X, seeds, ref, b)
    _check_predict(model, ref, 3, SPAN + 1, f'n={n}', seed=which)


@pytest.mark.parametrize('which', range(5))
def test_seed_counts_around_the_workgroup(which):
    T, G, SPAN, CEN = _consts()
    s = [1, G - 1, G, G + 1, 2 * G + 3][which]
    spec, b = (2 * T + 3, 7, 4, 0.07, 30), 0.3
    X, seeds, ref = _case(spec, b, n_seeds=s)
    assert seeds.shape == (s, 7)
    _check_fit('test_seed_counts_around_the_workgroup', f'S={s}', X, seeds, ref, b)


def test_seeds_without_neighbours_are_dropped_and_all_dropped_raises():
    from vqnerf_release_amd.decomp.nerfactor.util import meanshift
    T, G, SPAN, CEN = _consts()
    spec, b = (T + 41, 3, 4, 0.05, 40), 0.2
    X, seeds, ref = _case(spec, b, n_seeds=G + 9, seed_kind='cube')
    dropped = int((ref['counts'] == 0).sum())
    assert 0 < dropped < G + 9                                               # some seeds of the cube have no point within b, some do
    _check_fit('test_seeds_without_neighbours_are_dropped_and_all_dropped_raises', f'{dropped} of {G + 9} dropped', X, seeds, ref, b)
    X, seeds, ref = _case(spec, b, n_seeds=G + 9, seed_kind='far')
    assert isinstance(ref, ValueError)
    with launches() as rec, pytest.raises(ValueError, match='bandwidth'):
        meanshift.MeanShift(b, seeds=seeds.copy()).fit(X.copy())
    assert rec.counts == {'vqn_meanshift_seek': 1, 'vqn_meanshift_merge': 1}


@pytest.mark.parametrize('max_iter', [0, 1])
def test_max_iter_zero_and_one(max_iter):
    T, G, SPAN, CEN = _consts()
    spec, b = (T + 77, 8, 3, 0.1, 50), 0.4
    X, seeds, ref = _case(spec, b, max_iter=max_iter)
    assert ref['iters'].max() == max_iter and ref['n_iter'] == max_iter
    _check_fit('test_max_iter_zero_and_one', f'max_iter={max_iter}', X, seeds, ref, b, max_iter=max_iter)


def test_one_cluster_is_the_data_mean():
    T, G, SPAN, CEN = _consts()
    spec, b = (T + 9, 7, 5, 0.1, 60), 4.0
    X, seeds, ref = _case(spec, b)
    assert len(ref['centres']) == 1 and (ref['counts'] == T + 9).all()
    model = _check_fit('test_one_cluster_is_the_data_mean', 'K=1', X, seeds, ref, b)
    assert np.abs(model.cluster_centers_.cpu().numpy()[0] - X.mean(axis=0)).max() <= _bound(T + 9)


def test_cluster_all_false_labels_far_points_minus_one():
    T, G, SPAN, CEN = _consts()
    spec, b = (2 * T + 3, 3, 5, 0.05, 70), 0.15
    X, seeds, ref = _case(spec, b, cluster_all=False, n_seeds=3)             # three seeds: the blobs they do not reach are orphans
    far = int((ref['labels'] == -1).sum())
    assert 0 < far < 2 * T + 3 and np.abs(ref['dist'] - b).min() >= 1e-9      # no point lies on the bandwidth
    model = _check_fit('test_cluster_all_false_labels_far_points_minus_one', f'{far} orphans', X, seeds, ref, b, cluster_all=False)
    _check_predict(model, ref, 3, SPAN + 5, 'predict labels every point')
    assert int(model.predict(X.copy()).min()) >= 0


def test_uint8_features_are_read_as_k_over_255():
    T, G, SPAN, CEN = _consts()
    b = 0.3                                                                  # (76.5 bytes: no byte pair lies exactly on the bandwidth)
    bytes8 = np.rint(M.blobs(T + 130, 7, 4, 0.06, 80) * 255).astype(np.uint8)
    X = bytes8 / 255.
    ref = M.fit(X, b)
    model = _check_fit('test_uint8_features_are_read_as_k_over_255', 'uint8 device tensor', X, None, ref, b,
                       x_dev=torch.as_tensor(bytes8, device=_dev()))
    from vqnerf_release_amd.decomp.nerfactor.util import meanshift
    again = meanshift.MeanShift(b).fit(bytes8)                               # numpy bytes in
    assert torch.equal(again.cluster_centers_, model.cluster_centers_) and torch.equal(again.labels_, model.labels_)
    f32 = meanshift.MeanShift(b).fit(X.astype(np.float32))                   # float32 in: widened, not k / 255.
    ref32 = M.fit(X.astype(np.float32).astype(np.float64), b)
    assert f32.cluster_centers_.shape == ref32['centres'].shape
    assert np.abs(f32.cluster_centers_.cpu().numpy() - ref32['centres']).max() <= _bound(T + 130)


def test_assign_ties_go_to_the_lowest_index():
    from vqnerf_release_amd import _C
    T, G, SPAN, CEN = _consts()
    centres = np.array([[0.5, 0.5], [0.25, 0.5], [0.5, 0.5], [0.75, 0.5], [0.25, 0.5]])          # two exact duplicates
    pts = np.array([[0.375, 0.5], [0.625, 0.5], [0.5, 0.5], [0.25, 0.5], [0.75, 0.25], [0.0, 0.5]])
    want, wdist, gap = M.assign(pts, centres, b=0.2)
    assert gap == 0.0 and want.tolist() == [0, 0, 0, 1, -1, -1]              # 0.375: as far from 0.5 as from 0.25, exactly
    pts_n = np.tile(pts, (SPAN // 6 + 2, 1))[:SPAN + 3]                      # a second workgroup, ragged
    with launches() as rec:
        lab, dist = _C.meanshift_assign(torch.as_tensor(pts_n, device=_dev()), torch.as_tensor(centres, device=_dev()), 0.2, want_dist=True)
    assert rec.counts == {'vqn_meanshift_assign': 1}
    want_n, wdist_n, _ = M.assign(pts_n, centres, b=0.2)
    np.testing.assert_array_equal(lab.cpu().numpy(), want_n)
    assert (np.abs(dist.cpu().numpy() - wdist_n) <= np.spacing(wdist_n)).all()          # the same d2; a square root within an ulp
    every = _C.meanshift_assign(torch.as_tensor(pts_n, device=_dev()), torch.as_tensor(centres, device=_dev()))[0]
    np.testing.assert_array_equal(every.cpu().numpy(), M.assign(pts_n, centres)[0])


def test_assign_with_more_centres_than_stay_resident_and_more_points_than_one_pass():
    from vqnerf_release_amd import _C
    T, G, SPAN, CEN = _consts()
    rng = np.random.default_rng(90)
    for K, n, D in ((CEN, 2 * SPAN + 5, 8), (CEN + 1, 2 * SPAN + 5, 8), (2 * CEN + 3, SPAN - 1, 5), (3, 4096 * SPAN + 300, 2)):
        centres, pts = rng.random((K, D)), rng.random((n, D))
        want, wdist, gap = M.assign(pts, centres)
        assert gap > 0.0                                                     # the same d2 on both sides: any gap decides alike
        lab, dist = _C.meanshift_assign(torch.as_tensor(pts, device=_dev()), torch.as_tensor(centres, device=_dev()), want_dist=True)
        np.testing.assert_array_equal(lab.cpu().numpy(), want, err_msg=f'K={K} n={n}')
        assert (np.abs(dist.cpu().numpy() - wdist) <= np.spacing(wdist)).all(), f'K={K} n={n}'


def test_merge_walks_sorted_candidates_like_the_statement():
    from vqnerf_release_amd import _C
    rng = np.random.default_rng(91)
    M_, D, b = 2 * 1024 + 77, 3, 0.11                                        # three blocks of the search for the first undecided one
    cand = rng.random((M_, D))
    counts = np.sort(rng.integers(0, 6, M_))[::-1].astype(np.int32).copy()   # descending; the last ones 0: dropped
    assert (counts == 0).sum() > 100
    alive, keep = counts > 0, []
    margin = np.inf
    for i in range(M_):
        if alive[i]:
            keep.append(i)
            d2 = M.dist2(cand[i + 1:], cand[i])
            margin = min(margin, float(np.abs(d2 - b * b).min())) if i + 1 < M_ else margin
            alive[i + 1:] &= ~(d2 <= b * b)
    assert margin > 0.0 and 50 < len(keep) < M_                              # the same d2 on both sides
    with launches() as rec:
        kept, n_kept = _C.meanshift_merge(torch.as_tensor(cand, device=_dev()), torch.as_tensor(counts, device=_dev()), b)
    assert rec.counts == {'vqn_meanshift_merge': 1}
    assert int(n_kept) == len(keep) and np.flatnonzero(kept.cpu().numpy()).tolist() == keep


def test_bad_shapes_are_refused_with_the_reason():
    from vqnerf_release_amd import _C
    x = torch.zeros((10, 9), dtype=torch.float64, device=_dev())
    with pytest.raises(_C.VqnError, match='D = 9'):
        _C.meanshift_seek(x, x, 0.2, 300)
    with pytest.raises(_C.VqnError, match='D = 9'):
        _C.meanshift_assign(x, x)
    with pytest.raises(_C.VqnError, match='float64'):
        _C.meanshift_seek(x[:, :3].float().contiguous(), x[:, :3].contiguous(), 0.2, 300)
    ok = x[:, :3].contiguous()
    with pytest.raises(_C.VqnError, match='bandwidth'):
        _C.meanshift_seek(ok, ok, 0.0, 300)
    assert _C.lib().vqn_meanshift_merge_scratch_bytes(100, 9) == 0 and _C.lib().vqn_meanshift_merge_scratch_bytes(100, 8) == 128


def _write_scene(root, rng):
    """2 training and 2 validation views of 24 x 24: three flat materials plus noise of a few bytes, partial alpha, idx.png"""
    from PIL import Image
    H = W = 24
    mats = np.array([[200, 40, 40, 30, 30, 30, 220], [40, 190, 60, 120, 120, 120, 60], [50, 60, 210, 220, 200, 40, 140]], np.int64)
    pred, data, labels = root / 'pred', root / 'data', root / 'labels'
    truth = {}
    for view in ('train_000', 'train_001', 'val_000', 'val_007'):
        for d in (pred / view, data / view) + ((labels / view,) if view.startswith('val') else ()):
            os.makedirs(d)
        yy, xx = np.mgrid[0:H, 0:W]
        which = ((yy // 7 + xx // 9 + int(view[-1])) % 3)
        z = np.clip(mats[which] + rng.integers(-6, 7, (H, W, 7)), 0, 255).astype(np.uint8)
        alpha = np.where(rng.random((H, W)) < 0.7, 255, np.where(rng.random((H, W)) < 0.5, 0, 100)).astype(np.uint8)
        alpha[0, :3] = [0, 1, 255]
        Image.fromarray(z[..., 0:3]).save(pred / view / 'albedo.png')
        Image.fromarray(z[..., 3:6]).save(pred / view / 'spec.png')
        Image.fromarray(z[..., 6]).save(pred / view / 'rough.png')
        Image.fromarray(np.dstack([rng.integers(0, 256, (H, W, 3)).astype(np.uint8), alpha])).save(data / view / 'rgba.png')
        if view.startswith('val'):
            Image.fromarray(S.GT_PALETTE[which]).save(labels / view / 'idx.png')
        truth[view] = (z, alpha > 0, which)
    return pred, data, labels, truth


def test_scene_driver_writes_the_baseline_and_the_evaluator_scores_it(tmp_path):
    pytest.importorskip('PIL.Image')
    from PIL import Image
    from vqnerf_release_amd.decomp import cluster_eval, meanshift as driver
    pred, data, labels, truth = _write_scene(tmp_path, np.random.default_rng(5))
    dst, b = tmp_path / 'out' / 'scene', 0.3
    with launches() as rec:
        res = driver.run(str(pred), str(data), str(dst), b, n_samples=300, seed=3)
    assert rec.counts == {'vqn_meanshift_seek': 1, 'vqn_meanshift_merge': 1, 'vqn_meanshift_assign': 3}      # the fit's labels, two views
    assert res['views'] == ['batch000000000', 'batch000000007'] and res['n_fit'] == 300
    sample = res['sample'].cpu().numpy()
    assert sample.shape == (300, 7) and sample.dtype == np.uint8
    train = np.concatenate([truth[v][0][truth[v][1]] for v in ('train_000', 'train_001')])
    assert len(train) > 300 and {tuple(r) for r in sample.tolist()} <= {tuple(r) for r in train.tolist()}     # masked training pixels only
    ref = M.fit(sample / 255., b)
    _assert_margins(ref, 'driver')
    assert len(ref['centres']) == 3
    centres = np.load(dst / 'center.npy')
    assert centres.dtype == np.float64 and centres.shape == (3, 7) and np.abs(centres - ref['centres']).max() <= _bound(300)
    np.testing.assert_array_equal(centres, res['centers'])
    colours = np.concatenate([np.zeros((1, 3), np.uint8), S.PD_PALETTE])
    for view, out in (('val_000', 'batch000000000'), ('val_007', 'batch000000007')):
        z, mask, which = truth[view]
        want = np.zeros(mask.shape, np.uint8)
        lab, _, gap = M.assign(z[mask] / 255., ref['centres'])
        assert gap >= 1e-9
        want[mask] = lab + 1
        got = np.load(dst / out / 'labels.npy')
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)
        png = np.asarray(Image.open(dst / out / 'labels.png'))
        np.testing.assert_array_equal(png, colours[want])                    # read back through the palette: labels.npy
        assert [len(np.unique(got[mask & (which == m)])) for m in range(3)] == [1, 1, 1] and len(np.unique(got[mask])) == 3
    score = cluster_eval.evaluate(str(dst), str(labels), str(data), pred_file='labels.png', alpha_thres=0.0)      # pairs batch...NNN with val_NNN
    assert score['views'] == ['batch000000000', 'batch000000007'] and score['purity'] == 1.0 and score['f1-macro'] == 1.0
    assert score['total'] == int(truth['val_000'][1].sum() + truth['val_007'][1].sum())
    everything = driver.run(str(pred), str(data), str(dst), b, n_samples=None)
    assert everything['n_fit'] == len(train) and everything['centers'].shape == (3, 7)
    Image.fromarray(np.zeros((24, 25), np.uint8)).save(pred / 'val_007' / 'rough.png')
    with pytest.raises(ValueError, match='sizes differ'):
        driver.run(str(pred), str(data), str(dst), b)


def test_scene_driver_refuses_more_clusters_than_the_palette_has(tmp_path):
    pytest.importorskip('PIL.Image')
    from PIL import Image
    from vqnerf_release_amd.decomp import meanshift as driver
    H, W = 4, 22                                                             # 22 materials, 40 bytes apart in the first channel alone
    z = np.zeros((H, W, 7), np.uint8)
    z[..., 0] = (np.arange(W) % 7) * 40
    z[..., 3] = (np.arange(W) // 7) * 80

    def write():
        for view in ('train_000', 'val_000'):
            os.makedirs(tmp_path / 'pred' / view, exist_ok=True), os.makedirs(tmp_path / 'data' / view, exist_ok=True)
            Image.fromarray(z[..., 0:3]).save(tmp_path / 'pred' / view / 'albedo.png')
            Image.fromarray(z[..., 3:6]).save(tmp_path / 'pred' / view / 'spec.png')
            Image.fromarray(z[..., 6]).save(tmp_path / 'pred' / view / 'rough.png')
            Image.fromarray(np.full((H, W, 4), 255, np.uint8)).save(tmp_path / 'data' / view / 'rgba.png')

    write()
    with pytest.raises(ValueError, match='22 clusters'):
        driver.run(str(tmp_path / 'pred'), str(tmp_path / 'data'), str(tmp_path / 'out'), 0.1)
    assert not os.path.exists(tmp_path / 'out' / 'center.npy')
    z[:, 21] = z[:, 20]                                                      # 21 fit
    write()
    res = driver.run(str(tmp_path / 'pred'), str(tmp_path / 'data'), str(tmp_path / 'out'), 0.1)
    assert res['centers'].shape == (21, 7) and np.load(tmp_path / 'out' / 'batch000000000' / 'labels.npy').max() == 21
