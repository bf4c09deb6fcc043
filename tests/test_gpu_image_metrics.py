"""GPU: the image metrics of csrc/image_metrics.hip (decomp/nerfactor/util/metric.py, the writer's `metrics=True`, decomp/metric_eval.py)
against their float64 statement tests/image_metrics_model.py.

Integer sums, counts, MSE and PSNR must equal the statement bit for bit; SSIM, luma SSIM and luma PSNR are held to twice the largest
error observed over all shapes below on an MI355X (profiles/observed_errors_image_metrics.json; the project's convention), and the
SSIM bound may never exceed 5e-5: published scores carry four decimals.  Observed: SSIM 1.8e-15, luma SSIM 2.8e-15, luma PSNR
3.6e-15 dB (float64 accumulation on the device; what is left is the order of the sums)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import image_metrics_model as M
from tests.gpu_util import launches, record_observed

pytestmark = pytest.mark.gpu

SSIM_BOUND = 5.6e-15          # 2 x 2.8e-15, the larger of the two SSIM forms' observed errors; the cap is 5e-5
PSNR_LUMA_BOUND = 7.2e-15     # 2 x 3.6e-15 dB
assert SSIM_BOUND <= 5e-5

TILE_IN = 42                  # one 32-position tile plus its 10-pixel halo
# (H, W, C, B): the smallest images; one pixel less than / equal to / more than a tile plus halo, per dimension; several tiles both ways
CASES = [(11, 11, 3, 1), (11, 12, 1, 3), (12, 11, 3, 3), (12, 12, 1, 1), (TILE_IN - 1, 20, 3, 1), (TILE_IN, 20, 3, 3), (TILE_IN + 1, 20, 1, 1),
         (20, TILE_IN - 1, 1, 3), (20, TILE_IN, 3, 1), (20, TILE_IN + 1, 3, 1), (TILE_IN + 1, TILE_IN + 1, 3, 1), (43, 75, 3, 17), (43, 75, 1, 3)]


def _dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _images(B, H, W, C, seed=0):
    """float32 pairs [B,H,W,C] in about [-0.15, 1.15]: a diagonal ramp that saturates at both ends, a flat block, noise on the rest"""
    rng = np.random.default_rng(1000 * seed + 7 * H + 13 * W + C + 31 * B)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = ((xx + yy) / float(H + W - 2) * 1.3 - 0.15)[None, :, :, None]
    tex = ((xx * 3 > W) | (yy * 3 > H))[None, :, :, None]                   # the top-left ninth stays smooth
    a = ramp + np.where(tex, rng.normal(0.0, 0.12, (B, H, W, C)), 0.0)
    a[:, H // 2:H // 2 + 6, :W // 2] = 0.6                                   # flat
    b = a + np.where(tex, rng.normal(0.0, 0.05, (B, H, W, C)), 0.0) + np.where(yy > H // 2, 0.02, 0.0)[None, :, :, None]
    a, b = a.astype(np.float32), b.astype(np.float32)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _reference(B, H, W, C):
    a, b = _images(B, H, W, C)
    a8, b8 = M.to_uint8(a), M.to_uint8(b)
    assert (a8 == 0).any() and (a8 == 255).any() and (a8[:, H // 2, :W // 2] == a8[:, H // 2, :1]).all()
    return a8, b8, [M.metrics(a8[i], b8[i]) for i in range(B)]


def _check_rows(raw, refs, test, case):
    """raw: the library's rows (int64 [B,16], host) against the statement's dicts; returns the largest errors"""
    f = raw.view(np.float64)
    worst = {'ssim': 0.0, 'ssim_luma': 0.0, 'psnr_luma': 0.0}
    for i, m in enumerate(refs):
        C = len(m['sse'])
        assert list(raw[i, 10:10 + C]) == m['sse'] and (raw[i, 10 + C:13] == 0).all(), (case, i)
        assert raw[i, 13] == m['n_pixels'] and raw[i, 14] == m['n_positions'], (case, i)
        assert f[i, 1] == m['mse'] and f[i, 0] == m['psnr'], (case, i, f[i, :2], m['mse'], m['psnr'])
        for k, col in (('ssim', 3), ('ssim_luma', 4), ('psnr_luma', 2)):
            worst[k] = max(worst[k], 0.0 if f[i, col] == m[k] else abs(f[i, col] - m[k]))
    for k, bound in (('ssim', SSIM_BOUND), ('ssim_luma', SSIM_BOUND), ('psnr_luma', PSNR_LUMA_BOUND)):
        record_observed(test, f'{case} {k}', worst[k], bound)
    for k, bound in (('ssim', SSIM_BOUND), ('ssim_luma', SSIM_BOUND), ('psnr_luma', PSNR_LUMA_BOUND)):
        assert worst[k] <= bound, (case, k, worst[k], bound)


@pytest.mark.parametrize('H,W,C,B', CASES)
def test_u8_form_matches_the_statement(H, W, C, B):
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    a8, b8, refs = _reference(B, H, W, C)
    with launches() as rec:
        raw = metric.image_metrics_raw(torch.as_tensor(a8, device=_dev()), torch.as_tensor(b8, device=_dev()))
    assert rec.counts == {'vqn_image_metrics_u8': 1}                        # one entry per batch: its kernel and the finalize launch
    _check_rows(raw.cpu().numpy(), refs, 'test_u8_form_matches_the_statement', f'{H}x{W}x{C} B={B}')


@pytest.mark.parametrize('H,W,C,B', [(TILE_IN + 1, 20, 1, 1), (20, TILE_IN + 1, 3, 1), (43, 75, 3, 17)])
def test_f32_form_equals_u8_form_bit_for_bit(H, W, C, B):
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    a, b = (np.array(t) for t in _images(B, H, W, C))
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    special = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                              np.float32([0.0, 1.0, -0.0, -1e-7, -3.0, 1.0000001, 7.5, 0.999999, 1e-30])])
    n = min(special.size, a[0, ..., 0].size)
    a[0, :, :, 0].flat[:n] = special[:n]                                      # channel 0 of the first pair, row by row
    b[-1, :, :, C - 1].flat[:n] = special[:n][::-1]
    a8, b8 = M.to_uint8(a), M.to_uint8(b)
    with launches() as rec:
        got32 = metric.image_metrics_raw(torch.as_tensor(a, device=_dev()), torch.as_tensor(b, device=_dev()))
        got8 = metric.image_metrics_raw(torch.as_tensor(a8, device=_dev()), torch.as_tensor(b8, device=_dev()))
    assert rec.counts == {'vqn_image_metrics_f32': 1, 'vqn_image_metrics_u8': 1}
    assert torch.equal(got32, got8)
    m = M.metrics(a8[0], b8[0])
    assert list(got32[0, 10:10 + C].cpu().numpy()) == m['sse']


def test_special_values_quantise_as_the_writer_does():
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)), np.float32([0.0, 1.0, -0.5, 1.5])])
    H, W = 11, 71
    a = np.resize(vals, (1, H, W, 1)).astype(np.float32)
    b = np.zeros_like(a)
    raw = metric.image_metrics_raw(torch.as_tensor(a, device=_dev()), torch.as_tensor(b, device=_dev())).cpu().numpy()
    q = M.to_uint8(a).astype(np.int64)
    assert raw[0, 10] == int((q * q).sum())                                  # sse against black = sum of the squared bytes


@pytest.mark.parametrize('form', ['u8', 'f32'])
def test_standard_background_is_strict(form):
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    B, H, W, C = 3, 20, TILE_IN + 1, 3
    a, b = _images(B, H, W, C)
    rng = np.random.default_rng(5)
    thres = 0.95
    alpha = rng.choice(np.float32([0.0, 0.5, thres, np.nextafter(np.float32(thres), np.float32(2)), 0.97, 1.0]), (B, H, W)).astype(np.float32)
    assert (alpha == np.float32(thres)).sum() > 10
    ca = np.stack([M.standard_background(a[i] if form == 'f32' else M.to_uint8(a[i]), alpha[i], thres) for i in range(B)])
    cb = np.stack([M.standard_background(b[i] if form == 'f32' else M.to_uint8(b[i]), alpha[i], thres) for i in range(B)])
    src = (a, b) if form == 'f32' else (M.to_uint8(a), M.to_uint8(b))
    dev = _dev()
    got = metric.image_metrics_raw(torch.as_tensor(src[0], device=dev), torch.as_tensor(src[1], device=dev),
                                   alpha=torch.as_tensor(alpha, device=dev), alpha_thres=thres)
    want = metric.image_metrics_raw(torch.as_tensor(ca, device=dev), torch.as_tensor(cb, device=dev))
    assert torch.equal(got, want)
    _check_rows(got.cpu().numpy(), [M.metrics(ca[i], cb[i]) for i in range(B)], 'test_standard_background_is_strict', f'{form} {H}x{W}')
    shared = metric.image_metrics_raw(torch.as_tensor(src[0], device=dev), torch.as_tensor(src[1], device=dev),
                                      alpha=torch.as_tensor(alpha[0], device=dev), alpha_thres=thres)      # one plane for all pairs
    assert torch.equal(shared[0], got[0]) and not torch.equal(shared[1], got[1])
    u8 = metric.image_metrics_raw(torch.as_tensor(src[0][:1], device=dev), torch.as_tensor(src[1][:1], device=dev),
                                  alpha=torch.as_tensor((alpha[0] > 0.5).astype(np.uint8) * 255, device=dev), alpha_thres=0.5)
    only = np.where((alpha[0] > 0.5)[..., None], M.to_uint8(a[0]), np.uint8(255)), np.where((alpha[0] > 0.5)[..., None], M.to_uint8(b[0]), np.uint8(255))
    assert list(u8[0, 10:13].cpu().numpy()) == M.metrics(*only)['sse']


def test_two_calls_return_equal_bits():
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    a, b = _images(17, 43, 75, 3)
    ta, tb = torch.as_tensor(a, device=_dev()), torch.as_tensor(b, device=_dev())
    first = metric.image_metrics_raw(ta, tb).clone()
    assert torch.equal(first, metric.image_metrics_raw(ta, tb))
    one = metric.image_metrics_raw(ta[5:6].contiguous(), tb[5:6].contiguous())
    assert torch.equal(one[0], first[5])                                     # a pair's score does not depend on its batch


def test_small_images_raise_and_name_the_size():
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    z = torch.zeros((1, 10, 40, 3), dtype=torch.uint8, device=_dev())
    with pytest.raises(_C.VqnError, match='10x40'):
        metric.image_metrics(z, z)
    with pytest.raises(_C.VqnError, match='40x10'):
        metric.image_metrics(z.reshape(1, 40, 10, 3).float(), z.reshape(1, 40, 10, 3).float())
    with pytest.raises(_C.VqnError, match='channels'):
        _C.image_metrics(torch.zeros((1, 12, 12, 2), dtype=torch.uint8, device=_dev()), torch.zeros((1, 12, 12, 2), dtype=torch.uint8, device=_dev()),
                         metric.gaussian_window())
    with pytest.raises(ValueError):
        metric.image_metrics(z[..., :2], z[..., :2])
    with pytest.raises(NotImplementedError):
        metric.SSIM('uint8')(z[0], z[0], multiscale=True)


def test_class_forms_equal_image_metrics():
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    a8, b8, refs = _reference(1, 20, TILE_IN + 1, 3)
    res = {k: float(v[0]) for k, v in metric.image_metrics(torch.as_tensor(a8, device=_dev()), torch.as_tensor(b8, device=_dev())).items()}
    assert set(res) == {'psnr', 'mse', 'psnr_luma', 'ssim', 'ssim_luma'}
    for cls, key in ((metric.PSNR, 'psnr'), (metric.MSE, 'mse'), (metric.PSNR_luma, 'psnr_luma'), (metric.SSIM, 'ssim'), (metric.SSIM_luma, 'ssim_luma')):
        assert cls('uint8')(a8[0], b8[0]) == res[key]                        # numpy in, Python float out
        assert isinstance(cls('uint8')(torch.as_tensor(a8[0], device=_dev()), torch.as_tensor(b8[0], device=_dev())), float)
    assert res['psnr'] == refs[0]['psnr'] and res['mse'] == refs[0]['mse']
    assert metric.PSNR('uint8')(a8[0], a8[0]) == float('inf') and metric.SSIM('uint8')(a8[0], a8[0]) == 1.0
    np.testing.assert_array_equal(metric.gaussian_window(), M.window_1d())


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_writer_scores_the_written_images(tmp_path):
    pytest.importorskip('PIL.Image')
    from tests.test_vis_output import _Stub, _view
    from vqnerf_release_amd.decomp.nerfactor import train_nfr
    from vqnerf_release_amd.decomp.nerfactor.util import vis
    H, W = 24, 20
    view = {k: (v.to(_dev()) if torch.is_tensor(v) and k != 'hw' else v) for k, v in _view(H, W, seed=3).items()}
    out = tmp_path / 'vis_vali' / 'epoch000000001' / 'batch000000000'
    plain = tmp_path / 'plain' / 'batch000000000'
    with launches() as rec:
        vis.vis_batch(_Stub(), view, str(plain), mode='vali').flush()
    assert not rec.ran('vqn_image_metrics')
    with launches() as rec:
        vis.vis_batch(_Stub(), view, str(out), mode='vali', metrics=True).flush()
    assert rec.counts.get('vqn_image_metrics_f32') == 1
    meta, meta_plain = json.load(open(out / 'metadata.json')), json.load(open(plain / 'metadata.json'))
    g8, p8 = _png(out / 'gt_rgb.png'), _png(out / 'pred_rgb.png')
    assert meta_plain == {'id': 'val_007', 'psnr': vis.psnr_uint8(g8, p8)}     # the default: what it has always been
    for name in sorted(os.listdir(plain)):
        if name != 'metadata.json':
            assert open(plain / name, 'rb').read() == open(out / name, 'rb').read(), name
    assert set(meta) == {'id', 'psnr', 'mse', 'psnr_luma', 'ssim', 'ssim_luma'}
    m = M.metrics(g8, p8)
    assert meta['psnr'] == m['psnr'] and meta['mse'] == m['mse']
    assert abs(meta['psnr'] - meta_plain['psnr']) < 1e-9
    for k, bound in (('ssim', SSIM_BOUND), ('ssim_luma', SSIM_BOUND), ('psnr_luma', PSNR_LUMA_BOUND)):
        record_observed('test_writer_scores_the_written_images', f'{H}x{W} {k}', abs(meta[k] - m[k]), bound)
        assert abs(meta[k] - m[k]) <= bound, (k, meta[k], m[k])
    metas = train_nfr.save_metas(str(tmp_path))
    assert metas['ssim'] == [meta['ssim']] and metas['mse'] == [meta['mse']] and metas['lpips'] == [None]


def _write_scene(root, n_views=2, H=16, W=14, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    pred_root, gt_root = root / 'pred', root / 'gt'
    tree = {}
    for v in range(n_views):
        pd, gd = pred_root / f'batch{v:09d}', gt_root / f'val_{v:03d}'
        os.makedirs(pd), os.makedirs(gd)
        yy, xx = np.mgrid[0:H, 0:W]
        alpha = np.where((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < 30, 255, rng.integers(0, 256, (H, W))).astype(np.uint8)
        alpha[0, :4] = [242, 243, 0, 255]                                     # 242 / 255 < 0.95 < 243 / 255
        imgs = {}
        for name in ('rgb', 'albedo', 'city', 'forest'):
            gt = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
            pred = np.clip(gt.astype(np.int64) * (0.7 if name == 'albedo' else 1.0) + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
            imgs[name] = (gt, pred)
        Image.fromarray(np.dstack([imgs['rgb'][0], alpha])).save(gd / 'rgba.png')
        Image.fromarray(imgs['rgb'][1]).save(pd / 'pred_rgb.png')
        Image.fromarray(imgs['albedo'][0]).save(gd / 'albedo.png')
        Image.fromarray(imgs['albedo'][1]).save(pd / 'pred_albedo.png')
        for probe in ('city', 'forest'):
            Image.fromarray(imgs[probe][0]).save(gd / f'rgba_{probe}.png')
            Image.fromarray(imgs[probe][1]).save(pd / f'pred_rgb_probes_{probe}.png')
        Image.fromarray(imgs['rgb'][1]).save(pd / 'pred_rgb_probes_unpaired.png')     # no ground truth: not scored
        tree[v] = (alpha, imgs)
    return pred_root, gt_root, tree


def test_evaluator_matches_the_statement(tmp_path):
    pytest.importorskip('PIL.Image')
    from PIL import Image
    from vqnerf_release_amd.decomp import metric_eval
    pred_root, gt_root, tree = _write_scene(tmp_path)
    with launches() as rec:
        res = metric_eval.evaluate(str(pred_root), str(gt_root), alpha_thres=0.95)
    assert rec.counts == {'vqn_image_metrics_u8': 2}                          # one call per view for all its pairs
    assert json.load(open(pred_root / 'metrics.json')) == res
    assert res['views'] == ['batch000000000', 'batch000000001'] and set(res) == {'rgb', 'kd', 'env', 'views'}

    def want(v, name, pred=None):
        alpha, imgs = tree[v]
        a01 = alpha.astype(np.float32) / np.float32(255)
        gt, pd = imgs[name][0], (imgs[name][1] if pred is None else pred)
        return M.metrics(M.standard_background(gt, a01, 0.95), M.standard_background(pd, a01, 0.95))

    def check(got, names_per_view, preds=None):
        ms = [want(v, n, None if preds is None else preds[v]) for v in sorted(tree) for n in names_per_view]
        assert got['psnr'] == [m['psnr'] for m in ms]
        worst = max(abs(g - m['ssim']) for g, m in zip(got['ssim'], ms))
        record_observed('test_evaluator_matches_the_statement', f'16x14 {"+".join(names_per_view)} ssim', worst, SSIM_BOUND)
        assert worst <= SSIM_BOUND
        assert got['psnr_mean'] == float(np.mean(got['psnr'])) and got['ssim_mean'] == float(np.mean(got['ssim']))

    check(res['rgb'], ['rgb'])
    check(res['kd'], ['albedo'])
    check(res['env'], ['city', 'forest'])
    assert M.standard_background(tree[0][1]['rgb'][0], tree[0][0].astype(np.float32) / np.float32(255), 0.95)[0, 0].tolist() == [255] * 3

    # use_scale: mean over views of sum(gt * alpha) / sum(pred * alpha) per channel; the scaled albedo is quantised as every image is
    scaled = metric_eval.evaluate(str(pred_root), str(gt_root), alpha_thres=0.95, use_scale=True)
    ratios = []
    for v in sorted(tree):
        alpha, imgs = tree[v]
        a = alpha.astype(np.float64)[..., None] / 255.0
        gt, pd = imgs['albedo'][0].astype(np.float64) / 255.0, imgs['albedo'][1].astype(np.float64) / 255.0
        ratios.append((gt * a).sum((0, 1)) / (pd * a).sum((0, 1)))
    np.testing.assert_allclose(scaled['kd_scale'], np.mean(ratios, 0), rtol=1e-12)
    assert all(1.2 < s < 1.7 for s in scaled['kd_scale'])
    s = np.asarray(scaled['kd_scale'])
    preds = {v: M.to_uint8((tree[v][1]['albedo'][1].astype(np.float64) / 255.0 * s).astype(np.float32)) for v in tree}
    check(scaled['kd'], ['albedo'], preds)
    assert scaled['rgb'] == res['rgb'] and scaled['kd']['psnr_mean'] > res['kd']['psnr_mean']

    Image.fromarray(np.zeros((16, 15, 3), np.uint8)).save(pred_root / 'batch000000001' / 'pred_albedo.png')
    with pytest.raises(ValueError, match='sizes differ'):
        metric_eval.evaluate(str(pred_root), str(gt_root))
