"""CPU: tests/image_metrics_model.py, the float64 statement the device image metrics are held to, pinned by known answers.

TensorFlow is not available to this suite, so parity with `tf.image.ssim` itself is NOT pinned here: what is pinned is the
definition as its documentation and source state it (window, 'VALID' positions, constants, the two quotients, the two means)."""
import math

import numpy as np
import pytest

from tests import image_metrics_model as M


def _noise(H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)


def test_window_is_the_outer_product_and_sums_to_one():
    w1, w2 = M.window_1d(), M.window_2d()
    assert w1.shape == (11,) and w2.shape == (11, 11)
    assert abs(w1.sum() - 1.0) < 1e-15 and abs(w2.sum() - 1.0) < 1e-15
    np.testing.assert_allclose(w2, np.outer(w1, w1), rtol=1e-13, atol=0)
    np.testing.assert_array_equal(w1, w1[::-1])
    assert abs(w1[5] / w1[4] - math.exp(1.0 / (2 * 1.5 * 1.5))) < 1e-14


def test_identical_images_score_one_and_inf():
    a = _noise(19, 23, 3, 0)
    m = M.metrics(a, a.copy())
    assert m['ssim'] == 1.0 and m['ssim_luma'] == 1.0
    assert m['psnr'] == float('inf') and m['psnr_luma'] == float('inf') and m['mse'] == 0.0 and m['sse'] == [0, 0, 0]


@pytest.mark.parametrize('a,b', [(10, 200), (255, 254), (0, 255), (128, 131)])
def test_constant_images_have_the_closed_form(a, b):
    x, y = np.full((14, 17, 3), a, np.uint8), np.full((14, 17, 3), b, np.uint8)
    m = M.metrics(x, y)
    want = (2.0 * a * b + M.C1) / (a * a + b * b + M.C1)                 # the variances vanish: cs = c2 / c2
    assert abs(m['ssim'] - want) < 1e-12 and abs(m['ssim_luma'] - want) < 1e-12
    assert m['mse'] == float((a - b) ** 2)
    assert abs(m['psnr'] - 10.0 * math.log10(255.0 ** 2 / (a - b) ** 2)) < 1e-12
    assert abs(m['psnr_luma'] - m['psnr']) < 1e-9                        # the luma weights sum to 1


def test_an_11x11_image_has_one_position():
    a, b = _noise(11, 11, 3, 1), _noise(11, 11, 3, 2)
    m = M.metrics(a, b)
    assert m['n_positions'] == 1 and M.n_positions(11, 12) == 2 and M.n_positions(43, 75) == 33 * 65
    w2 = M.window_2d()
    x, y = a[..., 1].astype(np.float64), b[..., 1].astype(np.float64)
    mx, my = np.sum(w2 * x), np.sum(w2 * y)
    want = (2 * mx * my + M.C1) / (mx * mx + my * my + M.C1) * (2 * np.sum(w2 * x * y) - 2 * mx * my + M.C2) / (
        np.sum(w2 * (x * x + y * y)) - mx * mx - my * my + M.C2)
    assert abs(M.ssim_plane_sum(x, y) - want) < 1e-12
    with pytest.raises(ValueError, match='10x40'):
        M.ssim_plane_sum(np.zeros((10, 40)), np.zeros((10, 40)))


def test_separable_form_equals_the_2d_window():
    a, b = _noise(15, 18, 3, 3), _noise(15, 18, 3, 4)
    b[:, :9] = a[:, :9]                                                  # half equal, half unrelated
    for c in range(3):
        x, y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        assert abs(M.ssim_plane_sum(x, y) / M.n_positions(15, 18) - M.ssim_plane_direct(x, y)) < 1e-12
    m = M.metrics(a, b)
    assert 0.0 < m['ssim'] < 1.0 and -1.0 < m['ssim_luma'] < 1.0


def test_luma_of_white_is_255_and_one_channel_luma_is_the_channel():
    assert abs(M.luma(np.full((1, 1, 3), 255, np.uint8))[0, 0] - 255.0) < 1e-12
    assert abs(sum(M.LUMA) - 1.0) < 1e-15
    a, b = _noise(12, 13, 1, 5), _noise(12, 13, 1, 6)
    m = M.metrics(a, b)
    assert m['ssim_luma'] == m['ssim'] and m['psnr_luma'] == m['psnr']
    np.testing.assert_array_equal(M.luma(a), a[..., 0].astype(np.float64))


def test_mse_and_psnr_come_from_the_integer_sum():
    a, b = _noise(13, 11, 3, 7), _noise(13, 11, 3, 8)
    m = M.metrics(a, b)
    d = a.astype(np.int64) - b.astype(np.int64)
    assert sum(m['sse']) == int((d * d).sum()) and m['n_pixels'] == 143
    assert m['mse'] == float(int((d * d).sum())) / float(143 * 3)
    assert abs(m['psnr'] - 10 * math.log10(255.0 ** 2 / m['mse'])) < 1e-12


def test_log10_det_is_within_two_ulp_of_libm():
    rng = np.random.default_rng(9)
    values = list(np.exp(rng.uniform(-30, 30, 2000))) + [1.0, 10.0, 100.0, 65025.0, 0.5, 2.0, 1e-300, 1e300, 0.7071067811865476]
    for r in values:
        got, want = M.log10_det(float(r)), math.log10(float(r))
        assert abs(got - want) <= 2 * math.ulp(want) + 1e-17, (r, got, want)
    assert M.log10_det(1.0) == 0.0


def test_to_uint8_and_the_standard_background():
    x = np.array([[-0.5, 0.0, 0.5, 1.0, 1.5, 254.999 / 255.0]], np.float32)
    np.testing.assert_array_equal(M.to_uint8(x), [[0, 0, 127, 255, 255, 254]])
    img = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    alpha = np.array([[0.95, 0.951], [1.0, 0.0]], np.float32)
    out = M.standard_background(img, alpha, 0.95)
    np.testing.assert_array_equal(out[0, 0], [255, 255, 255])            # strict: alpha == thres is background
    np.testing.assert_array_equal(out[0, 1], img[0, 1])
    np.testing.assert_array_equal(out[1, 0], img[1, 0])
    np.testing.assert_array_equal(out[1, 1], [255, 255, 255])
    np.testing.assert_array_equal(M.standard_background(img.astype(np.float32) / 255, alpha, 0.95)[0, 0], [255, 255, 255])
