"""Float64 statement of the image metrics of csrc/image_metrics.hip, written from the definition (numpy only).

SSIM is `tf.image.ssim` with its defaults: an 11x11 Gaussian window, sigma 1.5, normalised to sum 1; 'VALID' convolution, so
(H - 10)(W - 10) positions; c1 = (0.01 * 255)^2, c2 = (0.03 * 255)^2 on 8-bit data;
    luminance = (2 mx my + c1) / (mx^2 + my^2 + c1),   cs = (2 conv(xy) - 2 mx my + c2) / (conv(x^2 + y^2) - mx^2 - my^2 + c2),
each channel's score the mean of luminance * cs over the positions, the image's score the mean over channels.
MSE is the mean squared 8-bit difference over all pixels and channels, PSNR = 10 log10(255^2 / MSE), inf for MSE = 0.  The luma
forms score the one plane 0.2126 R + 0.7152 G + 0.0722 B (unrounded, float64); for one-channel images luma is the channel.

log10 here is `log10_det`: a fixed sequence of IEEE double operations (frexp, one division, an odd series of atanh), the same
one the library's finalize launch runs, so PSNR agrees with the device bit for bit.  It is within 2 ulp of libm's log10."""
import math

import numpy as np

WIN, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
LUMA = (0.2126, 0.7152, 0.0722)
_LOG10_2 = float.fromhex('0x1.34413509f79ffp-2')
_INV_LN10 = float.fromhex('0x1.bcb7b1526e50ep-2')
_SQRT_HALF = float.fromhex('0x1.6a09e667f3bcdp-1')
_SERIES = 13                                             # terms s^(2k+1) / (2k+1), k = 0 .. 12: |s| <= 0.1716, the rest < 1e-20


def window_1d():
    x = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def window_2d():
    """the window as tf.image.ssim builds it: softmax over the 121 values of -(dx^2 + dy^2) / (2 sigma^2)"""
    x = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2.0
    g = (x * x) * (-0.5 / (SIGMA * SIGMA))
    g = np.exp(g[None, :] + g[:, None])
    return g / g.sum()


def log10_det(r):
    """log10 of a positive float in a fixed order of IEEE operations (no fused multiply-add)"""
    m, e = math.frexp(r)
    if m < _SQRT_HALF:
        m, e = m * 2.0, e - 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    q = 1.0 / (2 * _SERIES - 1)
    for k in range(_SERIES - 2, -1, -1):
        q = q * z + 1.0 / (2 * k + 1)
    ln_m = (2.0 * s) * q
    return float(e) * _LOG10_2 + ln_m * _INV_LN10


def psnr_of_mse(mse):
    return float('inf') if mse == 0 else 10.0 * log10_det((255.0 * 255.0) / mse)


def to_uint8(x):
    """float rows in [0, 1] -> bytes, as the writer does: clip, * 255 in f32, truncate"""
    return (np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint8)


def standard_background(img, alpha, thres):
    """white wherever not alpha > thres (strict); img uint8 [H,W,C] or float [H,W,C], alpha [H,W]"""
    keep = (np.asarray(alpha) > np.float32(thres))[..., None]
    if img.dtype == np.uint8:
        return np.where(keep, img, np.uint8(255))
    return to_uint8(np.where(keep, img, np.float32(1.0)))


def luma(img):
    """[H,W,C] uint8 -> [H,W] float64"""
    f = img.astype(np.float64)
    if f.shape[2] == 1:
        return f[..., 0]
    return LUMA[0] * f[..., 0] + LUMA[1] * f[..., 1] + LUMA[2] * f[..., 2]


def _filter(p, w):
    H, W = p.shape
    h = sum(w[k] * p[:, k:k + W - WIN + 1] for k in range(WIN))
    return sum(w[k] * h[k:k + H - WIN + 1, :] for k in range(WIN))


def ssim_plane_sum(x, y):
    """sum of luminance * cs over the valid positions of two float64 planes"""
    if x.shape[0] < WIN or x.shape[1] < WIN:
        raise ValueError(f'image {x.shape[0]}x{x.shape[1]} is smaller than the {WIN}x{WIN} window')
    w = window_1d()
    mx, my = _filter(x, w), _filter(y, w)
    sxy, sxx = _filter(x * y, w), _filter(x * x + y * y, w)
    lum = (2.0 * mx * my + C1) / (mx * mx + my * my + C1)
    cs = (2.0 * sxy - 2.0 * mx * my + C2) / (sxx - mx * mx - my * my + C2)
    return float(np.sum(lum * cs))


def ssim_plane_direct(x, y):
    """the same mean with the 2-D window applied position by position (small images: the check of the separable form)"""
    w2 = window_2d()
    H, W = x.shape
    tot = 0.0
    for i in range(H - WIN + 1):
        for j in range(W - WIN + 1):
            a, b = x[i:i + WIN, j:j + WIN], y[i:i + WIN, j:j + WIN]
            mx, my = np.sum(w2 * a), np.sum(w2 * b)
            sxy, sxx = np.sum(w2 * a * b), np.sum(w2 * (a * a + b * b))
            tot += (2 * mx * my + C1) / (mx * mx + my * my + C1) * (2 * sxy - 2 * mx * my + C2) / (sxx - mx * mx - my * my + C2)
    return tot / ((H - WIN + 1) * (W - WIN + 1))


def n_positions(H, W):
    return (H - WIN + 1) * (W - WIN + 1)


def metrics(a, b):
    """a, b uint8 [H,W,C], C in {1, 3} -> dict of floats (psnr, mse, psnr_luma, ssim, ssim_luma) and the integer sums
    (sse per channel, n_pixels, n_positions)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 3 and a.shape[2] in (1, 3)
    H, W, C = a.shape
    d = a.astype(np.int64) - b.astype(np.int64)
    sse = [int(np.sum(d[..., c] * d[..., c])) for c in range(C)]
    mse = float(sum(sse)) / float(H * W * C)
    la, lb = luma(a), luma(b)
    mse_l = float(np.sum((la - lb) ** 2)) / float(H * W)
    n = n_positions(H, W)
    per_ch = [ssim_plane_sum(a[..., c].astype(np.float64), b[..., c].astype(np.float64)) / float(n) for c in range(C)]
    ssim = per_ch[0] if C == 1 else ((per_ch[0] + per_ch[1]) + per_ch[2]) / 3.0
    ssim_l = per_ch[0] if C == 1 else ssim_plane_sum(la, lb) / float(n)
    return dict(psnr=psnr_of_mse(mse), mse=mse, psnr_luma=psnr_of_mse(mse_l), ssim=ssim, ssim_luma=ssim_l,
                sse=sse, n_pixels=H * W, n_positions=n)
