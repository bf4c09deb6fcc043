"""Image metrics on the device: the seam of `xiuminglib/metric.py` (third party of the reference; `xm.metric.PSNR('uint8')` and
friends in decomp/nerfvq_nfr3/metric_eval.py and nerfactor/models/*.py).

`image_metrics` scores a batch of image pairs in two launches of csrc/image_metrics.hip and leaves the results on the device;
the classes `PSNR`, `PSNR_luma`, `SSIM`, `SSIM_luma`, `MSE` have the constructor and call shapes of the originals and return a
Python float.  Definitions (tests/image_metrics_model.py is their float64 statement):
  * MSE: mean squared 8-bit difference over pixels and channels (the originals' `drange` is 255 for uint8);
    PSNR = 10 log10(255^2 / MSE), inf when the images are equal; taken in float64 from the exact integer sum;
  * SSIM: `tf.image.ssim(im1, im2, max_val=255)` with its defaults -- 11x11 Gaussian window, sigma 1.5, 'VALID' positions,
    k1 = 0.01, k2 = 0.03 -- mean over positions, then over channels;
  * the luma forms score 0.2126 R + 0.7152 G + 0.0722 B (`xiuminglib/img.py: rgb2lum`), unrounded.
Float32 inputs are rows in [0, 1] as `fast_render` leaves them; the kernel quantises them as the writer's `to_uint8` does, so a
score is that of the PNG that would be written.

Out of scope: multi-scale SSIM (`multiscale=True` raises NotImplementedError), the originals' `mask=` of contributing pixels
(raises too: the evaluator composites over the standard background instead, `alpha=` here) and LPIPS, whose network weights are not part of
this package; `train_nfr.save_metas` keeps reporting None for `lpips`.  There is no CPU path: numpy inputs are uploaded."""
import numpy as np
import torch

from vqnerf_release_amd import _C

WINDOW_SIZE, WINDOW_SIGMA = _C.IMAGE_METRICS_WINDOW, 1.5
KEYS = ('psnr', 'mse', 'psnr_luma', 'ssim', 'ssim_luma')         # words 0..4 of the library's output row


def gaussian_window():
    """the normalised 1-D window (float64); tf.image.ssim's 2-D window is its outer product"""
    x = np.arange(WINDOW_SIZE, dtype=np.float64) - (WINDOW_SIZE - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * WINDOW_SIGMA * WINDOW_SIGMA))
    return g / g.sum()


_WINDOW = gaussian_window()


def _device_batch(im, device):
    t = torch.as_tensor(im)
    if t.dim() == 2:
        t = t[..., None]
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[-1] not in (1, 3):
        raise ValueError(f'expected images [H, W], [H, W, C] or [B, H, W, C] with C in (1, 3), got shape {tuple(t.shape)}')
    if t.is_floating_point():
        t = t.to(torch.float32)
    return t.to(device).contiguous()


def image_metrics_raw(a, b, alpha=None, alpha_thres=None):
    """-> the library's output rows, int64 [B, 16] (include/vqn_eval.h: scores, sums, integer sums and counts)"""
    dev = next((t.device for t in (a, b) if torch.is_tensor(t) and t.is_cuda), torch.device('cuda'))
    a, b = _device_batch(a, dev), _device_batch(b, dev)
    if (alpha is None) != (alpha_thres is None):
        raise ValueError('alpha and alpha_thres come together')
    if alpha is not None:
        alpha = torch.as_tensor(alpha).to(dev)
        if alpha.dtype == torch.uint8:
            alpha = alpha.to(torch.float32) / 255.0
        alpha = alpha.to(torch.float32).contiguous()
        if alpha.dim() == 4 and alpha.shape[-1] == 1:
            alpha = alpha[..., 0].contiguous()
        if alpha.dim() == 3 and a.shape[0] == 1 and alpha.shape[0] == 1:
            alpha = alpha[0]
    return _C.image_metrics(a, b, _WINDOW, alpha, 0.0 if alpha_thres is None else alpha_thres)


def image_metrics(a, b, alpha=None, alpha_thres=None):
    """Scores of the pairs (a[i], b[i]): a, b [B, H, W, C] (or one image [H, W, C] / [H, W]), C in (1, 3), uint8 or float32 in
    [0, 1], numpy or device tensors.  alpha [H, W] or [B, H, W] (float, or uint8 read as / 255) with alpha_thres: the
    evaluator's standard background -- every pixel that is not alpha > alpha_thres turns white in both images first.
    -> {'psnr', 'mse', 'psnr_luma', 'ssim', 'ssim_luma'}: float64 device tensors [B].  No host synchronisation."""
    out = image_metrics_raw(a, b, alpha, alpha_thres).view(torch.float64)
    return {k: out[:, i] for i, k in enumerate(KEYS)}


class Base:
    """dtype as in xiuminglib: only 'uint8' images carry the 255 range these scores are defined on; float inputs of the
    calls are rows in [0, 1] and are quantised first."""

    key = None

    def __init__(self, dtype='uint8'):
        self.dtype = np.dtype(dtype)
        if self.dtype != np.uint8 and self.dtype.kind != 'f':
            raise NotImplementedError(self.dtype.kind)
        self.drange = 255.0

    def _score(self, im1, im2, mask=None):
        if mask is not None:
            raise NotImplementedError('masked scores: composite with image_metrics(alpha=, alpha_thres=) instead')
        return float(image_metrics(im1, im2)[self.key][0])


class _Masked(Base):
    def __call__(self, im1, im2, mask=None):
        return self._score(im1, im2, mask)


class _Ssim(Base):
    def __call__(self, im1, im2, multiscale=False):
        if multiscale:
            raise NotImplementedError('multi-scale SSIM is not implemented')
        return self._score(im1, im2)


class PSNR(_Masked):
    key = 'psnr'


class PSNR_luma(_Masked):
    key = 'psnr_luma'


class MSE(_Masked):
    key = 'mse'


class SSIM(_Ssim):
    key = 'ssim'


class SSIM_luma(_Ssim):
    key = 'ssim_luma'
