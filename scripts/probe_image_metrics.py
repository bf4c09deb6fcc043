"""Time the image metrics on the scoring job of one relit view: 17 pairs (rgb + 16 probes) of 800 x 800 x 3, on three paths.

  kernel  decomp/nerfactor/util/metric.image_metrics on device-resident uint8 images (csrc/image_metrics.hip, two launches);
  torch   the same scores as torch ops on the same device: the four moment planes of the three channels and luma through two
          depthwise conv2d (float64, as the kernel accumulates; and float32 for comparison), then the quotient and the means;
  host    the float64 numpy statement on one pair (tests/image_metrics_model.py) times 17, plus the 34 device-to-host copies it needs.

    python scripts/probe_image_metrics.py [out.json]        -> profiles/image_metrics.json unless told otherwise

Times are medians of device-synchronised wall-clock repeats after a warm-up.  Needs an MI355X: there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import image_metrics_model as M                                  # noqa: E402
from tests.gpu_util import launches                                         # noqa: E402
from vqnerf_release_amd.decomp.nerfactor.util import metric                 # noqa: E402

B, H, W, C = 17, 800, 800, 3


def torch_scores(a8, b8, dtype):
    """SSIM and luma SSIM [B] with torch ops: NCHW planes (R, G, B, luma), two depthwise convolutions per moment"""
    w = torch.as_tensor(metric.gaussian_window(), device=a8.device, dtype=dtype)
    x, y = a8.permute(0, 3, 1, 2).to(dtype), b8.permute(0, 3, 1, 2).to(dtype)
    lw = torch.tensor(M.LUMA, device=a8.device, dtype=dtype).view(1, 3, 1, 1)
    x, y = torch.cat([x, (x * lw).sum(1, keepdim=True)], 1), torch.cat([y, (y * lw).sum(1, keepdim=True)], 1)
    planes = torch.cat([x, y, x * y, x * x + y * y], 1)                       # [B, 16, H, W]
    n = planes.shape[1]
    h = torch.nn.functional.conv2d(planes, w.view(1, 1, 1, -1).expand(n, 1, 1, -1), groups=n)
    v = torch.nn.functional.conv2d(h, w.view(1, 1, -1, 1).expand(n, 1, -1, 1), groups=n)
    mx, my, sxy, sxx = v[:, 0:4], v[:, 4:8], v[:, 8:12], v[:, 12:16]
    s = ((2 * mx * my + M.C1) * (2 * sxy - 2 * mx * my + M.C2)) / ((mx * mx + my * my + M.C1) * (sxx - mx * mx - my * my + M.C2))
    s = s.mean((2, 3))
    return s[:, :3].mean(1), s[:, 3]


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'repeats': repeats}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'image_metrics.json')
    assert torch.cuda.is_available(), 'needs cuda:0'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = ((xx + yy) / float(H + W - 2) * 1.3 - 0.15)[None, :, :, None] + rng.normal(0, 0.1, (B, H, W, C))
    base[:, :, :W // 4] = 1.0                                                # a white background strip
    a8 = M.to_uint8(base)
    b8 = M.to_uint8(base + rng.normal(0, 0.04, (B, H, W, C)))
    a, b = torch.as_tensor(a8, device=dev), torch.as_tensor(b8, device=dev)

    out = {'shape': [B, H, W, C], 'device': torch.cuda.get_device_name(0)}
    with launches() as rec:
        got = metric.image_metrics(a, b)
    out['kernel_entry_calls'] = rec.counts
    out['kernel_launches'] = 2 * sum(rec.counts.values())                    # the tile kernel and the finalize kernel per call
    out['kernel'] = timed(lambda: metric.image_metrics(a, b), 20)
    out['torch_f64'] = timed(lambda: torch_scores(a, b, torch.float64), 5, warmup=1)
    out['torch_f32'] = timed(lambda: torch_scores(a, b, torch.float32), 5, warmup=1)

    def host():
        ah, bh = [a[i].cpu().numpy() for i in range(B)], [b[i].cpu().numpy() for i in range(B)]        # the 34 copies
        return M.metrics(ah[0], bh[0])
    t0 = time.perf_counter()
    m0 = host()
    one = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for i in range(B):
        a[i].cpu(), b[i].cpu()
    copies = (time.perf_counter() - t0) * 1e3
    out['host_f64'] = {'copies_ms': copies, 'one_pair_ms': one - copies, 'estimated_17_pairs_ms': copies + B * (one - copies),
                       'note': 'one pair scored, times 17, plus the 34 device-to-host copies'}

    s64, l64 = torch_scores(a, b, torch.float64)
    s32, l32 = torch_scores(a, b, torch.float32)
    out['max_abs_diff'] = {'kernel_vs_torch_f64_ssim': float((got['ssim'] - s64).abs().max()), 'kernel_vs_torch_f64_ssim_luma': float((got['ssim_luma'] - l64).abs().max()),
                           'torch_f32_vs_torch_f64_ssim': float((s32.double() - s64).abs().max()), 'kernel_vs_host_pair0_ssim': abs(float(got['ssim'][0]) - m0['ssim']),
                           'kernel_vs_host_pair0_psnr': abs(float(got['psnr'][0]) - m0['psnr'])}
    out['kernel_faster_than_torch_f64'] = out['kernel']['median_ms'] < out['torch_f64']['median_ms']
    out['kernel_faster_than_torch_f32'] = out['kernel']['median_ms'] < out['torch_f32']['median_ms']
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
