"""Time the segmentation scores on the scoring job of one scene: 8 views of 800 x 800, on two inputs and two paths.

  inputs  flat    every pixel carries one colour pair: all 64 lanes of every wave hold the same key (full contention on one counter);
          random  independent uniform labels 0 .. 21 per pixel and side: 484 keys, hardly two lanes of a wave agree;
  kernel  decomp/nerfactor/util/segmentation.contingency on device-resident uint8 colour images and a float alpha plane
          (csrc/segmentation_metrics.hip, two launches), and its label form on int32 labels;
  torch   the same table as torch ops on the same device: the palette comparison (21 passes per side), then
          bincount(g * C + p) over the counted pixels.

    python scripts/probe_segmentation_metrics.py [out.json]        -> profiles/segmentation_metrics.json unless told otherwise

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

from tests.gpu_util import launches                                         # noqa: E402
from vqnerf_release_amd import _C                                           # noqa: E402
from vqnerf_release_amd.decomp.nerfactor.util import segmentation           # noqa: E402

VIEWS, H, W = 8, 800, 800
THRES = 0.8


def torch_table(gt_rgb, pd_rgb, alpha, gt_pal, pd_pal):
    """the torch formulation: labels through the palette comparison, then one bincount -> int64 [R, C]"""
    def labels(rgb, pal):
        out = torch.zeros(rgb.shape[0], dtype=torch.int64, device=rgb.device)
        for i in range(pal.shape[0] - 1, -1, -1):
            out[(rgb == pal[i]).all(-1)] = i + 1
        return out
    R, C = gt_pal.shape[0] + 1, pd_pal.shape[0] + 1
    keep = alpha > THRES
    key = labels(gt_rgb, gt_pal)[keep] * C + labels(pd_rgb, pd_pal)[keep]
    return torch.bincount(key, minlength=R * C).view(R, C)


def timed(fn, repeats, warmup=3):
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'segmentation_metrics.json')
    assert torch.cuda.is_available(), 'needs cuda:0'
    dev = torch.device('cuda:0')
    n = VIEWS * H * W
    rng = np.random.default_rng(0)
    gt_pal, pd_pal = torch.as_tensor(segmentation.GT_PALETTE, device=dev), torch.as_tensor(segmentation.PD_PALETTE, device=dev)
    gt_tab = torch.cat([torch.zeros((1, 3), dtype=torch.uint8, device=dev), gt_pal])
    pd_tab = torch.cat([torch.zeros((1, 3), dtype=torch.uint8, device=dev), pd_pal])
    alpha = ((torch.arange(n, device=dev) % (H * W)) >= (H * W) // 10).to(torch.float32)          # the first tenth of every view is background
    inputs = {'flat': (torch.full((n,), 3, dtype=torch.int32, device=dev), torch.full((n,), 17, dtype=torch.int32, device=dev)),
              'random': (torch.as_tensor(rng.integers(0, 22, n).astype(np.int32), device=dev),
                         torch.as_tensor(rng.integers(0, 22, n).astype(np.int32), device=dev))}
    out = {'shape': [VIEWS, H, W], 'pixels': n, 'device': torch.cuda.get_device_name(0), 'pixels_per_pass': _C.SEG_PIXELS_PER_PASS,
           'grid_cap': _C.SEG_GRID_CAP}
    for name, (g, p) in inputs.items():
        gt_rgb, pd_rgb = gt_tab[g.long()].contiguous(), pd_tab[p.long()].contiguous()
        mask = (alpha > THRES).to(torch.uint8)
        with launches() as rec:
            got = segmentation.contingency(gt_rgb, pd_rgb, alpha=alpha, alpha_thres=THRES)
        want = torch_table(gt_rgb, pd_rgb, alpha, gt_pal, pd_pal)
        lab = segmentation.contingency(g, p, mask=mask)
        out[name] = {
            'kernel_entry_calls': rec.counts, 'kernel_launches': 2 * sum(rec.counts.values()),
            'kernel_rgb': timed(lambda: segmentation.contingency(gt_rgb, pd_rgb, alpha=alpha, alpha_thres=THRES), 30),
            'kernel_labels': timed(lambda: _C.segmentation_counts(g, p, mask, n_gt=21, n_pd=21), 30),
            'torch_rgb': timed(lambda: torch_table(gt_rgb, pd_rgb, alpha, gt_pal, pd_pal), 5, warmup=1),
            'torch_labels_bincount_only': timed(lambda: torch.bincount(g.long()[mask.bool()] * 22 + p.long()[mask.bool()], minlength=484), 5, warmup=1),
            'tables_equal': bool(torch.equal(got['contingency'], want) and torch.equal(lab['contingency'], want)),
            'counted_pixels': int(got['total']), 'purity': float(got['purity'])}
        out[name]['kernel_faster_than_torch'] = out[name]['kernel_rgb']['median_ms'] < out[name]['torch_rgb']['median_ms']
    out['flat_over_random_kernel_rgb'] = out['flat']['kernel_rgb']['median_ms'] / out['random']['kernel_rgb']['median_ms']
    out['flat_over_random_kernel_labels'] = out['flat']['kernel_labels']['median_ms'] / out['random']['kernel_labels']['median_ms']
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
