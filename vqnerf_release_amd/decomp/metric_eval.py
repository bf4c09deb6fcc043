"""Scene evaluator: the counterpart of the reference's decomp/nerfvq_nfr3/metric_eval.py (the script behind the paper's tables) on
the device metrics of decomp/nerfactor/util/metric.py.

`evaluate(pred_root, gt_root)` walks the view directories `pred_root/batch<NNNNNNNNN>` that `train_nfr.render_views` writes and
pairs view number N with the ground-truth directory `gt_root/val_NNN` (the walk, the pairing, the loaders and the size check are
decomp/view_tree.py's):

    group   prediction                                   ground truth
    rgb     pred_rgb.png                                 rgba.png (its colour channels)
    kd      pred_albedo.png                              albedo.png
    ks      pred_ks.png, else pred_spec.png              metal.png
    rough   pred_rough.png                               rough.png
    env     pred_rgb_probes_<name>.png, every <name>     rgba_<name>.png
            (under relight_root/<view> if given)

A pair is scored when both files exist.  Every image is put on the evaluator's standard background first: wherever the alpha
channel of rgba.png is not above `alpha_thres` (strict; 0.95, the reference uses 0.8 for real captures) both images turn white, so
that differences in the methods' own masks do not enter the score.  All pairs of a view are uploaded once and scored by one call
(two launches).  PSNR and SSIM per group and view, their means, and `metrics.json` under `pred_root`.

`use_scale` aligns the predicted albedo to the ground truth per channel before scoring (albedo is only defined up to scale): the
scale is the mean over views of  sum(gt * alpha) / sum(pred * alpha)  with alpha the ground truth's alpha channel in [0, 1]; the
scaled prediction is clipped and quantised as every written image is.

Not rebuilt: LPIPS (no network weights in this package), the sRGB conversion switch of albedo / specular, the other methods'
directory layouts, and the `cv2` resize of images whose sizes differ -- a size mismatch raises."""
import glob
import json
import os

import numpy as np
import torch

from vqnerf_release_amd.decomp import view_tree
from vqnerf_release_amd.decomp.nerfactor.util import metric

_FIXED = (('rgb', ('pred_rgb.png',), 'rgba.png'), ('kd', ('pred_albedo.png',), 'albedo.png'),
          ('ks', ('pred_ks.png', 'pred_spec.png'), 'metal.png'), ('rough', ('pred_rough.png',), 'rough.png'))
GROUPS = ('rgb', 'kd', 'ks', 'rough', 'env')


def _first(dirname, names):
    return next((os.path.join(dirname, n) for n in names if os.path.exists(os.path.join(dirname, n))), None)


def _view_pairs(pred_dir, gt_dir, relight_dir):
    """[(group, prediction path, ground-truth path)] of one view"""
    pairs = []
    for group, preds, gt in _FIXED:
        p, g = _first(pred_dir, preds), os.path.join(gt_dir, gt)
        if p is not None and os.path.exists(g):
            pairs.append((group, p, g))
    for p in sorted(glob.glob(os.path.join(relight_dir, 'pred_rgb_probes_*.png'))):
        g = os.path.join(gt_dir, 'rgba_' + os.path.basename(p)[len('pred_rgb_probes_'):])
        if os.path.exists(g):
            pairs.append(('env', p, g))
    return pairs


def _views(pred_root, gt_root, relight_root):
    out = []
    for name in view_tree.view_dirs(pred_root, view_tree.BATCH_VIEWS):
        gt_dir = os.path.join(gt_root, view_tree.gt_view(name))
        if not os.path.exists(os.path.join(gt_dir, 'rgba.png')):
            continue
        relight_dir = os.path.join(relight_root if relight_root is not None else pred_root, name)
        out.append((name, os.path.join(pred_root, name), gt_dir, relight_dir))
    return out


def albedo_scale(views, device):
    """per-channel scale of the predicted albedo: mean over views of sum(gt * alpha) / sum(pred * alpha) -> float64 [3] (device)"""
    ratios = []
    for _, pred_dir, gt_dir, _ in views:
        p, g = os.path.join(pred_dir, 'pred_albedo.png'), os.path.join(gt_dir, 'albedo.png')
        if not (os.path.exists(p) and os.path.exists(g)):
            continue
        pred, gt, alpha = (torch.as_tensor(a, device=device).to(torch.float64) / 255.0
                           for a in (view_tree.read_image(p), view_tree.read_image(g), view_tree.read_alpha(os.path.join(gt_dir, 'rgba.png'))))
        view_tree.check_sizes(pred_dir, {p: pred.shape[:2], g: gt.shape[:2], 'alpha': alpha.shape})
        ratios.append((gt * alpha[..., None]).sum((0, 1)) / (pred * alpha[..., None]).sum((0, 1)))
    if not ratios:
        raise ValueError('use_scale: no view has both pred_albedo.png and albedo.png')
    return torch.stack(ratios).mean(0)


def evaluate(pred_root, gt_root, relight_root=None, alpha_thres=0.95, use_scale=False, device='cuda'):
    """-> {group: {'psnr': [...], 'ssim': [...], 'psnr_mean', 'ssim_mean'}, 'views': [...]} (only groups with a scored pair; with
    use_scale also 'kd_scale'), written to pred_root/metrics.json as well.  See the module docstring."""
    device = torch.device(device)
    views = _views(pred_root, gt_root, relight_root)
    scale = albedo_scale(views, device) if use_scale else None
    pending = []                                                 # (groups of the view's pairs, device scores): read back at the end
    for name, pred_dir, gt_dir, relight_dir in views:
        pairs = _view_pairs(pred_dir, gt_dir, relight_dir)
        if not pairs:
            continue
        alpha = view_tree.read_alpha(os.path.join(gt_dir, 'rgba.png'))
        images = {path: view_tree.read_image(path) for _, p, g in pairs for path in (p, g)}
        view_tree.check_sizes(name, dict({path: a.shape[:2] for path, a in images.items()}, alpha=alpha.shape))
        pred_d = torch.as_tensor(np.stack([images[p] for _, p, _ in pairs]), device=device)
        gt_d = torch.as_tensor(np.stack([images[g] for _, _, g in pairs]), device=device)
        if scale is not None:
            for i, (group, _, _) in enumerate(pairs):
                if group == 'kd':
                    scaled = (pred_d[i].to(torch.float64) / 255.0 * scale).to(torch.float32)
                    pred_d[i] = (scaled.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
        res = metric.image_metrics(gt_d, pred_d, alpha=torch.as_tensor(alpha, device=device), alpha_thres=alpha_thres)
        pending.append((name, [g for g, _, _ in pairs], res['psnr'], res['ssim']))
    out = {}
    for name, groups, psnr, ssim in pending:
        for group, p, s in zip(groups, psnr.tolist(), ssim.tolist()):
            d = out.setdefault(group, {'psnr': [], 'ssim': []})
            d['psnr'].append(p)
            d['ssim'].append(s)
    for d in out.values():
        d['psnr_mean'], d['ssim_mean'] = float(np.mean(d['psnr'])), float(np.mean(d['ssim']))
    out = {g: out[g] for g in GROUPS if g in out}
    out['views'] = [name for name, _, _, _ in pending]
    if scale is not None:
        out['kd_scale'] = scale.tolist()
    with open(os.path.join(pred_root, 'metrics.json'), 'w') as f:
        json.dump(out, f)
    return out
