"""Material segmentation scores on the device: what the reference's decomp/nerfvq_nfr3/cluster_eval.py computes on the host with
21 boolean passes per palette and `sklearn.metrics` -- purity, micro / macro F1, macro precision and macro recall of a predicted
label image against a hand-labelled one.

`contingency` turns two label images into the contingency table coo[g][p] and the scores in two launches of
csrc/segmentation_metrics.hip and leaves everything on the device (tests/segmentation_model.py is the float64 statement):
  * colour form, uint8 [..., 3]: a pixel's label is 1 + the index of the first palette row it equals exactly, 0 when it equals none
    (class 0 takes part).  `GT_PALETTE` is the reference's `sel_colors` (half intensity 127, the hand-labelled `idx.png`),
    `PD_PALETTE` its `embed_c` (half intensity 128, the written `embed_map.png`); the difference is the reference's;
  * label form, integers of any shape: labels in [0, n_gt] and [0, n_pd], e.g. `encoding_indices` or the float `embed` image;
  * a pixel is counted when alpha > alpha_thres (strict) and, if given, mask is set;
  * the labels that occur on each side are the *present* rows / columns; label_map[p] = the row with the largest count in column p
    (ties: the lowest); every predicted label is replaced by its row, and the scores are those of that replaced prediction.
There is no CPU path: numpy inputs are uploaded."""
import numpy as np
import torch

from vqnerf_release_amd import _C

KEYS = ('purity', 'f1-micro', 'f1-macro', 'p-macro', 'r-macro')  # words 0..4 of the library's output row; the reference's key names


def _palette(half):
    f, h = 255, half
    return np.array([[f, 0, 0], [0, f, 0], [0, 0, f], [f, f, 0], [f, 0, f], [0, f, f],
                     [h, 0, 0], [0, h, 0], [0, 0, h], [h, h, 0], [h, 0, h], [0, h, h],
                     [f, h, h], [h, f, h], [h, h, f], [f, f, h], [f, h, f], [h, f, f],
                     [f, h, 0], [f, 0, h], [0, f, h]], np.uint8)


GT_PALETTE = _palette(127)        # cluster_eval.py: sel_colors
PD_PALETTE = _palette(128)        # cluster_eval.py: embed_c
_UNIT8 = np.arange(256, dtype=np.float32) / np.float32(255)      # a byte of alpha as a float in [0, 1]


def _device_of(*ts):
    return next((t.device for t in ts if torch.is_tensor(t) and t.is_cuda), torch.device('cuda'))


def _labels(t, dev):
    """integer or float label image of any shape -> int32 [n] on the device (floats are rounded to nearest, as np.rint)"""
    t = torch.as_tensor(t).to(dev).reshape(-1)
    if t.is_floating_point():
        t = torch.round(t)
    elif t.dtype == torch.bool:
        raise ValueError('label images are integers (or the float embed image), got bool')
    return t.to(torch.int32).contiguous()


def contingency_raw(gt, pd, alpha=None, alpha_thres=0.8, mask=None, gt_palette=GT_PALETTE, pd_palette=PD_PALETTE, n_gt=None, n_pd=None):
    """-> (the library's output row, int64 [42 + R * C] (include/vqn_eval.h), R, C)"""
    dev = _device_of(gt, pd, alpha, mask)
    gt, pd = torch.as_tensor(gt), torch.as_tensor(pd)
    colour = gt.dtype == torch.uint8 and pd.dtype == torch.uint8 and gt.dim() >= 1 and gt.shape[-1] == 3 and pd.shape[-1] == 3
    if gt.shape != pd.shape:
        raise ValueError(f'the two label images differ in shape: {tuple(gt.shape)} and {tuple(pd.shape)}')
    n = gt.numel() // 3 if colour else gt.numel()
    keep = None
    if alpha is not None:
        alpha = torch.as_tensor(alpha).to(dev)
        if alpha.dtype == torch.uint8:                           # a / 255 correctly rounded, from a host table: a device division by a
            alpha = torch.as_tensor(_UNIT8, device=dev)[alpha.long()]        # constant may multiply by 1 / 255 and lift 204 / 255 above 0.8
        alpha = alpha.to(torch.float32).reshape(-1).contiguous()
        if alpha.numel() != n:
            raise ValueError(f'alpha has {alpha.numel()} values for {n} pixels')
    if mask is not None:
        keep = torch.as_tensor(mask).to(dev).reshape(-1) != 0
        if keep.numel() != n:
            raise ValueError(f'mask has {keep.numel()} values for {n} pixels')
    if colour:
        gt_palette, pd_palette = np.asarray(gt_palette, np.uint8).reshape(-1, 3), np.asarray(pd_palette, np.uint8).reshape(-1, 3)
        if (n_gt is not None and n_gt != len(gt_palette)) or (n_pd is not None and n_pd != len(pd_palette)):
            raise ValueError('n_gt / n_pd of the colour form are the palettes\' row counts')
        if keep is not None:                                     # both tests folded into one plane; alone, alpha goes to the kernel as it is
            if alpha is not None:
                keep = keep & (alpha > alpha_thres)
            alpha, alpha_thres = keep.to(torch.float32), 0.5
        out = _C.segmentation_counts(gt.to(dev).reshape(-1, 3).contiguous(), pd.to(dev).reshape(-1, 3).contiguous(), alpha, alpha_thres,
                                     gt_palette=gt_palette, pd_palette=pd_palette)
        return out, len(gt_palette) + 1, len(pd_palette) + 1
    n_gt = len(gt_palette) if n_gt is None else int(n_gt)
    n_pd = len(pd_palette) if n_pd is None else int(n_pd)
    if alpha is not None:
        keep = (alpha > alpha_thres) if keep is None else keep & (alpha > alpha_thres)
    sel = None if keep is None else keep.to(torch.uint8).contiguous()
    out = _C.segmentation_counts(_labels(gt, dev), _labels(pd, dev), sel, n_gt=n_gt, n_pd=n_pd)
    return out, n_gt + 1, n_pd + 1


def contingency(gt, pd, alpha=None, alpha_thres=0.8, mask=None, gt_palette=GT_PALETTE, pd_palette=PD_PALETTE, n_gt=None, n_pd=None):
    """Contingency table and scores of a predicted label image `pd` against the ground truth `gt` (numpy or device tensors).
    uint8 [..., 3]: the colour form (labels through the palettes, R = len(gt_palette) + 1, C = len(pd_palette) + 1); integers (or
    the float embed image, rounded) of any shape: the label form, labels in [0, n_gt] x [0, n_pd] (default: the palettes' row
    counts; 64 at most).  alpha [...] (float, or uint8 read as / 255): counted when alpha > alpha_thres, strict; mask [...]:
    counted when set.
    -> {'purity', 'f1-micro', 'f1-macro', 'p-macro', 'r-macro'}: float64 device scalars (NaN when no pixel is counted);
       'contingency' int64 [R, C]; 'label_map' int32 [C] (the ground-truth label a predicted label is read as, -1: absent);
       'total', 'invalid' (counted pixels with a label out of range: label form only), 'present_rows', 'present_cols': int64
       device scalars.  No host synchronisation."""
    out, R, C = contingency_raw(gt, pd, alpha, alpha_thres, mask, gt_palette, pd_palette, n_gt, n_pd)
    f = out[:5].view(torch.float64)
    res = {k: f[i] for i, k in enumerate(KEYS)}
    res['contingency'] = out[_C.SEG_HEAD_WORDS:].view(R, C)
    res['label_map'] = out[9:_C.SEG_HEAD_WORDS].view(torch.int32)[:C]
    res['total'], res['invalid'], res['present_rows'], res['present_cols'] = out[5], out[6], out[7], out[8]
    return res


def scores(gt, pd, alpha=None, alpha_thres=0.8, mask=None, gt_palette=GT_PALETTE, pd_palette=PD_PALETTE, n_gt=None, n_pd=None):
    """the same call -> only the five scores {'purity', 'f1-micro', 'f1-macro', 'p-macro', 'r-macro'} (float64 device scalars)"""
    res = contingency(gt, pd, alpha, alpha_thres, mask, gt_palette, pd_palette, n_gt, n_pd)
    return {k: res[k] for k in KEYS}
