"""Float64 statement of the segmentation scores of csrc/segmentation_metrics.hip, written from the definition (numpy only).

The reference's decomp/nerfvq_nfr3/cluster_eval.py scores a predicted label image against a hand-labelled one:
  * `img_embed`: a pixel's label is 1 + the index of the first palette row it equals exactly, 0 when it equals none; class 0 takes
    part like any other.  The two palettes differ: the ground truth's half intensity is 127, the prediction's 128;
  * only pixels with alpha > alpha_thres (strict) are counted;
  * `resort`: the labels that occur are renumbered 0, 1, ... in ascending order, per side -- here: the *present* rows / columns of
    the contingency table coo[g][p], those with a non-zero sum;
  * `correspond`: label_map[p] = argmax_g coo[g][p] (ties: the lowest row, as np.argmax), every predicted label is replaced by it;
  * purity = sum_p max_g coo[g][p] / total, and sklearn's f1_score (micro, macro), precision_score and recall_score (macro) of the
    replaced prediction: with the merged confusion M[g][g'] = sum of coo[g][p] over p with label_map[p] = g', per present row g
        tp = M[g][g], pred = sum_r M[r][g], true = sum_c M[g][c],
        precision = tp / pred (0 when pred = 0), recall = tp / true, f1 = 2 tp / (2 tp + (pred - tp) + (true - tp)),
    the macro scores being the sums over present rows in ascending order divided by their number, f1_micro = sum tp / total.
With no counted pixel the five scores are NaN (the reference would divide by zero).

The label form takes integer labels in [0, n_gt] x [0, n_pd] directly; a counted pixel with a label outside is not entered in the
table but counted as `invalid`."""
import numpy as np

KEYS = ('purity', 'f1-micro', 'f1-macro', 'p-macro', 'r-macro')


def _palette(half):
    f, h = 255, half
    return np.array([[f, 0, 0], [0, f, 0], [0, 0, f], [f, f, 0], [f, 0, f], [0, f, f],
                     [h, 0, 0], [0, h, 0], [0, 0, h], [h, h, 0], [h, 0, h], [0, h, h],
                     [f, h, h], [h, f, h], [h, h, f], [f, f, h], [f, h, f], [h, f, f],
                     [f, h, 0], [f, 0, h], [0, f, h]], np.uint8)


GT_PALETTE = _palette(127)        # cluster_eval.py: sel_colors
PD_PALETTE = _palette(128)        # cluster_eval.py: embed_c


def palette_labels(rgb, palette):
    """uint8 [n, 3] -> int64 [n]: 1 + the index of the first palette row the pixel equals, 0 for none"""
    rgb = np.asarray(rgb).reshape(-1, 3)
    labels = np.zeros(rgb.shape[0], np.int64)
    for i in range(len(palette) - 1, -1, -1):                    # descending: the first matching row is the one left standing
        labels[np.all(rgb == np.asarray(palette[i], rgb.dtype), axis=-1)] = i + 1
    return labels


def counted(alpha, thres):
    """bool [n]: alpha > thres, strict, compared in float32 as the kernel does"""
    return np.asarray(alpha, np.float32).reshape(-1) > np.float32(thres)


def table(gt, pd, n_gt, n_pd, keep=None):
    """integer labels [n] -> (coo int64 [n_gt + 1, n_pd + 1], invalid): counted pixels with a label out of range are `invalid`"""
    gt, pd = np.asarray(gt).reshape(-1).astype(np.int64), np.asarray(pd).reshape(-1).astype(np.int64)
    if keep is not None:
        keep = np.asarray(keep).reshape(-1).astype(bool)
        gt, pd = gt[keep], pd[keep]
    R, C = n_gt + 1, n_pd + 1
    ok = (gt >= 0) & (gt < R) & (pd >= 0) & (pd < C)
    coo = np.bincount(gt[ok] * C + pd[ok], minlength=R * C).reshape(R, C).astype(np.int64)
    return coo, int((~ok).sum())


def scores(coo):
    """contingency table -> dict: the five scores (Python floats), 'label_map' (int list, -1 for absent columns), 'total',
    'rows', 'cols' (the numbers of present rows / columns)"""
    coo = np.asarray(coo, np.int64)
    R, C = coo.shape
    rowsum, colsum = [int(v) for v in coo.sum(1)], [int(v) for v in coo.sum(0)]
    total = sum(rowsum)
    present = [g for g in range(R) if rowsum[g] > 0]
    label_map, colmax = [], []
    for p in range(C):
        best, arg = 0, -1
        for g in range(R):
            if int(coo[g, p]) > best:                            # strict: a tie stays with the lowest row
                best, arg = int(coo[g, p]), g
        label_map.append(arg)
        colmax.append(best)
    out = {'label_map': label_map, 'total': total, 'rows': len(present), 'cols': sum(c > 0 for c in colsum)}
    if total == 0:
        out.update({k: float('nan') for k in KEYS})
        return out
    ps = rs = fs = 0.0
    tp_sum = 0
    for g in present:
        tp = sum(int(coo[g, p]) for p in range(C) if label_map[p] == g)
        pred = sum(colsum[p] for p in range(C) if label_map[p] == g)
        true = rowsum[g]
        tp_sum += tp
        ps += 0.0 if pred == 0 else float(tp) / float(pred)
        rs += float(tp) / float(true)
        fs += float(2 * tp) / float(2 * tp + (pred - tp) + (true - tp))
    n = float(len(present))
    out.update({'purity': float(sum(colmax)) / float(total), 'f1-micro': float(tp_sum) / float(total),
                'f1-macro': fs / n, 'p-macro': ps / n, 'r-macro': rs / n})
    return out


def evaluate_labels(gt, pd, n_gt, n_pd, keep=None):
    coo, invalid = table(gt, pd, n_gt, n_pd, keep)
    out = scores(coo)
    out['contingency'], out['invalid'] = coo, invalid
    return out


def evaluate_rgb(gt_rgb, pd_rgb, alpha=None, alpha_thres=0.8, gt_palette=GT_PALETTE, pd_palette=PD_PALETTE):
    """the colour form: uint8 [..., 3] images, alpha [...] or None"""
    keep = None if alpha is None else counted(alpha, alpha_thres)
    return evaluate_labels(palette_labels(gt_rgb, gt_palette), palette_labels(pd_rgb, pd_palette), len(gt_palette), len(pd_palette), keep)
