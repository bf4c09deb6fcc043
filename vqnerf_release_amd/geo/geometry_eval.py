"""Surface scores of a mesh or point cloud against a reference, on the device (csrc/geometry_eval.hip): accuracy,
completeness and Chamfer distance (the DTU convention), precision / recall / F-score at distance thresholds, normal consistency.  The
counterpart of decomp/metric_eval.py (images) and decomp/cluster_eval.py (segmentation) for the geometry half; the reference ships no
geometry evaluator, so the definitions are the module's own and tests/geometry_eval_model.py restates them in NumPy.

Every score is a sum over the EXACT nearest neighbour of each point of one surface among the points of the other: `nearest` sorts the
reference into a uniform grid and answers every query in one launch; the cell size changes the time, never a bit of the result.
A call reads the host once per direction (the reference's bounding box) and once at the end (the sums)."""
import glob
import json
import os

import numpy as np
import torch

from vqnerf_release_amd import _C
from vqnerf_release_amd.geo import mesh

THRESHOLDS = (0.005, 0.01, 0.02, 0.05)      # default distance thresholds, in the units of the coordinates
N_SAMPLES = 1000000                         # surface samples of a mesh


def _points(t, what):
    _C.require_device(t, what)
    if t.dim() != 2 or t.shape[1] != 3:
        raise _C.VqnError(f'{what}: expected [n, 3], got {tuple(t.shape)}')
    return t.detach().to(torch.float32).contiguous()


class Reference:
    """A point cloud sorted into a grid: what `nearest` builds from `ref`, kept to answer several query sets."""

    def __init__(self, ref, cell=None):
        ref = _points(ref, 'nearest: ref')
        if ref.shape[0] == 0:
            raise _C.VqnError('nearest: the reference has no points')
        box = torch.stack([ref.min(0).values, ref.max(0).values]).tolist()      # the one host read
        self.grid = _C.geom_grid_plan(box[0], box[1], ref.shape[0], cell)
        ids, order = torch.sort(_C.geom_cell_ids(ref, self.grid), stable=True)
        cells = torch.arange(self.grid.cells + 1, dtype=torch.int32, device=ref.device)
        self.cell_start = torch.searchsorted(ids, cells, out_int32=True)
        self.packed = _C.geom_pack_sorted(ref, order)
        self.n = int(ref.shape[0])

    def nearest(self, query, max_dist=None):
        query = _points(query, 'nearest: query')
        max_d2 = float('inf') if max_dist is None else float(np.float32(max_dist) * np.float32(max_dist))
        q_order = None
        if query.shape[0] > _C.GEOM_THREADS:                  # queries of a wave walk the same cells
            q_order = torch.sort(_C.geom_cell_ids(query, self.grid)).indices.to(torch.int32)
        return _C.geom_nearest(query, self.packed, self.cell_start, self.grid, max_d2, q_order)


def nearest(query, ref, max_dist=None, cell=None):
    """query [n_q,3], ref [n_ref,3] device tensors -> (d2 f32 [n_q], idx int32 [n_q]): per query the least
    d2 = (dx dx + dy dy) + dz dz, every operation rounded to float32, and the index of the reference point that has it, the lowest
    among equals.  max_dist: a query whose d2 > fl(max_dist * max_dist) gets +inf and -1.  cell: the grid's cell size (None: chosen
    from the reference's bounding box and count); no result depends on it."""
    return Reference(ref, cell).nearest(query, max_dist)


def _surface(s, n_samples, generator, bounds, what):
    """(vertices, triangles) or (points, normals | None) -> (points f32 [n,3], normals f32 [n,3] | None), inside `bounds`"""
    a, b = s
    if b is not None and not b.dtype.is_floating_point:
        pts, nrm, _ = mesh.sample_surface(a, b, n_samples, generator=generator)
    else:
        pts, nrm = _points(a, what), None if b is None else _points(b, what + ' normals')
        if nrm is not None and nrm.shape != pts.shape:
            raise _C.VqnError(f'{what}: {tuple(nrm.shape)} normals for {tuple(pts.shape)} points')
    if bounds is not None:
        lo, hi = (torch.as_tensor(x, dtype=torch.float32, device=pts.device) for x in bounds)
        keep = ((pts >= lo) & (pts <= hi)).all(1)
        pts, nrm = pts[keep].contiguous(), None if nrm is None else nrm[keep].contiguous()
    if pts.shape[0] == 0:
        raise _C.VqnError(f'{what}: no point' + (' inside the bounds' if bounds is not None else ''))
    return pts, nrm


def _mean(s, n):
    return s / n if n else float('nan')


def scores_from_words(p, g, thresholds):
    """The scores from the two rows of vqn_geom_reduce's words (pred -> gt, gt -> pred), host int64 arrays."""
    pf, gf = p.view(np.float64), g.view(np.float64)
    K = len(thresholds)
    out = {'n_pred': int(p[0]), 'n_gt': int(g[0]), 'n_pred_valid': int(p[1]), 'n_gt_valid': int(g[1]),
           'n_pred_far': int(p[0] - p[1]), 'n_gt_far': int(g[0] - g[1]),
           'accuracy': _mean(float(pf[10]), int(p[1])), 'completeness': _mean(float(gf[10]), int(g[1])),
           'accuracy_max': float(pf[12]), 'completeness_max': float(gf[12])}
    out['chamfer'] = 0.5 * (out['accuracy'] + out['completeness'])
    out['chamfer_l2'] = 0.5 * (_mean(float(pf[11]), int(p[1])) + _mean(float(gf[11]), int(g[1])))
    out['thresholds'] = [float(t) for t in thresholds]
    out['precision'] = [_mean(int(c), int(p[1])) for c in p[2: 2 + K]]
    out['recall'] = [_mean(int(c), int(g[1])) for c in g[2: 2 + K]]
    out['fscore'] = [2.0 * a * b / (a + b) if a + b > 0 else (0.0 if a + b == 0 else float('nan'))
                     for a, b in zip(out['precision'], out['recall'])]
    out['normal_consistency'] = 0.5 * (_mean(float(pf[13]), int(p[14])) + _mean(float(gf[13]), int(g[14])))
    return out


def surface_scores(pred, gt, thresholds=THRESHOLDS, max_dist=None, n_samples=N_SAMPLES, seed=0, bounds=None, samples=None):
    """pred, gt: (vertices [V,3], triangles int [T,3]) -- sampled to n_samples points with their face normals, from a generator seeded
    with `seed` -- or (points [n,3], normals [n,3] | None).  bounds = (lo, hi): points outside that box are dropped first.  -> dict:
      accuracy = mean d(pred -> gt), completeness = mean d(gt -> pred), chamfer = their mean, chamfer_l2 = the mean of the two mean
      squared distances, accuracy_max / completeness_max = the two directed Hausdorff terms;
      precision[k] = the share of valid pred points with d < thresholds[k], recall[k] the same for gt -> pred,
      fscore = 2 P R / (P + R), 0 when P + R = 0;
      normal_consistency = the mean of the two directed means of |n . n_nearest| (NaN without normals on both sides);
      n_pred, n_gt, n_pred_valid, n_gt_valid, n_pred_far, n_gt_far: with max_dist, points farther than it from the other surface
      leave the means (valid = the rest; none valid: NaN).
    samples (a dict, optional) receives the points and normals that were scored."""
    thresholds = tuple(float(t) for t in thresholds)
    gen = None
    if any(s[1] is not None and not s[1].dtype.is_floating_point for s in (pred, gt)):
        gen = torch.Generator(device=pred[0].device)
        gen.manual_seed(int(seed))
    pp, pn = _surface(pred, n_samples, gen, bounds, 'surface_scores: pred')
    gp, gn = _surface(gt, n_samples, gen, bounds, 'surface_scores: gt')
    if samples is not None:
        samples.update(pred_points=pp, pred_normals=pn, gt_points=gp, gt_normals=gn)
    words = []
    for (qp, qn), (rp, rn) in (((pp, pn), (gp, gn)), ((gp, gn), (pp, pn))):
        d2, idx = nearest(qp, rp, max_dist)
        words.append(_C.geom_reduce(d2, idx, rp.shape[0], thresholds, qn, rn))
    p, g = torch.stack(words).cpu().numpy()                   # the read-back
    return scores_from_words(p, g, thresholds)


def _load(path, device):
    v, t, n = mesh.read_ply(path, device)
    return (v, t) if t is not None and len(t) else (v, n)


def evaluate(pred_path, gt_path, out_json=None, device='cuda', **kw):
    """Scores the PLY file pred_path (a mesh, or a point cloud) against gt_path (the same; DTU's scans are point clouds) with
    `surface_scores` (**kw) and writes the dict as JSON: out_json, or geometry.json next to the prediction.  Returns the dict."""
    out = surface_scores(_load(pred_path, device), _load(gt_path, device), **kw)
    out['pred'], out['gt'] = os.path.basename(pred_path), os.path.basename(gt_path)
    if out_json is None:
        out_json = os.path.join(os.path.dirname(os.path.abspath(pred_path)), 'geometry.json')
    with open(out_json, 'w') as f:
        json.dump(out, f)
    return out


def newest_mesh(mesh_dir):
    """the `{iter:08d}.ply` of mesh_dir with the highest iteration"""
    files = sorted(p for p in glob.glob(os.path.join(mesh_dir, '*.ply')) if os.path.basename(p)[:-4].isdigit())
    if not files:
        raise FileNotFoundError(f'{mesh_dir}: no <iteration>.ply')
    return max(files, key=lambda p: int(os.path.basename(p)[:-4]))
