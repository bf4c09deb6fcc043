"""NumPy statement of the geometry scores (csrc/geometry_eval.hip, geo/geometry_eval.py): triangle areas and
surface samples in float64 from float32 coordinates, the nearest neighbour as a brute force in float32 whose three products and two
sums are separate float32 operations (argmin: the lowest index among equals), and the directed sums with math.fsum.  The kernels'
per-point results are compared with these bit for bit.  Helpers only, no tests."""
import math

import numpy as np

F32_INF = np.float32(np.inf)


def _corners(vertices, triangles):
    v = np.asarray(vertices, np.float32).astype(np.float64)
    t = np.asarray(triangles).astype(np.int64)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def _cross(v0, v1, v2):
    e1, e2 = v1 - v0, v2 - v0
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                     e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def _length(c):
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def tri_areas(vertices, triangles):
    """float64 [T]: 0.5 |(v1 - v0) x (v2 - v0)|"""
    return 0.5 * _length(_cross(*_corners(vertices, triangles)))


def sample_surface(vertices, triangles, cum, u):
    """cum float64 [T] (the inclusive prefix sum of the areas), u float32 [n, 3] -> (points f32 [n,3], normals f32 [n,3], face int32)"""
    cum = np.asarray(cum, np.float64)
    u = np.asarray(u, np.float32).astype(np.float64)
    x = u[:, 0] * cum[-1]
    face = np.minimum(np.searchsorted(cum, x, 'right'), len(cum) - 1)
    v0, v1, v2 = (c[face] for c in _corners(vertices, triangles))
    s = np.sqrt(u[:, 1])
    a, b, c = 1.0 - s, s * (1.0 - u[:, 2]), s * u[:, 2]
    points = (a[:, None] * v0 + b[:, None] * v1) + c[:, None] * v2
    n = _cross(v0, v1, v2)
    length = _length(n)
    with np.errstate(invalid='ignore', divide='ignore'):
        normals = np.where(length[:, None] > 0.0, n / length[:, None], 0.0)
    return points.astype(np.float32), normals.astype(np.float32), face.astype(np.int32)


def nearest(query, ref, max_d2=np.inf, chunk=512):
    """-> (d2 float32 [n_q], idx int32 [n_q]): the least d2 = (dx dx + dy dy) + dz dz in float32, ties to the lowest index; where
    that d2 > max_d2 (as float32): +inf and -1."""
    q, r = np.asarray(query, np.float32), np.asarray(ref, np.float32)
    d2, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int32)
    for s in range(0, len(q), chunk):
        d = r[None, :, :] - q[s: s + chunk, None, :]
        p = d * d
        t = (p[..., 0] + p[..., 1]) + p[..., 2]
        assert t.dtype == np.float32
        k = np.argmin(t, 1)
        idx[s: s + chunk], d2[s: s + chunk] = k, t[np.arange(len(k)), k]
    far = d2 > np.float32(max_d2)
    d2[far], idx[far] = F32_INF, -1
    return d2, idx


def reduce(d2, idx, thresholds=(), q_normals=None, ref_normals=None):
    """The directed sums of one nearest-neighbour result, over the valid queries (idx >= 0)."""
    d2, idx = np.asarray(d2, np.float32), np.asarray(idx)
    valid = idx >= 0
    dd = d2[valid].astype(np.float64)
    d = np.sqrt(dd)
    out = {'n': len(d2), 'n_valid': int(valid.sum()), 'count': [int((d < float(t)).sum()) for t in thresholds],
           'sum_d': math.fsum(d), 'sum_d2': math.fsum(dd), 'max_d': float(d.max()) if len(d) else 0.0, 'sum_dot': 0.0, 'pairs': 0}
    if q_normals is not None and ref_normals is not None:
        a = np.asarray(q_normals, np.float32)[valid].astype(np.float64)
        b = np.asarray(ref_normals, np.float32)[idx[valid]].astype(np.float64)
        both = (a != 0).any(1) & (b != 0).any(1)
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        out['sum_dot'], out['pairs'] = math.fsum(np.abs(dot[both])), int(both.sum())
    return out


def _mean(s, n):
    return s / n if n else float('nan')


def scores(pred_to_gt, gt_to_pred, thresholds=()):
    """The scores from the two directed reductions (the outputs of `reduce`)."""
    p, g = pred_to_gt, gt_to_pred
    out = {'n_pred': p['n'], 'n_gt': g['n'], 'n_pred_valid': p['n_valid'], 'n_gt_valid': g['n_valid'],
           'n_pred_far': p['n'] - p['n_valid'], 'n_gt_far': g['n'] - g['n_valid'],
           'accuracy': _mean(p['sum_d'], p['n_valid']), 'completeness': _mean(g['sum_d'], g['n_valid']),
           'accuracy_max': p['max_d'], 'completeness_max': g['max_d']}
    out['chamfer'] = 0.5 * (out['accuracy'] + out['completeness'])
    out['chamfer_l2'] = 0.5 * (_mean(p['sum_d2'], p['n_valid']) + _mean(g['sum_d2'], g['n_valid']))
    out['thresholds'] = [float(t) for t in thresholds]
    out['precision'] = [_mean(c, p['n_valid']) for c in p['count']]
    out['recall'] = [_mean(c, g['n_valid']) for c in g['count']]
    out['fscore'] = [2.0 * a * b / (a + b) if a + b > 0 else (0.0 if a + b == 0 else float('nan'))
                     for a, b in zip(out['precision'], out['recall'])]
    out['normal_consistency'] = 0.5 * (_mean(p['sum_dot'], p['pairs']) + _mean(g['sum_dot'], g['pairs']))
    return out


def surface_scores(pred_points, pred_normals, gt_points, gt_normals, thresholds=(), max_dist=None):
    """Point clouds (normals may be None) -> the dict of `scores`.  max_dist: queries farther than it leave the sums; the rule is
    d2 > fl(max_dist * max_dist) in float32."""
    max_d2 = np.inf if max_dist is None else np.float32(max_dist) * np.float32(max_dist)
    d2, idx = nearest(pred_points, gt_points, max_d2)
    p = reduce(d2, idx, thresholds, pred_normals, gt_normals)
    d2, idx = nearest(gt_points, pred_points, max_d2)
    g = reduce(d2, idx, thresholds, gt_normals, pred_normals)
    return scores(p, g, thresholds)
