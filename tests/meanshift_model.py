"""The float64 statement of mean-shift clustering as csrc/meanshift.hip computes it: brute force in numpy, no
sklearn call.  It is what `sklearn.cluster.MeanShift(bandwidth=b, cluster_all=..., bin_seeding=False)` computes, with the arithmetic
fixed (tests/test_meanshift_model.py holds it to sklearn):

    d2(x, m) = sum over d = 0 .. D-1, in that order, of (x_d - m_d) * (x_d - m_d), product and sum rounded separately
    seek    per seed m: neighbours = the points with d2 <= b * b; none: dropped (count 0); m' = their mean; stop when
            sqrt(d2(m', m)) <= 1e-3 * b or when max_iter iterations are complete
    merge   means that are equal as tuples count once; sorted descending by (count, tuple); a mean that is not suppressed is kept and
            suppresses every other within d2 <= b * b
    assign  the index of the centre with the least d2, ties to the lowest; cluster_all=False: -1 where sqrt(d2) > b

While it runs it records how close it came to deciding otherwise (`margins`): a device that sums a mean in another order differs by
~1e-13 and takes the same decisions as long as these stay far above that."""
import numpy as np


def blobs(n, D, k, sigma, seed):
    """the test inputs: k Gaussian blobs of unequal weight in [0, 1]^D"""
    rng = np.random.default_rng(seed)
    cen = rng.random((k, D)) * 0.8 + 0.1
    w = rng.random(k) + 0.3
    lab = rng.choice(k, n, p=w / w.sum())
    return np.clip(cen[lab] + sigma * rng.standard_normal((n, D)), 0, 1)


def dist2(x, m):
    """x [..., D] against m [..., D] (broadcast) -> d2 in the fixed order"""
    x, m = np.asarray(x, np.float64), np.asarray(m, np.float64)
    s = np.zeros(np.broadcast_shapes(x.shape[:-1], m.shape[:-1]), np.float64)
    for d in range(x.shape[-1]):
        t = x[..., d] - m[..., d]
        s = s + t * t
    return s


def seek(X, seeds, b, max_iter=300, chunk=32):
    """-> (means [S, D], counts int [S] (0: dropped), iters int [S], margins {'distance', 'shift'})"""
    X, seeds = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(seeds, np.float64)
    S, D = seeds.shape
    bb, stop = b * b, 1e-3 * b
    means, counts, iters = seeds.copy(), np.zeros(S, np.int64), np.zeros(S, np.int64)
    active = np.ones(S, bool)
    XT = np.ascontiguousarray(X.T)                                           # a coordinate of all points, contiguous
    margin_d, margin_s = np.inf, np.inf
    while active.any():
        for s0 in range(0, S, chunk):
            idx = s0 + np.nonzero(active[s0:s0 + chunk])[0]
            if idx.size == 0:
                continue
            d2 = np.zeros((idx.size, X.shape[0]), np.float64)                # [seeds of the chunk, n]: dist2, a coordinate at a time
            for d in range(D):
                t = XT[d][None, :] - means[idx, d][:, None]
                np.multiply(t, t, out=t)
                np.add(d2, t, out=d2)
            margin_d = min(margin_d, float(np.abs(d2 - bb).min()))
            near = d2 <= bb
            for r, s in enumerate(idx):
                c = int(near[r].sum())
                counts[s] = c
                if c == 0:
                    active[s] = False
                    continue
                new = X[near[r]].mean(axis=0)
                shift = float(np.sqrt(dist2(new, means[s])))
                means[s] = new
                if shift > 0:
                    margin_s = min(margin_s, abs(shift - stop))
                if shift <= stop or iters[s] == max_iter:
                    active[s] = False
                else:
                    iters[s] += 1
    return means, counts, iters, {'distance': margin_d, 'shift': margin_s}


def merge(means, counts, b):
    """-> (centres [K, D] in order, the number of distinct means among the seeds that were not dropped, the merge margin
    min |d2 - b * b| over the pairs the walk compares)"""
    bb = b * b
    table = {}
    for m, c in zip(means, counts):
        if c > 0:
            table[tuple(m.tolist())] = int(c)
    ranked = sorted(table.items(), key=lambda kv: (kv[1], kv[0]), reverse=True)
    cand = np.array([k for k, _ in ranked], np.float64).reshape(len(ranked), means.shape[1])
    alive = np.ones(len(ranked), bool)
    keep, margin = [], np.inf
    for i in range(len(ranked)):
        if not alive[i]:
            continue
        keep.append(i)
        if i + 1 < len(ranked):
            d2 = dist2(cand[i + 1:], cand[i])
            margin = min(margin, float(np.abs(d2 - bb).min()))
            alive[i + 1:] &= ~(d2 <= bb)
    return cand[keep], len(ranked), margin


def assign(X, centres, b=0.0):
    """-> (labels int [n] (b > 0: -1 where the nearest centre is farther than b), dist [n], the smallest gap between a point's
    nearest and second nearest centre distance (inf for one centre))"""
    X, centres = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(centres, np.float64)
    labels, dist, gap = np.zeros(len(X), np.int64), np.zeros(len(X), np.float64), np.inf
    for i0 in range(0, len(X), 65536):
        d = np.sqrt(dist2(X[i0:i0 + 65536, None, :], centres[None, :, :]))   # [points, K]
        lab = d.argmin(axis=1)                                               # the first of equal minima
        labels[i0:i0 + 65536], dist[i0:i0 + 65536] = lab, d[np.arange(len(lab)), lab]
        if centres.shape[0] > 1:
            two = np.partition(d, 1, axis=1)
            gap = min(gap, float((two[:, 1] - two[:, 0]).min()))
    if b > 0:
        labels = np.where(dist > b, -1, labels)
    return labels, dist, gap


def fit(X, b, max_iter=300, cluster_all=True, seeds=None):
    """-> dict(centres, labels, dist, n_iter, means, counts, iters, distinct, margins {'distance', 'shift', 'merge', 'label_gap'});
    ValueError when every seed is dropped"""
    X = np.ascontiguousarray(X, np.float64)
    means, counts, iters, margins = seek(X, X if seeds is None else seeds, b, max_iter)
    if not (counts > 0).any():
        raise ValueError(f'no point was within bandwidth={b} of any seed')
    centres, distinct, margins['merge'] = merge(means, counts, b)
    labels, dist, margins['label_gap'] = assign(X, centres, 0.0 if cluster_all else b)
    return dict(centres=centres, labels=labels, dist=dist, n_iter=int(iters.max()), means=means, counts=counts, iters=iters, distinct=distinct,
                margins=margins)
