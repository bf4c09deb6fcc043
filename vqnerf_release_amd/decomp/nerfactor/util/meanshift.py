"""Mean-shift clustering on the device: what the reference's decomp/nerfvq_nfr3/meanshift.py gets from `sklearn.cluster.MeanShift`
(flat kernel, `bin_seeding=False`: every sample is a seed, `cluster_all`) -- the baseline column of the segmentation table.

Three kernels of csrc/meanshift.hip, everything float64 and left on the device (tests/meanshift_model.py is the statement, DESIGN
section 10 the arithmetic):
  * seek    every seed climbs to its mode in ONE launch: neighbours are the points with d2 <= b * b, the mean is their sum / their
            number, a seed stops when it moved by <= 1e-3 * b or after `max_iter` completed iterations; a seed without neighbours
            is dropped;
  * merge   the seeds' means, sorted descending by (neighbour count, coordinates) with torch on the device, are walked in order: a
            mean that is not suppressed becomes a centre and suppresses every later one within b;
  * assign  a point's label is the index of its nearest centre, ties to the lowest; `cluster_all=False`: -1 beyond b.
`fit` reads one number back, K (0: every seed was dropped).  There is no CPU path: numpy inputs are uploaded."""
import numpy as np
import torch

from vqnerf_release_amd import _C

_UNIT8 = np.arange(256, dtype=np.float64) / 255.      # a byte as k / 255. in float64, correctly rounded


def _shape_of(x, what):
    if not torch.is_tensor(x):
        x = np.asarray(x)
    shape = tuple(int(s) for s in x.shape)
    if len(shape) != 2:
        raise ValueError(f'{what} must be [n, D], got shape {shape}')
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError(f'{what} is empty: shape {shape}')
    if shape[1] > _C.MEANSHIFT_MAX_DIM:
        raise ValueError(f'{what} has D = {shape[1]} features per point; the kernels take at most {_C.MEANSHIFT_MAX_DIM}')
    return shape


def features(x, device=None, what='x'):
    """numpy array or tensor [n, D], float32 / float64 / uint8 (read as k / 255.) -> contiguous float64 [n, D] on the device.
    Raises ValueError (before anything touches the device) for an empty input, D > 8 or another dtype."""
    if not torch.is_tensor(x):
        x = np.asarray(x)
    _shape_of(x, what)
    t = torch.as_tensor(x)
    if t.dtype not in (torch.float32, torch.float64, torch.uint8):
        raise ValueError(f'{what} must be float32, float64 or uint8, got {t.dtype}')
    if device is None:
        device = t.device if t.is_cuda else torch.device('cuda')
    t = t.to(device)
    if t.dtype == torch.uint8:                                   # k / 255. from a host table: a device division by a constant may
        t = torch.as_tensor(_UNIT8, device=device)[t.long()]     # multiply by a rounded reciprocal
    return t.to(torch.float64).contiguous()


class MeanShift:
    """MeanShift(bandwidth, max_iter=300, cluster_all=True, seeds=None): `fit(x)`, `predict(x)`; after a fit
        cluster_centers_   float64 [K, D] on the device, in sklearn's order (descending neighbour count)
        labels_            int32 [n] on the device (-1: farther than the bandwidth from every centre, cluster_all=False only)
        n_iter_            the largest number of completed iterations of a seed
        means_, counts_, iters_   per seed: where it stopped, the size of its last neighbour set (0: dropped), its iterations
    seeds: [S, D] start points (default: every sample)."""

    def __init__(self, bandwidth, max_iter=300, cluster_all=True, seeds=None):
        self.bandwidth, self.max_iter, self.cluster_all, self.seeds = bandwidth, max_iter, cluster_all, seeds

    def _check(self):
        if not float(self.bandwidth) > 0.0:
            raise ValueError(f'bandwidth must be > 0, got {self.bandwidth}')
        if int(self.max_iter) < 0:
            raise ValueError(f'max_iter must be >= 0, got {self.max_iter}')

    def fit(self, x):
        self._check()
        n, D = _shape_of(x, 'x')
        if self.seeds is not None and _shape_of(self.seeds, 'seeds')[1] != D:
            raise ValueError(f'seeds and x differ in their features per point; x has {D}')
        x = features(x)
        seeds = x if self.seeds is None else features(self.seeds, x.device, 'seeds')
        b = float(self.bandwidth)
        means, counts, iters = _C.meanshift_seek(x, seeds, b, int(self.max_iter))
        # descending by (count, m_0, .., m_{D-1}): stable sorts from the last key to the first
        order = torch.arange(means.shape[0], device=x.device)
        for key in [means[:, d] for d in range(D - 1, -1, -1)] + [counts]:
            order = order[torch.sort(key[order], descending=True, stable=True)[1]]
        cand = means[order].contiguous()
        kept, n_kept = _C.meanshift_merge(cand, counts[order].contiguous(), b)
        K = int(n_kept)                                          # the one read-back
        if K == 0:
            raise ValueError(f'No point was within bandwidth={b} of any seed. Try a different seeding strategy or increase the bandwidth.')
        first = torch.sort(kept, descending=True, stable=True)[1][:K]        # the kept rows, in order
        self.means_, self.counts_, self.iters_ = means, counts, iters
        self.cluster_centers_ = cand[first].contiguous()
        self._n_iter = iters.max()
        self.labels_ = _C.meanshift_assign(x, self.cluster_centers_, 0.0 if self.cluster_all else b)[0]
        return self

    @property
    def n_iter_(self):
        return int(self._n_iter)

    def predict(self, x):
        """-> int32 [n] on the device: the index of the nearest centre (every point is labelled, as sklearn's predict does)"""
        centres = getattr(self, 'cluster_centers_', None)
        if centres is None:
            raise ValueError('predict before fit')
        n, D = _shape_of(x, 'x')
        if D != centres.shape[1]:
            raise ValueError(f'x has {D} features per point, the model was fitted on {centres.shape[1]}')
        return _C.meanshift_assign(features(x, centres.device), centres, 0.0)[0]
