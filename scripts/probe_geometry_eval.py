"""Time the nearest-neighbour search of the geometry scores on the job of one evaluation: both directions between 1,000,000 surface
samples of a resolution-512 marching-cubes sphere and 1,000,000 points of the analytic sphere, on three paths.

  kernel  geo/geometry_eval.nearest on device-resident points (csrc/geometry_eval.hip): the whole call -- bounding box, grid plan,
          cell ids, the two sorts, the pack, the search -- and the search launch alone;
  torch   a brute force on the same device: torch.cdist of 1024 queries against all reference points, then min, chunk by chunk
          (timed on the first 65,536 queries of each direction and scaled to all of them: the full pass is 10^12 pairs);
  host    scipy.spatial.cKDTree(ref).query(query, workers=16) in float64, with the two device-to-host copies, if scipy imports.

    python scripts/probe_geometry_eval.py [out.json]        -> profiles/geometry_eval.json unless told otherwise

Kernel times are medians of 20 repeats between device events after a warm-up.  Also recorded: the points per occupied cell at the
default cell size, and the times at half and twice that size.  Needs an MI355X: there is no fallback."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqnerf_release_amd import _C                                           # noqa: E402
from vqnerf_release_amd.geo import geometry_eval as ge                      # noqa: E402
from vqnerf_release_amd.geo import mesh                                     # noqa: E402

N, RES, RADIUS = 1000000, 512, 0.6
TORCH_QUERIES, TORCH_CHUNK = 65536, 1024


def timed(fn, repeats=20, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'repeats': repeats}


def torch_bruteforce(query, ref):
    d2 = torch.empty(query.shape[0], device=query.device)
    idx = torch.empty(query.shape[0], dtype=torch.int64, device=query.device)
    for s in range(0, query.shape[0], TORCH_CHUNK):
        m = torch.cdist(query[s: s + TORCH_CHUNK], ref).min(1)
        d2[s: s + TORCH_CHUNK], idx[s: s + TORCH_CHUNK] = m.values, m.indices
    return d2, idx


def search_only(query, ref, cell=None):
    """the launch of vqn_geom_nearest alone, on a reference and a query order built beforehand"""
    r = ge.Reference(ref, cell)
    q_order = torch.sort(_C.geom_cell_ids(query, r.grid)).indices.to(torch.int32)
    return r, (lambda: _C.geom_nearest(query, r.packed, r.cell_start, r.grid, float('inf'), q_order))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'geometry_eval.json')
    assert torch.cuda.is_available(), 'needs cuda:0'
    dev = torch.device('cuda:0')
    ax = torch.linspace(-1.0, 1.0, RES, device=dev)
    u = RADIUS - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    step = 2.0 / (RES - 1)
    v, t = mesh.marching_cubes(u.contiguous(), 0.0, origin=(-1.0, -1.0, -1.0), step=(step, step, step))
    del u
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    pred, _, _ = mesh.sample_surface(v, t, N, generator=gen)
    g = torch.randn((N, 3), device=dev, generator=gen, dtype=torch.float64)
    gt = (RADIUS * g / g.norm(dim=1, keepdim=True)).float().contiguous()
    pairs = {'pred_to_gt': (pred, gt), 'gt_to_pred': (gt, pred)}

    out = {'points': N, 'mesh': {'resolution': RES, 'vertices': int(v.shape[0]), 'triangles': int(t.shape[0])},
           'device': torch.cuda.get_device_name(0), 'directions': {}}
    results = {}
    for name, (q, r) in pairs.items():
        d = out['directions'][name] = {}
        results[name] = ge.nearest(q, r)
        ref, fn = search_only(q, r)
        h = float(ref.grid.h)
        counts = (ref.cell_start[1:] - ref.cell_start[:-1]).to(torch.float64)
        occupied = counts[counts > 0]
        d['grid'] = {'h': h, 'dims': list(ref.grid.dims), 'cells': int(ref.grid.cells), 'occupied_cells': int(occupied.numel()),
                     'points_per_occupied_cell_mean': float(occupied.mean()), 'points_per_occupied_cell_max': int(occupied.max())}
        d['kernel_whole_call'] = timed(lambda: ge.nearest(q, r))
        d['kernel_search_only'] = timed(fn)
        for tag, cell in (('half_h', h / 2), ('h_over_1.6', h / 1.6), ('twice_h', 2 * h)):
            try:
                _, fn_c = search_only(q, r, cell)
            except ValueError as e:                               # (at 10^6 points h / 2 needs more than 2^24 cells)
                d['kernel_' + tag] = {'h': cell, 'refused': str(e)}
                continue
            d['kernel_' + tag] = {'h': cell, 'whole_call': timed(lambda: ge.nearest(q, r, cell=cell), 10), 'search_only': timed(fn_c, 10)}
            d2c, idxc = ge.nearest(q, r, cell=cell)
            d['kernel_' + tag]['same_bits_as_default'] = bool(torch.equal(d2c, results[name][0]) and torch.equal(idxc, results[name][1]))
        sub = q[:TORCH_QUERIES]
        tb = timed(lambda: torch_bruteforce(sub, r), 3, warmup=1)
        tb['queries'] = TORCH_QUERIES
        tb['estimated_all_queries_ms'] = tb['median_ms'] * N / TORCH_QUERIES
        tb['note'] = f'cdist + min in chunks of {TORCH_CHUNK} queries, timed on the first {TORCH_QUERIES} queries and scaled to {N}'
        d['torch_bruteforce'] = tb
        bi = torch_bruteforce(sub, r)[1]
        d['torch_bruteforce']['indices_equal_to_kernel'] = float((bi == results[name][1][:TORCH_QUERIES]).double().mean())

    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
        out['host_kdtree'] = 'not run: scipy does not import here'
    if cKDTree is not None:
        for name, (q, r) in pairs.items():
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                qh, rh = q.cpu().numpy().astype(np.float64), r.cpu().numpy().astype(np.float64)      # the two copies
                dist, idx = cKDTree(rh).query(qh, workers=16)
                ts.append((time.perf_counter() - t0) * 1e3)
            out['directions'][name]['host_kdtree'] = {
                'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'repeats': 3, 'workers': 16,
                'note': 'float64 cKDTree build + query, with the two device-to-host copies',
                'indices_equal_to_kernel': float((idx == results[name][1].cpu().numpy()).mean()),
                'max_rel_d2_difference': float(np.max(np.abs(results[name][0].cpu().numpy().astype(np.float64) - dist ** 2) / np.maximum(dist ** 2, 1e-30)))}

    def total(key, field='median_ms'):
        return sum(d[key][field] for d in out['directions'].values())
    out['both_directions_ms'] = {'kernel_whole_call': total('kernel_whole_call'), 'kernel_search_only': total('kernel_search_only'),
                                 'torch_bruteforce_estimated': total('torch_bruteforce', 'estimated_all_queries_ms')}
    out['kernel_faster_than_torch_bruteforce'] = out['both_directions_ms']['kernel_whole_call'] < out['both_directions_ms']['torch_bruteforce_estimated']
    out['torch_bruteforce_over_kernel'] = out['both_directions_ms']['torch_bruteforce_estimated'] / out['both_directions_ms']['kernel_whole_call']
    if cKDTree is not None:
        out['both_directions_ms']['host_kdtree'] = total('host_kdtree')
        out['kernel_faster_than_host_kdtree'] = out['both_directions_ms']['kernel_whole_call'] < out['both_directions_ms']['host_kdtree']
        out['host_kdtree_over_kernel'] = out['both_directions_ms']['host_kdtree'] / out['both_directions_ms']['kernel_whole_call']
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
