"""Time mean-shift clustering on the device at the reference's size and at ten times it.

  fit      decomp/nerfactor/util/meanshift.MeanShift(0.2).fit on n = 10,000 and n = 100,000 points of 7 features (every point a seed):
           8 Gaussian blobs of sigma 0.07 in the unit cube, the generator of tests/meanshift_model.py;
  predict  640,000 fresh points against the centres of the n = 10,000 fit (a validation view of 800 x 800).

    python scripts/probe_meanshift.py [out.json]        -> profiles/meanshift.json unless told otherwise

Times are HIP events around a whole call on the launch stream (a fit ends in its read-back of K, so the stream is drained), medians
of repeats after a warm-up; the per-kernel times of one fit come from the package's KernelClock.  The float64 vector rate of this
part has not been measured in this project: the pair rate below is what these kernels reach, not a share of any peak.  The host
figure beside them was NOT measured on this machine.  Needs an MI355X: there is no fallback."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.gpu_util import launches                                         # noqa: E402
from tests.meanshift_model import blobs                                     # noqa: E402
from vqnerf_release_amd import _C                                           # noqa: E402
from vqnerf_release_amd.decomp.nerfactor.util.meanshift import MeanShift    # noqa: E402

D, BANDWIDTH, BLOBS, SIGMA = 7, 0.2, 8, 0.07
# sklearn.cluster.MeanShift(bandwidth=0.2).fit on 10,000 x 7 of the same generator: 9 clusters, 12 iterations (scikit-learn 1.7.2,
# n_jobs=None, 8 virtual CPUs of a DIFFERENT host than the one this script runs on)
HOST_SKLEARN = {'seconds': 37.0, 'n': 10000, 'clusters': 9, 'n_iter': 12, 'measured_on': 'a different host: 8 vCPUs, scikit-learn 1.7.2, n_jobs=None'}


def timed(fn, repeats, warmup=2):
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


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'meanshift.json')
    assert torch.cuda.is_available(), 'needs cuda:0'
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'features': D, 'bandwidth': BANDWIDTH, 'points_per_tile': _C.MEANSHIFT_POINTS_PER_TILE,
           'seeds_per_workgroup': _C.MEANSHIFT_SEEDS_PER_GROUP, 'host_sklearn': HOST_SKLEARN,
           'note': 'float64 vector rate of the part not measured in this project: pair rates are achieved rates, not shares of a peak'}
    centres = None
    for n, repeats in ((10000, 10), (100000, 3)):
        x = torch.as_tensor(blobs(n, D, BLOBS, SIGMA, 0), device=dev)
        with launches() as rec:
            model = MeanShift(BANDWIDTH).fit(x)
        clock = _C.KernelClock
        clock.reset(True)
        MeanShift(BANDWIDTH).fit(x)
        torch.cuda.synchronize()
        kernels = {k: v[1] for k, v in clock.summary().items()}
        clock.reset(False)
        iters = model.iters_.to(torch.int64)
        pairs = int((iters + 1).sum()) * n                                   # (seed, iteration, point) distance tests of the seek launch
        res = {'fit': timed(lambda: MeanShift(BANDWIDTH).fit(x), repeats), 'n_iter': model.n_iter_, 'mean_iters_per_seed': float(iters.double().mean()),
               'clusters': int(model.cluster_centers_.shape[0]), 'entry_calls_per_fit': rec.counts, 'hip_kernel_launches_per_fit': sum(rec.counts.values()),
               'kernel_ms_one_fit': kernels, 'seek_distance_tests': pairs,
               'seek_distance_tests_per_second': pairs / (kernels['vqn_meanshift_seek'] * 1e-3)}
        out[f'n={n}'] = res
        if centres is None:
            centres = model
    fresh = torch.rand((640000, D), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    calls = 50                                                               # one call is tens of microseconds: time a run of them

    def predicts():
        for _ in range(calls):
            centres.predict(fresh)
    run = timed(predicts, 10, warmup=2)
    out['predict_640000'] = {'calls_per_window': calls, 'per_call_ms': run['median_ms'] / calls, 'window': run,
                             'note': 'the 36 MB of points stay cache-resident between calls'}
    out['n=10000']['host_sklearn_over_fit'] = HOST_SKLEARN['seconds'] * 1e3 / out['n=10000']['fit']['median_ms']
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
