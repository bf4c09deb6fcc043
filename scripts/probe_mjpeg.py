"""Time the device JPEG encoder on the frames of a relighting sweep: 800 x 800, N = 1 and N = 17 frames a batch (one view under 16 probes
plus the model light), quality 75, both subsamplings, restart interval one MCU row.

    python scripts/probe_mjpeg.py [out.json]                 -> profiles/mjpeg.json unless told otherwise
    python scripts/probe_mjpeg.py --kernels SUB N            -> only encodes (CALLS batches after a warm-up): the program to put under
                                                                `rocprofv3 --kernel-trace --stats`, in a run of its own
    python scripts/probe_mjpeg.py --merge out.json SUB N kernel_stats.csv   -> folds that run's per-kernel times into out.json

Per configuration the first form records
  batch_to_host   host clock around JpegEncoder.encode: launches, the read of the [N, 2] offsets and lengths, the copy of the bytes --
                  it ends with the bytes on the host; median / min / max of REPEATS calls after a warm-up;
  entry_events    HIP events around the C entry (five launches, the device otherwise idle);
  bytes_per_frame
and beside them, on the same host and frames: PIL's JPEG encode (libjpeg, one thread, same quality and subsampling) and the existing
util/vis.write_png, per frame.  The frames are a shaded, textured disc over white, a different one per index: what a render looks like to
an entropy coder (flat background, smooth object, some grain).  Nothing here is asserted.  Needs an MI355X: there is no fallback."""
import csv
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vqnerf_release_amd import _C                                           # noqa: E402
from vqnerf_release_amd.decomp.nerfactor.util import mjpeg, vis             # noqa: E402

H = W = 800
QUALITY = 75
CALLS, REPEATS, WARMUP = 20, 15, 3
PIL_SUB = {'420': 2, '444': 0}


def frames(n):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for i in range(n):
        rng = np.random.default_rng(i)
        r2 = ((yy - 400) ** 2 + (xx - 400 - 4 * i) ** 2) / 300.0 ** 2
        shade = np.clip(1.0 - r2, 0, 1) ** 0.5
        col = np.array([0.9 - 0.03 * i, 0.5, 0.2 + 0.04 * i], np.float32)
        img = shade[..., None] * col * (0.8 + 0.2 * np.sin(xx / 9.0 + i)[..., None]) + rng.normal(0, 0.01, (H, W, 3)).astype(np.float32)
        img = np.where((r2 < 1)[..., None], img, 1.0)
        out.append((np.clip(img, 0, 1) * 255).astype(np.uint8))
    return np.stack(out)


def stat(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def measure(sub, n):
    host = frames(n)
    dev = torch.tensor(host).cuda()
    enc = mjpeg.JpegEncoder(quality=QUALITY, subsampling=sub)
    g, _ = enc._plan(dev)
    for _ in range(WARMUP):
        files = enc.encode(dev)
    t_host = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.encode(dev)
        t_host.append((time.perf_counter() - t0) * 1e3)
    _C.KernelClock.reset(True)
    for _ in range(REPEATS):
        enc.encode(dev)
        torch.cuda.synchronize()
    t_entry = [a.elapsed_time(b) for a, b in _C.KernelClock.pairs['vqn_jpeg_encode']]
    _C.KernelClock.reset(True)
    for _ in range(REPEATS):
        enc.coefficients(dev)
        torch.cuda.synchronize()
    t_dct = [a.elapsed_time(b) for a, b in _C.KernelClock.pairs['vqn_jpeg_encode']]
    _C.KernelClock.reset(False)
    from PIL import Image
    Image.fromarray(host[0]).save(io.BytesIO(), 'JPEG', quality=QUALITY, subsampling=PIL_SUB[sub])      # (the first call loads the codec)
    t_pil, pil_bytes = [], []
    for i in range(n):
        im = Image.fromarray(host[i])
        t0 = time.perf_counter()
        buf = io.BytesIO()
        im.save(buf, 'JPEG', quality=QUALITY, subsampling=PIL_SUB[sub])
        t_pil.append((time.perf_counter() - t0) * 1e3)
        pil_bytes.append(len(buf.getvalue()))
    t_png = []
    with tempfile.TemporaryDirectory() as d:
        for i in range(n):
            t0 = time.perf_counter()
            vis.write_png(os.path.join(d, f'{i}.png'), host[i])
            t_png.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(t_host)
    return {'frames': n, 'subsampling': sub, 'restart_interval_mcus': g['ri'], 'intervals_per_frame': g['intervals'],
            'entropy_workgroups': g['intervals'] * n, 'slot_bytes': g['slot_bytes'], 'scratch_bytes': g['scratch_bytes'], 'out_bytes_worst_case': g['out_bytes'],
            'bytes_per_frame': statistics.mean(len(f) for f in files), 'batch_to_host': stat(t_host), 'batch_to_host_per_frame_ms': med / n,
            'entry_events': stat(t_entry), 'entry_events_per_frame_ms': statistics.median(t_entry) / n,
            'first_kernel_alone_events': stat(t_dct),
            'pil_jpeg_one_thread_per_frame': stat(t_pil), 'pil_bytes_per_frame': statistics.mean(pil_bytes), 'write_png_per_frame': stat(t_png)}


def kernels_only(sub, n):
    dev = torch.tensor(frames(n)).cuda()
    enc = mjpeg.JpegEncoder(quality=QUALITY, subsampling=sub)
    for _ in range(WARMUP + CALLS):
        enc.encode(dev)
    torch.cuda.synchronize()


def merge(path, sub, n, stats_csv):
    out = json.load(open(path))
    per = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            if 'jpeg_' in row['Name']:
                name = row['Name'].split('jpeg_')[1].split('(')[0].split('<')[0]
                per['jpeg_' + name] = {'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3,
                                       'per_frame_us': float(row['AverageNs']) / 1e3 / int(n)}
    out['configs'][f'{sub}-N{n}']['kernels'] = per
    json.dump(out, open(path, 'w'), indent=1)
    print(json.dumps(per))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--kernels':
        return kernels_only(sys.argv[2], int(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == '--merge':
        return merge(*sys.argv[2:6])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'mjpeg.json')
    assert torch.cuda.is_available(), 'needs cuda:0'
    out = {'device': torch.cuda.get_device_name(0), 'frame': [H, W], 'quality': QUALITY, 'repeats': REPEATS, 'configs': {}}
    for sub in ('420', '444'):
        for n in (1, 17):
            out['configs'][f'{sub}-N{n}'] = measure(sub, n)
    out['note'] = ('batch_to_host is a host clock around one encode() call, which ends with the bytes on the host; entry_events one HIP event pair '
                   'around the C entry; kernels (where present) are rocprofv3 --kernel-trace --stats averages of a separate run of '
                   f'{WARMUP + CALLS} batches; the PIL and PNG times are per frame on one host thread')
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
