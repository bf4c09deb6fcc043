"""Time the device PNG encoder on the frames of a relighting sweep (those of scripts/probe_mjpeg.py): 800 x 800, N = 1 and N = 17 images a
batch, C = 3 and C = 1 (the green plane), adaptive filter, default segments; and the output path of one view with both writers.

    python scripts/probe_png.py [out.json]                   -> profiles/png.json unless told otherwise
    python scripts/probe_png.py --view out.json              -> adds the view of scripts/probe_output.py (800 x 800, 16 probes, 28 files)
                                                                 written with png='host' and png='device' to out.json
    python scripts/probe_png.py --kernels C N                -> only encodes (CALLS batches after a warm-up): the program to put under
                                                                 `rocprofv3 --kernel-trace --stats`, in a run of its own
    python scripts/probe_png.py --merge out.json C N kernel_stats.csv   -> folds that run's per-kernel times into out.json

Each is one GPU step: run them one after the other, each under its own `timeout`, chained with `&&`.

Per configuration the first form records
  batch_to_host   host clock around PngEncoder.streams: launches, the read of the [N, 2] offsets and lengths, the copy of the bytes --
                  it ends with the compressed bytes on the host; median / min / max of REPEATS calls after a warm-up;
  files           the same around PngEncoder.encode, which adds the IDAT CRC and the chunk framing on the calling thread;
  entry_events    HIP events around the C entry (four launches, the device otherwise idle); filter_alone_events the first kernel alone;
  bytes_per_frame against PIL at compress_level=3 (what util/vis.write_png writes)
and beside them, in the same run on the same frames, the baseline: util/vis.write_png per frame on one host thread.  Nothing here is
asserted.  Needs an MI355X: there is no fallback."""
import csv
import importlib.util
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
from vqnerf_release_amd.decomp.nerfactor.util import png, vis               # noqa: E402

CALLS, REPEATS, WARMUP = 20, 15, 3


def frames(n, c):
    spec = importlib.util.spec_from_file_location('probe_mjpeg', os.path.join(ROOT, 'scripts', 'probe_mjpeg.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    f = mod.frames(n)
    return f if c == 3 else np.ascontiguousarray(f[..., 1])


def stat(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def clocked(fn, repeats=REPEATS):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def measure(c, n):
    host = frames(n, c)
    dev = torch.tensor(host).cuda()
    enc = png.PngEncoder()
    _, (g, _) = enc._plan(dev)
    for _ in range(WARMUP):
        files = enc.encode(dev)
    t_streams = clocked(lambda: enc.streams(dev))
    t_files = clocked(lambda: enc.encode(dev))
    _C.KernelClock.reset(True)
    for _ in range(REPEATS):
        enc.streams(dev)
        torch.cuda.synchronize()
    t_entry = [a.elapsed_time(b) for a, b in _C.KernelClock.pairs['vqn_png_encode']]
    _C.KernelClock.reset(True)
    for _ in range(REPEATS):
        enc.filtered(dev)
        torch.cuda.synchronize()
    t_filter = [a.elapsed_time(b) for a, b in _C.KernelClock.pairs['vqn_png_encode']]
    _C.KernelClock.reset(False)
    from PIL import Image
    t_png, pil_bytes = [], []
    with tempfile.TemporaryDirectory() as d:
        vis.write_png(os.path.join(d, 'warm.png'), host[0])
        for i in range(n):
            t0 = time.perf_counter()
            vis.write_png(os.path.join(d, f'{i}.png'), host[i])
            t_png.append((time.perf_counter() - t0) * 1e3)
            pil_bytes.append(os.path.getsize(os.path.join(d, f'{i}.png')))
    for i in range(n):                                                      # the files are PNGs of these frames
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[i]))), host[i])
    med = statistics.median(t_streams)
    return {'images': n, 'channels': c, 'rows_per_segment': g['rows_per_segment'], 'segment_bytes': g['segment_bytes'],
            'segments_per_image': g['segments'], 'deflate_waves': g['segments'] * n, 'scratch_bytes': g['scratch_bytes'],
            'out_bytes_worst_case': g['out_bytes'], 'bytes_per_frame': statistics.mean(len(f) for f in files),
            'pil_level3_bytes_per_frame': statistics.mean(pil_bytes), 'batch_to_host': stat(t_streams), 'batch_to_host_per_frame_ms': med / n,
            'files': stat(t_files), 'files_per_frame_ms': statistics.median(t_files) / n, 'entry_events': stat(t_entry),
            'entry_events_per_frame_ms': statistics.median(t_entry) / n, 'filter_alone_events': stat(t_filter),
            'write_png_per_frame': stat(t_png)}


def kernels_only(c, n):
    dev = torch.tensor(frames(n, c)).cuda()
    enc = png.PngEncoder()
    for _ in range(WARMUP + CALLS):
        enc.streams(dev)
    torch.cuda.synchronize()


def merge(path, c, n, stats_csv):
    out = json.load(open(path))
    per = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            if 'png_' in row['Name']:
                name = row['Name'].split('png_')[1].split('(')[0].split('<')[0]
                per['png_' + name] = {'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3,
                                      'per_frame_us': float(row['AverageNs']) / 1e3 / int(n)}
    out['configs'][f'C{c}-N{n}']['kernels'] = per
    json.dump(out, open(path, 'w'), indent=1)
    print(json.dumps(per))


def view(path):
    """the loop of scripts/probe_output.py with both writers: ms per view of the GPU loop and until the files are on disk"""
    import bench
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.nerfactor.util.io import config_from_dict
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(1)
    model = get_model_class('vq_nfr')(config_from_dict(bench.DECOMP_INI))
    model.build_nets(device=dev, seed=0).to(dev)
    cb = rng.uniform(0, 1, (15, 256)).astype(np.float32)
    model.set_codebook(cb / np.linalg.norm(cb, axis=1, keepdims=True))
    model.set_light(rng.uniform(0, 1, (16, 32, 3)).astype(np.float32))
    model.novel_probes = {f'probe{i:02d}': torch.tensor(rng.uniform(0, 2, (16, 32, 3)).astype(np.float32)).to(dev) for i in range(16)}
    H = W = 800
    n = H * W
    xyz = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1)
    nrm = torch.nn.functional.normalize(xyz + 0.1 * torch.randn(n, 3, device=dev), dim=-1)
    one = torch.ones(n, 1, device=dev)
    batch = (['v'], torch.tensor([[H, W]], device=dev).repeat(n, 1), torch.tensor([[0, 0, 4.0]], device=dev).repeat(n, 1),
             torch.zeros(n, 3, device=dev), torch.rand(n, 3, device=dev), one, one.clone(), xyz, nrm,
             (torch.rand(n, 512, device=dev) < 0.7).float())
    res = {'views': 6, 'writer_threads': 12}
    with torch.no_grad(), tempfile.TemporaryDirectory() as out:
        for _ in range(2):
            model.fast_render(batch, mode='test', relight_probes=True)
        torch.cuda.synchronize()
        V = res['views']
        t0 = time.perf_counter()
        for v in range(V):
            model.fast_render(batch, mode='test', relight_probes=True)
        torch.cuda.synchronize()
        res['render_only_ms_per_view'] = (time.perf_counter() - t0) / V * 1e3
        for mode in ('host', 'device'):
            w = vis.AsyncWriter(n_threads=res['writer_threads'])
            _, _, _, to_vis = model.fast_render(batch, mode='test', relight_probes=True)           # (warm-up of this writer's path)
            model.vis_batch(to_vis, os.path.join(out, mode + 'w'), mode='test', writer=w, png=mode).flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for v in range(V):
                _, _, _, to_vis = model.fast_render(batch, mode='test', relight_probes=True)
                model.vis_batch(to_vis, os.path.join(out, mode + str(v)), mode='test', writer=w, png=mode)
            torch.cuda.synchronize()
            t_loop = (time.perf_counter() - t0) / V
            w.flush()
            t_total = (time.perf_counter() - t0) / V
            names = os.listdir(os.path.join(out, mode + '0'))
            res[mode] = {'gpu_loop_ms_per_view': t_loop * 1e3, 'files_on_disk_ms_per_view': t_total * 1e3, 'files_per_view': len(names),
                         'png_bytes_per_view': sum(os.path.getsize(os.path.join(out, mode + '0', f)) for f in names if f.endswith('.png'))}
    doc = json.load(open(path))
    doc['view_800x800_16_probes'] = res
    json.dump(doc, open(path, 'w'), indent=1)
    print(json.dumps(res))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--kernels':
        return kernels_only(int(sys.argv[2]), int(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == '--merge':
        return merge(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    if len(sys.argv) > 1 and sys.argv[1] == '--view':
        return view(sys.argv[2])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'png.json')
    assert torch.cuda.is_available(), 'needs cuda:0'
    out = {'device': torch.cuda.get_device_name(0), 'frame': [800, 800], 'filters': 'adaptive', 'repeats': REPEATS, 'configs': {}}
    for c in (3, 1):
        for n in (1, 17):
            out['configs'][f'C{c}-N{n}'] = measure(c, n)
    out['note'] = ('batch_to_host is a host clock around one streams() call, which ends with the compressed bytes on the host; files the same '
                   'around encode() (+ CRC and framing on the calling thread); entry_events one HIP event pair around the C entry; kernels '
                   f'(where present) are rocprofv3 --kernel-trace --stats averages of a separate run of {WARMUP + CALLS} batches; '
                   'write_png is the host baseline per frame on one thread, in the same run on the same frames')
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
