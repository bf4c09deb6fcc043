"""Time the material selection and edit on two shapes: 640,000 rows (one 800 x 800 view, all foreground) and 2,048 rows.

  kernel  decomp/nerfactor/util/material_edit.select_apply: selection (codes, a roughness bound and a diff_scale bound), edit of the
          three materials and the opt_scale scaling in the single launch of csrc/material_edit.hip;
  torch   the statements that launch replaces inside fast_render, on the same device: the mask built by torch compares, then the six
          blend ops (src * (1 - m) + m * v per material), then the two scalings.

    python scripts/probe_material_edit.py [out.json]        -> profiles/material_edit.json unless told otherwise

Times are HIP events around CALLS back-to-back calls, divided by CALLS (one launch is shorter than an event pair resolves), medians of
REPEATS such windows after a warm-up, the two paths alternating.  `bytes_min` is what the launch must move at least (every input tensor
read once, every output written once); `bytes_requested` counts albedo and rough twice, as the kernel reads them for the selection and
again for the edit (the second read is served by the caches).  Needs an MI355X: there is no fallback."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.gpu_util import launches                                         # noqa: E402
from vqnerf_release_amd import _C                                           # noqa: E402
from vqnerf_release_amd.decomp.nerfactor.util import material_edit          # noqa: E402

CODES = (1, 2, 3, 5)
ROUGH = (0.2, 0.9)
DIFF_SCALE = ((0.1, 0.1), (5.0, 5.0))
DST = {'diff': [0.1, 0.07, 0.02], 'spec': [0.85, 0.7, 0.35], 'rough': [0.35]}
SCALE = [1.25, 0.8, 1.1]
CALLS, REPEATS, WARMUP = 20, 30, 3


def torch_statements(albedo, spec, rough, embed, scale_t, dst_t):
    """what fast_render would run without the kernel: compares -> float mask -> six blend ops -> two scalings"""
    member = (embed == CODES[0])
    for c in CODES[1:]:
        member = member | (embed == c)
    ds = albedo[:, :2] / (albedo[:, 2:3] + material_edit.EPS)
    lo, hi = dst_t['ds_lo'], dst_t['ds_hi']
    cond = ((rough > ROUGH[0]) & (rough < ROUGH[1])).all(-1) & ((ds > lo) & (ds < hi)).all(-1)
    m = (cond & member).to(torch.float32)[:, None]
    upd = lambda src, v: src * (1 - m) + m * v
    albedo, spec, rough = upd(albedo, dst_t['diff']), upd(spec, dst_t['spec']), upd(rough, dst_t['rough'])
    return m, albedo, spec, rough, albedo * scale_t, spec * scale_t


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'material_edit.json')
    assert torch.cuda.is_available(), 'needs cuda:0'
    dev = torch.device('cuda:0')
    sel = material_edit.Selection(CODES, [('rough',) + tuple([x] for x in ROUGH), ('diff_scale',) + DIFF_SCALE], ['and'])
    out = {'device': torch.cuda.get_device_name(0), 'rows_per_pass': _C.MATEDIT_ROWS_PER_PASS, 'grid_cap': _C.MATEDIT_GRID_CAP,
           'calls_per_window': CALLS, 'windows': REPEATS, 'shapes': {}}
    for n in (640000, 2048):
        g = torch.Generator(device=dev).manual_seed(n)
        albedo, spec = torch.rand(n, 3, device=dev, generator=g) * 0.98 + 0.02, torch.rand(n, 3, device=dev, generator=g)
        rough = torch.rand(n, 1, device=dev, generator=g)
        embed = torch.as_tensor(np.repeat(np.random.default_rng(n).integers(0, 9, n // 64 + 1), 64)[:n].astype(np.int32), device=dev)   # flat runs
        scale_t = torch.tensor([SCALE], device=dev)
        dst_t = {k: torch.tensor([v], device=dev) for k, v in DST.items()}
        dst_t['ds_lo'], dst_t['ds_hi'] = torch.tensor([DIFF_SCALE[0]], device=dev), torch.tensor([DIFF_SCALE[1]], device=dev)
        props = {'diff': albedo, 'rough': rough}
        kernel = lambda: material_edit.select_apply(props, sel, albedo, spec, rough, DST, embed=embed, opt_scale=SCALE)
        torch_fn = lambda: torch_statements(albedo, spec, rough, embed, scale_t, dst_t)
        with launches() as rec:
            res, got = kernel()
        want = torch_fn()
        equal = bool(torch.equal(res['mask'].to(torch.float32)[:, None], want[0]) and all(torch.equal(a, b) for a, b in zip(got, want[1:])))
        for _ in range(WARMUP):
            window(kernel), window(torch_fn)
        tk, tt = [], []
        for _ in range(REPEATS):                                 # alternating: a disturbance of the machine hits both
            tk.append(window(kernel))
            tt.append(window(torch_fn))
        _C.KernelClock.reset(True)                               # the entry alone: events around the zeroing of the counts row + the launch
        for _ in range(REPEATS):
            kernel()
            torch.cuda.synchronize()
        te = [a.elapsed_time(b) for a, b in _C.KernelClock.pairs['vqn_material_select_edit']]
        _C.KernelClock.reset(False)
        stat = lambda ts: {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}
        bytes_min = n * (12 + 12 + 4 + 4) + n * (12 + 12 + 4 + 12 + 12 + 1)
        k_ms = statistics.median(tk)
        out['shapes'][str(n)] = {
            'rows': n, 'selected': int(res['selected']), 'entry_calls': rec.counts, 'outputs_equal_torch': equal,
            'kernel_call': stat(tk), 'kernel_entry_events': stat(te), 'torch_statements': stat(tt), 'bytes_min': bytes_min, 'bytes_requested': bytes_min + n * 16,
            'kernel_call_bytes_per_s': bytes_min / (k_ms * 1e-3), 'kernel_entry_bytes_per_s': bytes_min / (statistics.median(te) * 1e-3),
            'kernel_faster_than_torch': k_ms < statistics.median(tt), 'torch_over_kernel': statistics.median(tt) / k_ms}
    out['note'] = ('kernel_call is the whole host call (validation, program packing, five output allocations, the zeroing of the counts row '
                   'and the launch) per call in a back-to-back window; kernel_entry_events is one HIP event pair around the entry alone (the zeroing '
                   'and the launch, the device otherwise idle), at the resolution of an event pair; each bytes/s is bytes_min over that time')
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
