"""Timing probe: vqn_vq_assign / vqn_vq_ema_stats at 1 M rows (HBM roofline rows K8 / K9).
`probe_vq.py --host [N]`: wall time per call of every VQ entry point at N rows (default 1), where the host side dominates."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vqnerf_release_amd import _C

def t_gpu(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3

def t_host(fn, n=2000):
    """wall time per call, microseconds: n calls back to back, one synchronisation at the end"""
    for _ in range(20): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6

if len(sys.argv) > 1 and sys.argv[1] == '--host':
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    lib, g = _C.lib(), torch.Generator(device='cuda')
    g.manual_seed(0)
    for D, K in ((256, 15), (256, 33), (256, 64), (20, 40)):
        x, C = torch.rand((N, D), device='cuda', generator=g), torch.rand((D, K), device='cuda', generator=g)
        idx = torch.empty((N,), dtype=torch.int64, device='cuda')
        q, dist, ste = torch.empty_like(x), torch.empty((N, K), device='cuda'), torch.empty_like(x)
        loss, counts, dw = torch.empty((), device='cuda'), torch.empty((K,), device='cuda'), torch.empty((D, K), device='cuda')
        ws = torch.empty((4096,), device='cuda')
        need = lib.vqn_vq_ema_stats_ws_bytes(N, D, K)
        ews = torch.empty((max(need, 4) // 4,), device='cuda')
        P, call = _C._ptr, _C._call                      # (the raw entry points: no allocation in the timed loop)
        legs = {
            'assign': lambda: call('vqn_vq_assign', P(x), N, D, P(C), K, None, None, P(idx), P(q), None),
            'assign+dist': lambda: call('vqn_vq_assign', P(x), N, D, P(C), K, None, None, P(idx), P(q), P(dist)),
            'quantize_rows': lambda: call('vqn_vq_quantize_rows', P(x), N, D, P(C), K, None, 1e-6, 1.0, P(ws), P(idx), P(ste), P(loss), P(counts)),
            'ema_stats': lambda: call('vqn_vq_ema_stats', P(x), P(idx), N, D, K, P(counts), P(dw), P(ews) if need else None, need),
            'counts': lambda: call('vqn_vq_ema_stats', None, P(idx), N, 4, K, P(counts), None, None, 0),
            'ste_loss': lambda: call('vqn_vq_ste_loss', P(x), P(q), N * D, 1.0, P(ste), P(loss), P(ws)),
            'l2_normalize_rows': lambda: call('vqn_l2_normalize_rows', P(x), N, D, 1e-6, P(q)),
        }
        legs['assign']()                                 # (valid indices for the statistics)
        for name, fn in legs.items():
            print(f'host N={N} D={D} K={K} {name}: {t_host(fn):.2f} us/call', flush=True)
    sys.exit(0)

N, D = (int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20), 256
g = torch.Generator(device='cuda'); g.manual_seed(0)
x = torch.rand((N, D), device='cuda', generator=g)
for K in (15, 32, 64):
    C = torch.rand((D, K), device='cuda', generator=g)
    idx, _, _ = _C.vq_assign(x, C, want_quant=False)
    ta = t_gpu(lambda: _C.vq_assign(x, C, want_quant=False))
    te = t_gpu(lambda: _C.vq_ema_stats(x, idx, K))
    ba = N * (4 * D + 8) + 4 * D * K
    be = N * (4 * D + 8) + 4 * K * (D + 1)
    print(f'K={K}: assign {ta*1e3:.3f} ms {ba/ta/1e9:.0f} GB/s   ema {te*1e3:.3f} ms {be/te/1e9:.0f} GB/s', flush=True)

# the fused quantiser (l2-normalise + assign + straight-through + commitment + counts) on encoder-like rows
z = torch.sigmoid(torch.randn((N, D), device='cuda', generator=g))
for K in (15, 32, 64):
    C = torch.rand((D, K), device='cuda', generator=g)
    C = C / C.norm(dim=0, keepdim=True)
    tq = t_gpu(lambda: _C.vq_quantize_rows(z, C))
    bq = N * (8 * D + 8) + 4 * D * K
    print(f'K={K}: quantize_rows {tq*1e3:.3f} ms {bq/tq/1e9:.0f} GB/s (variant {_C.vq_assign_variant(D, K)})', flush=True)
