#!/usr/bin/env python3
"""bench.py -- rays/sec of the NeuS ray-march hot path on MI355X (driver contract: one JSON line on rank 0).

Workload (BASELINE.json configs[1]): NeuSRenderer.render on the rays of a synthetic 800x800 view, full
nets (SDF 8x256 -> 257, colour 4x256), 64 coarse + 64 importance samples per ray (4 up-sampling steps),
fp32 end to end.  A "step" = one render() call over `--rays` rays already resident in HBM (default 640,000 = one whole
800x800 image per rank per step; rank r renders the view from its own camera, weak scaling).
Ranks shard views / rays with no data-path collective (gen_geo.py --num_p/--p_i is the reference's own scheme).

--mode train: the timed step is the data-parallel geo TRAINING step instead (2560 rays per rank, forward + backward + Adam,
one flat-bucket RCCL all-reduce of the gradients per step); `value` is then training rays/s.  With --full, a render-mode
multi-rank run also times that step and the reflectance (VQ) training step -- gradient bucket + codebook-statistics
all-reduce -- after the timed render region and reports them under "extra.dp_train" (all-reduce time per step included).

The stdout line is short (< 8 KB: numbers and identifiers only, `compact_line`); the full report -- notes, sample descriptions,
timing windows, per-kernel tables -- is the sidecar gpurun_out/bench_detail.json (`detail` on the line names it; $VQN_BENCH_DETAIL).
`python bench.py --gpus N` without WORLD_SIZE starts its N ranks itself as a child `python -m torch.distributed.run` (before any
GPU call) and exits with that child's code; if the data-parallel legs hang, every rank exits 3 after rank 0 printed the render line.

A plain run (no --full) does only what the headline needs: set-up, W warm-up steps, K timed steps, the outputs of the last timed
step if --dump-outputs DIR is given, and the line.  Everything else -- the live roofline.traffic passes, the CPU baselines and PSNR
checks, the other precisions, the secondary workloads under `extra`, the data-parallel legs and the sidecar -- runs with --full.
--dump-outputs DIR writes the arrays the timed step returns to its caller (render: the dict of NeuSRenderer.render; train: the
step's losses and the networks' parameters after it) as DIR/<name>.npy, float32 (float64 for float64 and integer outputs), at most
64 MB in all: beyond that every array with one row per ray is cut to the same fixed, seeded sample of rows.

Extra objects in the JSON line:
  roofline     -- dominant kernel (vqn_neus_fine_points): algorithmic FLOPs per launch / its average
                  launch duration measured with HIP events on the launch stream, vs the dense f32 MFMA peak
  cpu_baseline -- (--full) the faithful torch-CPU oracle (oracle/geo.py, a port of the reference op sequence) timed
                  on this host's cores over a bounded sample of the same workload (rank 0, N=1 only): B = 2560 rays spread
                  over the whole image, 1 warm-up + 3 timed calls, median
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

F32_MFMA_PEAK_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md: dense f32-input MFMA (= f32 vector peak)
BF16_MFMA_PEAK_TFLOPS = 2500.0   # same guide: dense bf16 MFMA.  The exact-split (x3) kernels spend SIX bf16 MFMAs per f32 product, so a kernel
                                 # doing A algorithmic TFLOP/s keeps the bf16 pipe 6 A / 2500 busy; both fractions are reported for them

# `bias` is the radius of the geometric-init sphere (fields.py:45-63; nerf.conf ships 0.5): 0.85 makes its silhouette cover
# ~29 % of the 800x800 view from (0, 0, 4), the "~30 % of rays hit" of SURVEY 8(d), so hit and miss compositing both count
FULL = dict(
    sdf=dict(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=(4,), multires=6, bias=0.85, scale=1.0,
             geometric_init=True, weight_norm=True),
    color=dict(d_feature=256, mode='idr', d_in=9, d_out=3, d_hidden=256, n_layers=4, weight_norm=True,
               multires_view=4, squeeze_out=True),
    renderer=dict(n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=1.0),
)


def image_rays(rows, H=800, W=800, fov=0.6911, cam_z=4.0, yaw=0.0):
    """Pin-hole camera at distance cam_z from the origin, looking at it ((0,0,4) looking down -z), turned by `yaw`
    about the y axis (each rank of a multi-GPU run renders its own view); returns o, d [len(rows)*W, 3]."""
    f = 0.5 * W / math.tan(0.5 * fov)
    j, i = np.meshgrid(np.asarray(rows, np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    d = np.stack([(i - 0.5 * W + 0.5) / f, -(j - 0.5 * H + 0.5) / f, -np.ones_like(i)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.array([[0.0, 0.0, cam_z]]), (d.shape[0], 1))
    if yaw != 0.0:
        c, s_ = math.cos(yaw), math.sin(yaw)
        R = np.array([[c, 0.0, s_], [0.0, 1.0, 0.0], [-s_, 0.0, c]])
        o, d = o @ R.T, d @ R.T
    return o.astype(np.float32), d.astype(np.float32)


def cpu_model_string():
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.lower().startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or 'unknown'


def macs_per_point(sdf, col):
    """MACs of one SDF forward and one colour forward, from the layer shapes."""
    m_sdf = 0
    for l in range(sdf.num_layers - 1):
        lin = getattr(sdf, f'lin{l}')
        m_sdf += lin.bias.numel() * (lin.weight_v.shape[1] if lin.weight_norm else lin.weight.shape[1])
    m_col = 0
    for l in range(col.num_layers - 1):
        lin = getattr(col, f'lin{l}')
        m_col += lin.bias.numel() * (lin.weight_v.shape[1] if lin.weight_norm else lin.weight.shape[1])
    return m_sdf, m_col


_T0 = time.perf_counter()


def _log(msg):
    """progress on stderr (stdout carries the ONE JSON line): a run that stays silent for minutes looks hung to its driver"""
    print(f'[bench {time.perf_counter() - _T0:7.1f} s] {msg}', file=sys.stderr, flush=True)


def _time_gpu(fn, n, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def _time_windows(fn, n, windows=3, warm=0, clock=False):
    """`windows` back-to-back windows of n calls each -> (median seconds per call, [ms per call of every window], kernel clock of the
    median window | None).  Every secondary leg reports the MEDIAN and lists all windows (round 3 reported the fastest)."""
    from vqnerf_release_amd import _C
    res = []
    for w in range(windows):
        if clock:
            _C.KernelClock.reset(True)
        dt = _time_gpu(fn, n, warm=warm if w == 0 else 0)
        res.append((dt, _C.KernelClock.summary() if clock else None))
    if clock:
        _C.KernelClock.reset(False)
    order = sorted(range(windows), key=lambda i: res[i][0])
    mid = order[(windows - 1) // 2]
    return res[mid][0], [r[0] * 1e3 for r in res], res[mid][1]


DECOMP_INI = dict(
    model='vq_nfr', data_type='nerf', white_bg='True', mlp_width=128, conv_width=256, pos_enc='True', n_freqs_xyz=10,
    n_freqs_ldir=4, n_freqs_vdir=4, light_h=16, light_init_val=0.5, num_embed=15, commitment_cost=0.1, vq_loss_weight=1.0,
    chr_alpha=60, chr_thres=0.1, combine_weight=0.2, mat_sloss_weight=0.05, chromaticity_loss_weight=1.0,
    sim_loss_weight=1e-4, lambert_weight=1e-3, random_seed=2, n_rays_per_step=1024, lr=5e-4)


def secondary_measurements(dev, sdf, col, var, ren, m_sdf, m_col):
    """The other workloads of the path, each a short timed loop on rank 0 (reported under "extra", never as `value`):
    geo training step, reflectance-model render / training step, standalone VQ assign + EMA statistics."""
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.nerfactor.util.io import config_from_dict
    from vqnerf_release_amd.decomp.nerfactor import train_nfr
    from vqnerf_release_amd.geo.nerf_runner import SyntheticDataset
    out = {}
    rng = np.random.default_rng(1)

    _log('leg: geo training step')
    # ---- geo training step: nerf.conf batch (2560 rays), L1 colour + 0.1 eikonal + 0.1 mask BCE, Adam ----
    B = 2560
    ds = SyntheticDataset(device=dev, n_images=8)
    params = list(sdf.parameters()) + list(var.parameters()) + list(col.parameters())
    opt = torch.optim.Adam(params, lr=5e-4)
    bg = torch.ones(1, 3, device=dev)

    def geo_train():
        data = ds.gen_random_rays_at(0, B)
        o, d, rgb, mask = data[:, :3].contiguous(), data[:, 3:6].contiguous(), data[:, 6:9], data[:, 9:10]
        near, far = ds.near_far_from_sphere(o, d)
        opt.zero_grad(set_to_none=True)
        r = ren.render(o, d, near, far, 2.0, background_rgb=bg, cos_anneal_ratio=1.0)
        loss = ((r['color_fine'] - rgb) * mask).abs().sum() / (mask.sum() + 1e-5) + 0.1 * r['gradient_error'] \
            + 0.1 * torch.nn.functional.binary_cross_entropy(r['weight_sum'].clip(1e-3, 1 - 1e-3), mask)
        loss.backward()
        opt.step()
    for _ in range(3):          # (the caching allocator settles on the step's workspaces over the first few steps)
        geo_train()
    # three windows of 6 steps: the median (all listed)
    dt, geo_windows, clk = _time_windows(geo_train, 6, windows=3, clock=True)
    S_c, S_f = 64 + 48, 128
    # algorithmic FLOPs of one step: coarse SDF passes + [fwd, reverse sweep, tangent, reverse, 2 weight
    # contractions] of the SDF net + [fwd, reverse, weight contraction] of the colour net, per fine sample
    flop = 2.0 * B * (S_c * m_sdf + S_f * (6 * m_sdf + 3 * m_col))
    # per kernel group: algorithmic FLOPs of what it computes (per fine sample: prog_fwd = SDF forward + reverse sweep + colour forward,
    # prog_sbwd = tangent pass + second reverse sweep, prog_cbwd = colour reverse sweep, wgrad = 2 SDF + 1 colour contraction; the coarse
    # passes are SDF forwards) over its HIP-event time, against the f32-input MFMA peak ("f32-equivalent" for the bf16x3 contraction)
    kflop = {'vqn_neus_sdf_points': 2.0 * B * S_c * m_sdf, 'vqn_neus_sdf_points_x3': 2.0 * B * S_c * m_sdf, 'vqn_tile_program:prog_fwd': 2.0 * B * S_f * (2 * m_sdf + m_col),
             'vqn_tile_program:prog_sbwd': 2.0 * B * S_f * 2 * m_sdf, 'vqn_tile_program:prog_cbwd': 2.0 * B * S_f * m_col,
             # (round 3: the full-size networks run the forward / backward on the two-image engine instead of the interpreted programs)
             'vqn_neus_train_fwd': 2.0 * B * S_f * (2 * m_sdf + m_col), 'vqn_neus_train_bwd': 2.0 * B * S_f * (2 * m_sdf + m_col),
             'vqn_neus_train_fwd_x3': 2.0 * B * S_f * (2 * m_sdf + m_col),       # (exact-split engine: f32-equivalent FLOPs over the f32 peak)
             'vqn_neus_train_bwd_x3': 2.0 * B * S_f * (2 * m_sdf + m_col),
             'vqn_wgrad_partials': 2.0 * B * S_f * (2 * m_sdf + m_col), 'vqn_wgrad_partials_x3': 2.0 * B * S_f * (2 * m_sdf + m_col)}
    kfrac = {k: {'ms': clk[k][1] / 6, 'tflops': kflop[k] / (clk[k][1] / 6 * 1e-3) / 1e12,
                 'frac_of_f32_mfma_peak': kflop[k] / (clk[k][1] / 6 * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS} for k in kflop if k in clk}
    for k, v in kfrac.items():               # exact-split kernels: the pipe they run on is the bf16 one, six MFMAs per product
        if k.endswith('_x3'):                # -> `frac` is the bf16-pipe fraction; the f32-equivalent one stays as the secondary key
            v['frac'] = v['frac_of_bf16_mfma_peak_at_6_mfma_per_product'] = 6.0 * v['tflops'] / BF16_MFMA_PEAK_TFLOPS
            v['bound'] = 'bf16 mfma (6 issued per f32 product)'
        else:
            v['frac'] = v['frac_of_f32_mfma_peak']
    out['geo_train'] = {'rays_per_s': B / dt, 'ms_per_step': dt * 1e3, 'windows_ms_per_step': geo_windows, 'batch_rays': B,
                        'achieved_tflops': flop / dt / 1e12, 'frac_of_f32_mfma_peak': flop / dt / 1e12 / F32_MFMA_PEAK_TFLOPS,
                        'kernel_ms_per_step': {k: v[1] / 6 for k, v in sorted(clk.items())}, 'kernel_roofline': kfrac,
                        'device_ms_outside_listed_kernels': dt * 1e3 - sum(v[1] / 6 for v in clk.values()),
                        'arithmetic': 'layer products of the up-sampling passes, the forward and the backward as exact bf16 piece triples (six bf16 '
                                      'MFMAs per f32 product, f32 accumulation: the *_x3 kernels, default since they pass the reference gradient '
                                      'goldens), the weight-gradient contraction likewise; frac_of_f32_mfma_peak = f32-equivalent FLOPs over the '
                                      'f32-input MFMA peak, as rounds 1-2 priced the f32 kernels; VQN_TRAIN_FWD/BWD=fused, VQN_TRAIN_COARSE=f32, '
                                      'VQN_WGRAD=f32 select the f32-input MFMA kernels',
                        'note': 'all HIP: up-sampling kernels, forward (vqn_neus_train_fwd_x3) and backward (vqn_neus_train_bwd_x3: colour '
                                'backward + tangent pass + reverse sweep, second-order eikonal term included) on the two-image engine, '
                                'weight-gradient contraction, compositing fwd/bwd; torch only for Adam (one launch under Runner(graph=True)), '
                                'the weight-norm chain rule and small reductions'}
    # the same step with the weight-gradient contraction on the f32-input MFMA (round 2's default; VQN_WGRAD=f32).  The default since
    # round 3 is the exact three-way bf16 split (csrc/wgrad_x3.hip: six bf16 MFMAs per product down to 2^-24), which passes the
    # reference-gradient goldens at the same 5e-3 bound.
    try:
        from vqnerf_release_amd.geo import train_programs as _tp
        wg_default = _tp.wgrad_mode()
        out['geo_train']['wgrad_mode'] = wg_default
        _tp.wgrad_mode('f32')
        geo_train()
        dt3, w3, clk3 = _time_windows(geo_train, 6, windows=3, clock=True)
        _tp.wgrad_mode(wg_default)
        out['geo_train_wgrad_f32'] = {'rays_per_s': B / dt3, 'ms_per_step': dt3 * 1e3, 'windows_ms_per_step': w3, 'achieved_tflops': flop / dt3 / 1e12,
                                      'frac_of_f32_mfma_peak': flop / dt3 / 1e12 / F32_MFMA_PEAK_TFLOPS,
                                      'wgrad_ms_per_step': clk3['vqn_wgrad_partials'][1] / 6,
                                      'note': 'the f32-input MFMA contraction (bit-for-bit a k-ordered fmaf chain), opt-in since round 3'}
    except Exception as e:                                      # noqa: BLE001
        out['geo_train_wgrad_f32'] = {'error': repr(e)[:300]}
    finally:
        _tp.wgrad_mode(os.environ.get('VQN_WGRAD', 'bf16x3'))

    _log('leg: the same training step through the Runner, captured once into a HIP gr')
    # ---- the same training step through the Runner, captured once into a HIP graph and replayed (Runner(graph=True)) ----
    try:
        g_runner, g_step = geo_train_setup(dev, 0, B, graph=True)
        for _ in range(g_runner.GRAPH_WARMUP + 2):
            g_step()
        dtg, wg, _ = _time_windows(g_step, 10, windows=3)
        out['geo_train_graph'] = {'rays_per_s': B / dtg, 'ms_per_step': dtg * 1e3, 'windows_ms_per_step': wg, 'batch_rays': B, 'captured': g_runner._cap is not None,
                                  'achieved_tflops': flop / dtg / 1e12, 'frac_of_f32_mfma_peak': flop / dtg / 1e12 / F32_MFMA_PEAK_TFLOPS,
                                  'note': 'geo_train with the whole optimisation step (up-sampling passes, forward / backward tile programs, '
                                          'compositing, weight-gradient contractions, weight-norm chain rule, capturable Adam) replayed from one '
                                          'captured HIP graph; bit-identical to the eager step (tests/test_gpu_train.py)'}
        del g_runner, g_step
    except Exception as e:                                      # noqa: BLE001
        out['geo_train_graph'] = {'error': repr(e)[:300]}

    _log('leg: the headline render on the split-precision kernels')
    # ---- the headline render on the split-precision kernels (renderer.matrix_mode = 'f16s'), opt-in mode ----
    Bq = 80000
    o_np, d_np = image_rays(np.arange(0, 800, 8))             # 100 rows spread over the view: hits and misses
    oq, dq = torch.tensor(o_np, device=dev), torch.tensor(d_np, device=dev)
    nq, fq = torch.full((Bq, 1), 2.0, device=dev), torch.full((Bq, 1), 6.0, device=dev)
    bgq = torch.ones(1, 3, device=dev)
    rend = lambda: ren.render(oq, dq, nq, fq, 2.0, perturb_overwrite=0, background_rgb=bgq, cos_anneal_ratio=1.0)
    flop_fine = 2.0 * (2 * m_sdf + m_col) * Bq * 128
    with torch.no_grad():
        ref_img = rend()['color_fine']

    def alt_mode_leg(mode, entry, issued_per_flop, peak, what):
        with torch.no_grad():
            ren.matrix_mode = mode
            try:
                got_img = rend()['color_fine']
                _C.KernelClock.reset(True)
                dtm = _time_gpu(rend, 3, warm=0)
                clkm = _C.KernelClock.summary()
            finally:
                ren.matrix_mode = 'f32'
                _C.KernelClock.reset(False)
        t_f = clkm[entry][1] / clkm[entry][0] * 1e-3
        mse = float(((got_img - ref_img) ** 2).mean())
        return {'rays_per_s': Bq / dtm, 'ms_per_step': dtm * 1e3, 'rays': Bq,
                'psnr_vs_f32_render_db': -10.0 * math.log10(mse + 1e-30), 'max_abs_diff_vs_f32': float((got_img - ref_img).abs().max()),
                'fine_kernel': {'ms': t_f * 1e3, 'achieved': flop_fine / t_f / 1e12, 'unit': 'TFLOP/s (algorithmic f32 FLOPs)',
                                'frac_of_f32_mfma_peak_equiv': flop_fine / t_f / 1e12 / F32_MFMA_PEAK_TFLOPS,
                                'issued_tflops': issued_per_flop * flop_fine / t_f / 1e12, 'peak': peak,
                                'frac': issued_per_flop * flop_fine / t_f / 1e12 / peak,
                                'frac_note': f'issued 16-bit MFMA FLOPs ({issued_per_flop:g} per algorithmic FLOP) over the dense 16-bit peak'},
                'kernel_ms_per_step': {k: v[1] / 3 for k, v in sorted(clkm.items())}, 'note': what}

    out['geo_render_f16s'] = alt_mode_leg('f16s', 'vqn_neus_fine_points_f16s', 3.0, 2516.6,
                                          'opt-in precision mode (renderer.matrix_mode = "f16s": f16 hi/lo operands, 3 f16 MFMAs per product, '
                                          'f32 accumulate; ~2^-21 per product, |w| < 6e4); `value` is the f32 path')
    # round 3: the exact-split engine (every f32 operand as three bf16 pieces, six bf16 MFMAs per product down to 2^-24, f32
    # accumulate): f32-level results with no operand-range caveat, held to the f32 kernels' tolerances against the reference goldens
    try:
        out['geo_render_x3'] = alt_mode_leg('x3', 'vqn_neus_fine_points_x3', 6.0, 2516.6,
                                            'exact-split mode (renderer.matrix_mode = "x3"): bf16x3 operands, 6 bf16 MFMAs per product, f32 '
                                            'accumulate; passes every reference-golden test at the f32 tolerances; since round 4 (activation pieces cut with '
                                            'round-to-nearest) its error against float64 is not above the f32 kernels\' (tests/test_gpu_neus_x3.py); '
                                            '`value` is the f32-input-MFMA path')
    except Exception as e:                                      # noqa: BLE001
        out['geo_render_x3'] = {'error': repr(e)[:300]}

    _log('leg: the literal "x64 samples" headline of the metric string')
    # ---- the literal "x64 samples" headline of the metric string: n_samples = 64, n_importance = 0 -- no
    # coarse pass at all (renderer.py:335), 169.0 MFLOP/ray -- one whole 800x800 view per step ----
    from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
    ren64 = NeuSRenderer(None, sdf, var, col, n_samples=64, n_importance=0, n_outside=0, up_sample_steps=4, perturb=1.0)
    B64 = 640000
    o64, d64 = [torch.tensor(a, device=dev) for a in image_rays(np.arange(800))]
    n64, f64 = torch.full((B64, 1), 2.0, device=dev), torch.full((B64, 1), 6.0, device=dev)
    rend64 = lambda: ren64.render(o64, d64, n64, f64, 2.0, perturb_overwrite=0, background_rgb=bgq, cos_anneal_ratio=1.0)
    with torch.no_grad():
        rend64()
        _C.KernelClock.reset(True)
        dt64 = _time_gpu(rend64, 3, warm=0)
        clk64 = _C.KernelClock.summary()
        _C.KernelClock.reset(False)
    t_fine64 = clk64['vqn_neus_fine_points'][1] / clk64['vqn_neus_fine_points'][0] * 1e-3
    flop64 = 2.0 * (2 * m_sdf + m_col) * B64 * 64
    out['geo_render_s64'] = {
        'rays_per_s': B64 / dt64, 'ms_per_step': dt64 * 1e3, 'rays': B64, 'mflop_per_ray': flop64 / B64 / 1e6,
        'fine_kernel': {'ms': t_fine64 * 1e3, 'achieved': flop64 / t_fine64 / 1e12, 'unit': 'TFLOP/s', 'peak': F32_MFMA_PEAK_TFLOPS,
                        'frac': flop64 / t_fine64 / 1e12 / F32_MFMA_PEAK_TFLOPS},
        'kernel_ms_per_step': {k: v[1] / 3 for k, v in sorted(clk64.items())},
        'note': 'n_samples = 64, n_importance = 0 (the "800x800x64 samples" of the metric string): no up-sampling pass, one fused '
                'SDF + gradient + colour launch over 64 section mid-points per ray; `value` is the shipped 64 + 64 configuration'}
    del o64, d64, n64, f64

    _log('leg: light-visibility extraction')
    # ---- light-visibility extraction (gen_geo.py compute_vis): secondary rays surface -> light, occupancy only ----
    from vqnerf_release_amd.geo.gen_geo import GeoExtractor
    ex = GeoExtractor(ren, max_radius=2.0, light_h=16, max_rays=1 << 20)
    npts = 4096
    u = torch.randn(npts, 3, device=dev)
    nrm = u / u.norm(dim=-1, keepdim=True)
    surf = 0.5 * nrm                                            # points on the 0.5-sphere the geometric init approximates
    msk = torch.ones(npts, 1, device=dev)
    with torch.no_grad():
        ex.compute_vis(surf[:256], nrm[:256], msk[:256], perturb_overwrite=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lv = ex.compute_vis(surf, nrm, msk, perturb_overwrite=0)
        torch.cuda.synchronize()
        dtv = time.perf_counter() - t0
    ren.matrix_mode = 'f16s'
    try:
        with torch.no_grad():
            ex.compute_vis(surf[:256], nrm[:256], msk[:256], perturb_overwrite=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lv16 = ex.compute_vis(surf, nrm, msk, perturb_overwrite=0)
            torch.cuda.synchronize()
            dtv16 = time.perf_counter() - t0
    finally:
        ren.matrix_mode = 'f32'
    n_sec = int((torch.einsum('ijk,ik->ij', torch.nn.functional.normalize(ex.lxyz.to(dev) - surf[:, None, :], dim=-1), nrm) > 0).sum())
    # per secondary ray: 64 coarse + 48 up-sampling SDF forwards, then 128 fine samples of SDF forward + reverse sweep (colour skipped)
    vis_flop = 2.0 * n_sec * (112 * m_sdf + 128 * 2 * m_sdf)
    out['compute_vis'] = {'secondary_rays_per_s': n_sec / dtv, 'surface_points': npts, 'secondary_rays': n_sec, 'ms': dtv * 1e3,
                          'roofline': {'bound': 'mfma', 'achieved': vis_flop / dtv / 1e12, 'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                                       'frac': vis_flop / dtv / 1e12 / F32_MFMA_PEAK_TFLOPS, 'mflop_per_secondary_ray': vis_flop / n_sec / 1e6,
                                       'note': 'whole call (wall clock incl. the host-side chunk loop), not one kernel'},
                          'secondary_rays_per_s_f16s': n_sec / dtv16, 'max_abs_diff_f16s_vs_f32': float((lv16 - lv).abs().max()),
                          'note': 'all front-lit (point, light) pairs of a chunk in one batch; colour network skipped (weights_only); '
                                  'the reference walks 512 lights one by one with a host sync each (gen_geo.py:202-242)'}

    _log('leg: reflectance model')
    # ---- reflectance model (vq_nfr): full-view inference and one training step ----
    model = get_model_class('vq_nfr')(config_from_dict(DECOMP_INI))
    model.build_nets(device=dev, seed=0).to(dev)
    cb = rng.uniform(0, 1, (15, 256)).astype(np.float32)
    model.set_codebook(cb / np.linalg.norm(cb, axis=1, keepdims=True))
    model.set_light(rng.uniform(0, 1, (16, 32, 3)).astype(np.float32))

    def points(n):
        xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        xyz /= np.linalg.norm(xyz, axis=1, keepdims=True)
        nrm = xyz + 0.1 * rng.normal(size=(n, 3)).astype(np.float32)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        T = lambda a: torch.tensor(a, device=dev)
        one = torch.ones(n, 1, device=dev)
        return (['v'] * 1, torch.zeros(n, 2, device=dev), T(np.tile(np.array([[0, 0, 4.0]], np.float32), (n, 1))),
                torch.zeros(n, 3, device=dev), T(rng.uniform(0, 1, (n, 3)).astype(np.float32)), one, one.clone(),
                T(xyz * rng.uniform(0.5, 1.0, (n, 1)).astype(np.float32)), T(nrm),
                (torch.rand(n, 512, device=dev) < 0.7).float())
    N = 640000
    big = points(N)
    with torch.no_grad():
        # mode 'test' = a render (no loss follows): the quantised rows stay on the chip.  mode 'vali' also writes them out for the
        # chromaticity-smoothness term of compute_loss (mat_sloss_weight > 0): reported beside it
        model.call(big, mode='vali')
        dt_vali = _time_gpu(lambda: model.call(big, mode='vali'), 3, warm=0)
        model.call(big, mode='test')
        _C.KernelClock.reset(True)
        dt = _time_gpu(lambda: model.call(big, mode='test'), 3, warm=0)
    clk = _C.KernelClock.summary()
    _C.KernelClock.reset(False)
    per = lambda k: clk[k][1] / clk[k][0] * 1e-3
    launches_per_call = {k: v[0] // 3 for k, v in clk.items()}
    SHADE_BYTES = 2048 + 36 + 56 + 60      # lvis row + xyz/normal/rayo + two (albedo, spec, rough) sets in; normal + 4 rgb outputs
    SHADE_FLOP_PER_POINT = 54165            # measured: profiles/r02_pmc_units.json (27.73 GFLOP per 512,000-point launch = 106 FLOP per point and light, both sets; valu_busy_frac 0.77)
    enc_macs, head_macs = model._enc_program().macs_per_point(), 296832 + 297600
    t_chain = sum(v[1] for k, v in clk.items() if k in ('vqn_mlp_chain_fwd', 'vqn_mlp_chain_vq_fwd')) / 3 * 1e-3      # (the fused launch carries the VQ step too)
    t_shade = per('vqn_brdf_shade_fwd')
    out['decomp_render'] = {
        'points_per_s': N / dt, 'ms_per_view': dt * 1e3, 'points': N, 'ms_per_view_vali_mode': dt_vali * 1e3,
        'mlp_chain': {'bound': 'mfma', 'achieved': 2.0 * (enc_macs + head_macs) * N / t_chain / 1e12,
                      'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                      'frac': 2.0 * (enc_macs + head_macs) * N / t_chain / 1e12 / F32_MFMA_PEAK_TFLOPS, 'ms': t_chain * 1e3},
        # both rooflines: the 2 KB visibility row per point against HBM, and the per-light arithmetic against the f32
        # vector pipe.  FLOPs per point are MEASURED (rocprofv3 SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F32 of this kernel on this
        # workload, profiles/r02_pmc_units.json: 27.73 GFLOP per 512,000-point launch); the same file has its vector-pipe
        # occupancy (valu_busy_frac 0.77) -- the kernel is vector-issue bound, not HBM bound
        'brdf_shade': {'bound': 'valu', 'ms': t_shade * 1e3, 'note': 'two material sets + diffuse/specular split per pass',
                       'hbm': {'achieved': N * SHADE_BYTES / t_shade / 1e9, 'peak': 8000.0, 'unit': 'GB/s',
                               'frac': N * SHADE_BYTES / t_shade / 1e9 / 8000.0, 'bytes_per_point': SHADE_BYTES},
                       'valu': {'achieved': N * SHADE_FLOP_PER_POINT / t_shade / 1e12, 'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                                'frac': N * SHADE_FLOP_PER_POINT / t_shade / 1e12 / F32_MFMA_PEAK_TFLOPS,
                                'flop_per_point': SHADE_FLOP_PER_POINT,
                                'peak_note': '157.3 TFLOP/s is the packed-FMA (v_pk_fma_f32) vector peak; scalar v_fma_f32 issue '
                                             'peaks at half of it, transcendentals (rsq / rcp / sqrt: 9 per light for the two '
                                             'material sets together, counted) at an eighth; counters: valu_busy_frac 0.77'}},
        'kernel_launches_per_call': launches_per_call}
    _log('leg: the same view on the split-precision MLP kernels')
    # ---- the same view on the split-precision MLP kernels (matrix_mode 'f16s': f16 hi/lo operands, 3 f16 MFMAs per product) ----
    with torch.no_grad():
        ref_pred = model.call(big, mode='vali')[0]
        model.matrix_mode = 'f16s'
        try:
            got_pred = model.call(big, mode='vali')[0]
            _C.KernelClock.reset(True)
            dt16 = _time_gpu(lambda: model.call(big, mode='vali'), 3, warm=0)
            clk16 = _C.KernelClock.summary()
        finally:
            model.matrix_mode = 'f32'
            _C.KernelClock.reset(False)
    t_chain16 = sum(v[1] for k, v in clk16.items() if k == 'vqn_mlp_chain_fwd_f16s') / 3 * 1e-3
    F16_MFMA_PEAK_TFLOPS = 2516.6
    eff = 2.0 * (enc_macs + head_macs) * N / t_chain16 / 1e12
    same_code = (got_pred['embed'] == ref_pred['embed']).float().mean()
    out['decomp_render_f16s'] = {
        'points_per_s': N / dt16, 'ms_per_view': dt16 * 1e3, 'points': N,
        'mlp_chain': {'bound': 'mfma', 'achieved': eff, 'unit': 'TFLOP/s (algorithmic f32 FLOPs)', 'ms': t_chain16 * 1e3,
                      'issued_f16_tflops': 3.0 * eff, 'peak': F16_MFMA_PEAK_TFLOPS, 'frac': 3.0 * eff / F16_MFMA_PEAK_TFLOPS,
                      'frac_note': 'issued f16 MFMA FLOPs (3 per algorithmic FLOP) over the dense f16 peak',
                      'speedup_vs_f32_kernel': t_chain / t_chain16},
        'max_abs_diff_vs_f32': {k: float((got_pred[k] - ref_pred[k]).abs().max()) for k in ('rgb', 'albedo', 'rough', 'vq_rgb')},
        'vq_idx_match_vs_f32_pct': 100.0 * float(same_code),
        'note': 'opt-in precision mode (model.matrix_mode = "f16s"); `value` and every other line are the f32 path'}
    _log('leg: the same view on the exact-split stack kernel')
    # ---- the same view with the MLP stacks on the exact-split kernel of the trainers (matrix_mode 'x3': bf16 piece triples, 6 bf16 MFMAs
    # per product, f32-level products with no operand-range caveat; csrc/refl_train_x3.hip with nothing kept for a backward) ----
    with torch.no_grad():
        model.matrix_mode = 'x3'
        try:
            got_x3 = model.call(big, mode='vali')[0]
            _C.KernelClock.reset(True)
            dtx3 = _time_gpu(lambda: model.call(big, mode='vali'), 3, warm=0)
            clkx3 = _C.KernelClock.summary()
        finally:
            model.matrix_mode = 'f32'
            _C.KernelClock.reset(False)
    t_chainx3 = sum(v[1] for k, v in clkx3.items() if k == 'vqn_refl_train_fwd_x3') / 3 * 1e-3
    effx3 = 2.0 * (enc_macs + head_macs) * N / max(t_chainx3, 1e-9) / 1e12
    out['decomp_render_x3'] = {
        'points_per_s': N / dtx3, 'ms_per_view': dtx3 * 1e3, 'points': N,
        'mlp_chain': {'bound': 'mfma', 'achieved': effx3, 'unit': 'TFLOP/s (algorithmic f32 FLOPs)', 'ms': t_chainx3 * 1e3,
                      'issued_bf16_tflops': 6.0 * effx3, 'peak': BF16_MFMA_PEAK_TFLOPS, 'frac': 6.0 * effx3 / BF16_MFMA_PEAK_TFLOPS,
                      'frac_note': 'issued bf16 MFMA FLOPs (6 per algorithmic FLOP) over the dense bf16 peak',
                      'f32_equivalent_frac': effx3 / F32_MFMA_PEAK_TFLOPS, 'speedup_vs_f32_kernel': t_chain / max(t_chainx3, 1e-9)},
        'max_abs_diff_vs_f32': {k: float((got_x3[k] - ref_pred[k]).abs().max()) for k in ('rgb', 'albedo', 'rough', 'vq_rgb')},
        'vq_idx_match_vs_f32_pct': 100.0 * float((got_x3['embed'] == ref_pred['embed']).float().mean()),
        'kernel_launches_per_call': {k: v[0] // 3 for k, v in clkx3.items()},
        'note': 'opt-in mode (model.matrix_mode = "x3"): encoder + main heads in one launch, quantiser, VQ heads in one launch, shading; '
                '`value` and every other line are the f32 path'}
    del got_x3
    _log('leg: BASELINE.json configs[4]')
    # ---- BASELINE.json configs[4]: relighting one view under 16 probes (test.py pd_relit pass), f32 and split-precision MLP stacks ----
    model.novel_probes = {f'probe{i:02d}': torch.tensor(rng.uniform(0, 2, (16, 32, 3)).astype(np.float32), device=dev) for i in range(16)}
    rel = {}
    with torch.no_grad():
        for mm in ('f32', 'f16s'):
            model.matrix_mode = mm
            try:
                pr = model.fast_render(big, mode='test', relight_probes=True)[0]
                rel[mm] = (_time_gpu(lambda: model.fast_render(big, mode='test', relight_probes=True), 3, warm=0), pr['rgb_probes'])
            finally:
                model.matrix_mode = 'f32'
    model.novel_probes = {}
    out['decomp_relight16'] = {
        'points': N, 'probes': 16, 'ms_per_view_f32': rel['f32'][0] * 1e3, 'ms_per_view_f16s': rel['f16s'][0] * 1e3,
        'relit_pixels_per_s_f32': 16 * N / rel['f32'][0], 'relit_pixels_per_s_f16s': 16 * N / rel['f16s'][0],
        'max_abs_diff_f16s_vs_f32': float((rel['f16s'][1] - rel['f32'][1]).abs().max()),
        'note': 'fast_render(relight_probes=True): encoder + main heads + ONE shading pass against all 16 probes (the reference loops '
                'over probes, vq_nfr.py:724-733); f16s = the fp16-MFMA path of BASELINE.json configs[4] (opt-in)'}
    del rel
    small = points(2048)
    model.get_codebook(); _ = model.light            # lazily created variables must exist before the optimiser is built
    # Keras Adam(amsgrad) as the reference builds it (train_nfr.py:121-139; epsilon outside the debiased root: optim.HipAdam(eps_mode='keras'))
    opt2, _, clip2 = train_nfr.make_optimizer(config_from_dict(DECOMP_INI), model.trainable_variables)
    tr = train_nfr.Trainer(model, opt2, clip=clip2)
    dt, w_small, _ = _time_windows(lambda: tr.train_iter(small, global_bs=1024), 5, windows=3, warm=2)
    TRAIN_FLOP_PER_POINT = 3 * 2.0 * (enc_macs + head_macs)      # forward + reverse sweep + weight-gradient contraction of every Dense layer
    tfrac = lambda n, t: {'achieved_tflops': TRAIN_FLOP_PER_POINT * n / t / 1e12, 'flop_per_point': TRAIN_FLOP_PER_POINT,
                          'frac_of_f32_mfma_peak': TRAIN_FLOP_PER_POINT * n / t / 1e12 / F32_MFMA_PEAK_TFLOPS,
                          # the pipe the step actually runs on: forward, backward and contraction as exact bf16 piece triples = six issued
                          # bf16 MFMAs per f32 product
                          'frac_of_bf16_mfma_peak_at_6_mfma_per_product': 6.0 * TRAIN_FLOP_PER_POINT * n / t / 1e12 / BF16_MFMA_PEAK_TFLOPS}
    train_note = ('all HIP: encoder + continuous heads and the VQ heads forward / backward on the dedicated exact-split kernels '
                  '(vqn_refl_train_fwd_x3 / _bwd_x3, round 4; the interpreted tile programs of rounds 1-3: VQN_REFL_TRAIN=prog), batched '
                  'weight-gradient contractions (bf16x3 on the matrix pipe, the 1..3-output last layers as a vector-ALU stream), fused shading '
                  'forward + backward, VQ assign / EMA statistics, loss terms, Keras-Adam as one launch; torch for the glue')
    out['decomp_train'] = {'points_per_s': 2048 / dt, 'ms_per_step': dt * 1e3, 'windows_ms_per_step': w_small, 'batch_points': 2048,
                           'roofline': tfrac(2048, dt), 'note': train_note + ' (eager: launch-latency-bound at the reference batch of 2048 points)'}
    big_tr = points(262144)
    # (the step is timed WITHOUT the per-kernel clock -- two HIP events around each of its ~100 launches cost the 14 ms step ~0.4 ms --
    #  and the kernel breakdown comes from one more, clocked window)
    dt, w_big, _ = _time_windows(lambda: tr.train_iter(big_tr, global_bs=262144), 3, windows=3, warm=1)
    _, _, clk_big = _time_windows(lambda: tr.train_iter(big_tr, global_bs=262144), 3, windows=1, clock=True)
    n_big = 262144
    kf = {'vqn_refl_train_fwd_x3': 2.0 * (enc_macs + head_macs) * n_big, 'vqn_refl_train_bwd_x3': 2.0 * (enc_macs + head_macs) * n_big,
          'vqn_wgrad_partials_x3': 2.0 * (enc_macs + head_macs) * n_big}
    kroof = {}
    for k, fl in kf.items():
        if k in clk_big:
            ms = clk_big[k][1] / 3
            kroof[k] = {'ms': ms, 'tflops_f32_equivalent': fl / (ms * 1e-3) / 1e12, 'bound': 'bf16 mfma (6 issued per f32 product)',
                        'frac': 6.0 * fl / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 'frac_of_f32_mfma_peak': fl / (ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS}
    out['decomp_train_256k'] = {'points_per_s': n_big / dt, 'ms_per_step': dt * 1e3, 'windows_ms_per_step': w_big, 'batch_points': n_big,
                                'roofline': tfrac(n_big, dt), 'kernel_ms_per_step': {k: v[1] / 3 for k, v in sorted(clk_big.items())},
                                'kernel_roofline': kroof,
                                'note': 'same step on a 128x larger batch (what a data-parallel / large-batch run would use); ' + train_note}
    # the same reference-size step captured once into a HIP graph and replayed (Trainer(graph=True)); last, as it switches
    # the model to its all-foreground statement
    opt3, _, clip3 = train_nfr.make_optimizer(config_from_dict(DECOMP_INI), model.trainable_variables, capturable=True)
    tr_g = train_nfr.Trainer(model, opt3, clip=clip3, graph=True)
    dt, w_graph, _ = _time_windows(lambda: tr_g.train_iter(small, global_bs=1024), 20, windows=3, warm=train_nfr.Trainer.GRAPH_WARMUP + 2)
    out['decomp_train_graph'] = {'points_per_s': 2048 / dt, 'ms_per_step': dt * 1e3, 'windows_ms_per_step': w_graph, 'batch_points': 2048,
                                 'roofline': tfrac(2048, dt), 'captured': tr_g._captured is not None,
                                 'note': 'decomp_train with the whole step (forward, loss, backward, EMA codebook move, Adam) '
                                         'replayed from one captured HIP graph; one 32-point image per workgroup and one workgroup row per head '
                                         '(64 point tiles x 3 heads on 256 CUs)'}

    _log('leg: stage-3 (ref_nfr) training step')
    # ---- stage 3 (ref_nfr): frozen stage-2 encoder + specular head on the inference kernels, rgb_enc + the two 512-wide heads on the exact-split
    # training kernels with a second head input (round 5; the interpreted tile programs before: VQN_REFL_TRAIN=prog) ----
    try:
        ini3 = dict(DECOMP_INI)
        ini3['model'] = 'ref_nfr'
        m3 = get_model_class('ref_nfr')(config_from_dict(ini3))
        m3.build_nets(device=dev, seed=0).to(dev)
        m3.set_light(rng.uniform(0, 1, (16, 32, 3)).astype(np.float32))
        for name in ('fine_enc', 'bottleneck', 'spec_out'):                # what load_stage2 does to the stage-2 parts
            for prm in m3.net[name].parameters():
                prm.requires_grad_(False)
        m3.register_trainable()
        _ = m3.light

        def ref_points(n):
            b = points(n)
            return b[:9] + (torch.rand(n, 3, device=dev),) + b[9:]
        res3 = {}
        for label, env in (('x3', {}), ('prog', {'VQN_REFL_TRAIN': 'prog'})):
            old_env = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                opt_s3, _, clip_s3 = train_nfr.make_optimizer(config_from_dict(ini3), m3.trainable_variables)
                tr3 = train_nfr.Trainer(m3, opt_s3, clip=clip_s3)
                for nb, reps in ((2048, 10), (262144, 3)):
                    b3 = ref_points(nb)
                    dt3, w3, _ = _time_windows(lambda: tr3.train_iter(b3, global_bs=nb // 2), reps, windows=3, warm=2)
                    res3[f'{label}_{nb}'] = {'ms_per_step': dt3 * 1e3, 'points_per_s': nb / dt3, 'windows_ms_per_step': w3}
                    del b3
            finally:
                for k, v in old_env.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        rgb_enc_macs = 3 * 256 + 2 * 256 * 256
        head3_macs = 2 * (512 * 256 + 256 * 128) + 640 * 3 + 640 * 1
        res3['trained_macs_per_point'] = rgb_enc_macs + head3_macs
        res3['speedup_262144_points'] = res3['prog_262144']['ms_per_step'] / res3['x3_262144']['ms_per_step']
        res3['note'] = ('train_nfr.Trainer.train_iter of the stage-3 model at the reference batch (2048 points) and a 128x larger one, eager; x3 = '
                        'the default (vqn_refl_train_fwd_x3_zx / _bwd_x3, frozen parts on vqn_mlp_chain_fwd), prog = the interpreted tile programs')
        out['ref_nfr_train'] = res3
        del m3
    except Exception as e:                                          # noqa: BLE001
        out['ref_nfr_train'] = {'error': repr(e)[:300]}

    _log('leg: standalone VQ nearest-code assignment + EMA statistics')
    # ---- standalone VQ nearest-code assignment + EMA statistics (HBM-bound) ----
    Nv, D, K = 1 << 20, 256, 15
    x = torch.rand(Nv, D, device=dev)
    x = x / x.norm(dim=1, keepdim=True)
    C = torch.tensor((cb / np.linalg.norm(cb, axis=1, keepdims=True)).T.copy(), device=dev)
    t_a = _time_gpu(lambda: _C.vq_assign(x, C, want_quant=False), 10)
    idx, _, _ = _C.vq_assign(x, C, want_quant=False)
    t_s = _time_gpu(lambda: _C.vq_ema_stats(x, idx, K), 10)
    by_a, by_s = Nv * (4 * D + 8) + 4 * D * K, Nv * (4 * D + 8) + 4 * K * (D + 1)
    out['vq_assign'] = {'rows': Nv, 'D': D, 'K': K, 'bound': 'hbm', 'achieved': by_a / t_a / 1e9, 'peak': 8000.0, 'unit': 'GB/s',
                        'frac': by_a / t_a / 1e9 / 8000.0, 'ms': t_a * 1e3, 'rows_per_s': Nv / t_a}
    out['vq_ema_stats'] = {'rows': Nv, 'bound': 'hbm', 'achieved': by_s / t_s / 1e9, 'peak': 8000.0, 'unit': 'GB/s',
                           'frac': by_s / t_s / 1e9 / 8000.0, 'ms': t_s * 1e3}

    _log('leg: BASELINE.json configs[2]')
    # ---- BASELINE.json configs[2]: the full decomposition with a 64-entry codebook (VERDICT r02 missing #2) ----
    K64 = 64
    cb64 = rng.uniform(0, 1, (K64, 256)).astype(np.float32)
    C64 = torch.tensor((cb64 / np.linalg.norm(cb64, axis=1, keepdims=True)).T.copy(), device=dev)
    t_a64 = _time_gpu(lambda: _C.vq_assign(x, C64, want_quant=False), 10)
    by_a64 = Nv * (4 * D + 8) + 4 * D * K64
    out['vq_assign_k64'] = {'rows': Nv, 'D': D, 'K': K64, 'bound': 'hbm', 'achieved': by_a64 / t_a64 / 1e9, 'peak': 8000.0, 'unit': 'GB/s',
                            'frac': by_a64 / t_a64 / 1e9 / 8000.0, 'ms': t_a64 * 1e3, 'rows_per_s': Nv / t_a64,
                            'kernel': 'vq_assign_split_kernel (f16-pair prefilter, exact re-evaluation of the candidates: bit-identical indices)'}
    # the same call on rows that lie NEAR codes (code + 5 % noise, normalised: what a trained encoder hands the quantiser).  The kernel's
    # cost depends on the data: a row whose two best codes are closer than the prefilter's error margin is re-evaluated exactly (f32 chain),
    # and the uniform positive rows above -- every row and code shares a large mean component, distances crowd together -- send most
    # 16-row groups there.  scripts/debug/vq_k64_paths.py: uniform rows 3.5 TB/s, gaussian rows 4.0, rows near codes 5.1.
    near = torch.nn.functional.normalize(C64.t()[torch.randint(0, K64, (Nv,), device=dev)] + 0.05 * torch.randn(Nv, D, device=dev), dim=1).contiguous()
    t_n64 = _time_gpu(lambda: _C.vq_assign(near, C64, want_quant=False), 10)
    out['vq_assign_k64']['rows_near_codes'] = {'achieved': by_a64 / t_n64 / 1e9, 'frac': by_a64 / t_n64 / 1e9 / 8000.0, 'ms': t_n64 * 1e3,
                                               'note': 'rows = code + 5 % noise, normalised; the headline of this entry keeps the uniform rows of rounds 1-2'}
    del near
    # SURVEY 8(d)'s rows: L2-normalised ENCODER outputs (the reflectance encoder on random surface points), the codebook cut from such
    # rows (what the k-means initialisation hands the VQ stage)
    with torch.no_grad():
        xyz_e = torch.nn.functional.normalize(torch.randn(Nv, 3, device=dev), dim=-1) * (0.5 + 0.5 * torch.rand(Nv, 1, device=dev))
        enc_rows = _C.l2_normalize_rows(model._pred_enc_at(xyz_e).contiguous())
        C_enc = enc_rows[torch.randperm(Nv, device=dev)[:K64]].t().contiguous()
    t_e64 = _time_gpu(lambda: _C.vq_assign(enc_rows, C_enc, want_quant=False), 10)
    out['vq_assign_k64']['rows_encoder_outputs'] = {'achieved': by_a64 / t_e64 / 1e9, 'frac': by_a64 / t_e64 / 1e9 / 8000.0, 'ms': t_e64 * 1e3,
                                                    'note': 'SURVEY 8(d) rows: l2-normalised outputs of the (random-init) encoder, codes = 64 of them'}
    del enc_rows, xyz_e
    xr = torch.rand(Nv, D, device=dev)                       # un-normalised rows: the fused quantiser normalises them itself
    from vqnerf_release_amd.decomp.nerfactor.networks.vq_layers import VectorQuantizerEMA
    vql = VectorQuantizerEMA(embedding_dim=D, num_embeddings=K64, commitment_cost=0.1, seed=0).to(dev)
    with torch.no_grad():
        vql.infer_from_raw(xr, C64)['quantize']
        t_q64 = _time_gpu(lambda: vql.infer_from_raw(xr, C64)['quantize'], 10)
    by_q64 = Nv * (8 * D + 8) + 4 * D * K64                  # rows in, straight-through rows out, index out
    out['vq_quantize_rows_k64'] = {'rows': Nv, 'D': D, 'K': K64, 'bound': 'hbm', 'achieved': by_q64 / t_q64 / 1e9, 'peak': 8000.0,
                                   'unit': 'GB/s', 'frac': by_q64 / t_q64 / 1e9 / 8000.0, 'ms': t_q64 * 1e3,
                                   'what': 'l2-normalise + nearest code + straight-through rows + commitment term + usage, one pass'}
    del x, xr
    ini64 = dict(DECOMP_INI)
    ini64['num_embed'] = K64
    model64 = get_model_class('vq_nfr')(config_from_dict(ini64))
    model64.build_nets(device=dev, seed=0).to(dev)
    model64.set_codebook(cb64 / np.linalg.norm(cb64, axis=1, keepdims=True))
    model64.set_light(rng.uniform(0, 1, (16, 32, 3)).astype(np.float32))
    view = list(points(N))
    alpha80 = (torch.rand(N, 1, device=dev) < 0.8).float()                    # 80 % foreground, like a test.py view (20-70 % background)
    n_fg = int(alpha80.sum())

    def call64():
        # a FRESH alpha tensor per call: the foreground-row cache (keyed on the tensor) misses, the `nonzero` + gather / scatter are paid
        view[5] = alpha80.clone()
        return model64.call(tuple(view), mode='test')
    with torch.no_grad():
        call64()
        _C.KernelClock.reset(True)
        dt64 = _time_gpu(call64, 3, warm=0)
    clk64 = _C.KernelClock.summary()
    _C.KernelClock.reset(False)
    t_front = sum(v[1] for k, v in clk64.items() if k in ('vqn_mlp_chain_fwd', 'vqn_mlp_chain_vq_fwd')) / 3 * 1e-3
    out['decomp_render_k64'] = {
        'rays': N, 'foreground_points': n_fg, 'ms_per_view': dt64 * 1e3, 'foreground_points_per_s': n_fg / dt64, 'K': K64,
        'mlp_chain': {'bound': 'mfma', 'achieved': 2.0 * (enc_macs + head_macs) * n_fg / t_front / 1e12, 'peak': F32_MFMA_PEAK_TFLOPS,
                      'unit': 'TFLOP/s', 'frac': 2.0 * (enc_macs + head_macs) * n_fg / t_front / 1e12 / F32_MFMA_PEAK_TFLOPS, 'ms': t_front * 1e3},
        'kernel_ms_per_view': {k: v[1] / 3 for k, v in sorted(clk64.items())},
        'kernel_launches_per_call': {k: v[0] // 3 for k, v in clk64.items()},
        'note': 'vq_nfr.call(mode="test") on an 800x800 view with 80 % foreground rays and a 64-entry codebook; every call gets a fresh '
                'alpha tensor, so the foreground `nonzero`, the row gathers and the scatters back to ray slots are inside the time'}
    del model64
    return out


def full_conf_text(batch_size=2560):
    """The `model` / `train` blocks of geo/confs/nerf.conf with the bench's network shapes (the Runner parses the same grammar)."""
    s, c, r = FULL['sdf'], FULL['color'], FULL['renderer']
    return f"""
general {{ base_exp_dir = /tmp/vqn_bench_exp/CASE_NAME }}
dataset {{ data_dir = /nonexistent/CASE_NAME, near = 2., far = 6., n_train = 8 }}
train {{
    learning_rate = 5e-4, learning_rate_alpha = 0.05, end_iter = 300000, batch_size = {batch_size}, validate_resolution_level = 1
    warm_up_end = 5000, anneal_end = 0, use_white_bkgd = True, save_freq = 100000000, val_freq = 0, val_mesh_freq = 0
    report_freq = 100000000, igr_weight = 0.1, mask_weight = 0.1
}}
model {{
    nerf {{ D = 8, d_in = 4, d_in_view = 3, W = 256, multires = 10, multires_view = 4, output_ch = 4, skips = [4], use_viewdirs = True }}
    sdf_network {{ d_out = {s['d_out']}, d_in = 3, d_hidden = {s['d_hidden']}, n_layers = {s['n_layers']}, skip_in = [{', '.join(map(str, s['skip_in']))}]
                  multires = {s['multires']}, bias = {s['bias']}, scale = {s['scale']}, geometric_init = True, weight_norm = True }}
    variance_network {{ init_val = 0.3 }}
    rendering_network {{ d_feature = {c['d_feature']}, mode = idr, d_in = 9, d_out = 3, d_hidden = {c['d_hidden']}, n_layers = {c['n_layers']}
                        weight_norm = True, multires_view = {c['multires_view']}, squeeze_out = True }}
    neus_renderer {{ n_samples = {r['n_samples']}, n_importance = {r['n_importance']}, n_outside = 0, up_sample_steps = {r['up_sample_steps']}, perturb = 1.0 }}
}}
"""


def _max_over_ranks(x, dev, world, backend):
    if world == 1:
        return x
    import torch.distributed as dist
    t = torch.tensor([x], device=dev if backend == 'nccl' else 'cpu', dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


WATCHDOG_EXIT = 3          # exit status of every rank when the data-parallel legs hang (bench.py's watchdog)
PRIME_LAUNCHES = 4600      # Round 3 primed the training legs past a one-off ~100 ms stall around a process's 4,100th clocked launch.  Its cause
                           # (round 4, scripts/debug/launch_stall.py): not launches -- 12,000 plain launches of either path show no stall --
                           # but live HIP EVENTS: the runtime extends its event pool with a stall of tens of ms (37 ms at the 2,400th live
                           # event), and _C.KernelClock kept two per clocked call alive.  The clock now pools its events (reserved up front
                           # in _timed_steps); the priming stays as a belt (allocator growth of the first steps).


def _timed_steps(fn, steps, warmup, dev, world, backend, prime=0):
    """W untimed + K timed calls bracketed by barrier + synchronize; returns (max-over-ranks seconds, kernel clock of the K calls).
    prime: extra untimed calls BEFORE the W warm-up calls, to carry a training process past its one-off launch-count stall."""
    from vqnerf_release_amd import _C
    _C.KernelClock.reserve(4096)                # the timed region creates no events (see PRIME_LAUNCHES)
    for _ in range(prime):
        fn()

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()
    for _ in range(warmup):
        fn()
    barrier()
    _C.KernelClock.reset(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    barrier()
    dt = time.perf_counter() - t0
    clock = _C.KernelClock.summary()
    _C.KernelClock.reset(False)
    return _max_over_ranks(dt, dev, world, backend), clock


def _collective_report(clock, steps):
    """Device time of the step's collectives (HIP events on the launch stream around each dist.all_reduce), per step."""
    rep = {k.split(':', 1)[1]: {'calls_per_step': v[0] / steps, 'us_per_step': v[1] / steps * 1e3}
           for k, v in sorted(clock.items()) if k.startswith('all_reduce:')}
    rep['total_us_per_step'] = sum(v['us_per_step'] for v in rep.values())
    return rep


def geo_train_setup(dev, rank, batch_rays=2560, graph=False):
    """The geo trainer (geo/nerf_runner.py `Runner`: nerf.conf batch of 2560 rays per rank, L1 colour + 0.1 eikonal + 0.1 mask
    BCE, Adam, cosine schedule; forward / backward on the HIP tile programs; under N ranks one flat-bucket all-reduce of the
    gradients + one 2-float all-reduce of the loss normalisers per step).  Every rank draws its own pixels."""
    from vqnerf_release_amd.geo.nerf_runner import Runner, SyntheticDataset
    torch.manual_seed(0)                                        # identical initial weights on every rank
    runner = Runner(conf_text=full_conf_text(batch_rays), case='bench', dataset=SyntheticDataset(device=dev, n_images=8, seed=rank),
                    device=dev, graph=graph)
    runner.update_learning_rate()
    it = [0]

    def step():
        data = runner.dataset.gen_random_rays_at(it[0] % 8, batch_rays)
        it[0] += 1
        return runner.train_step(data)
    return runner, step


def decomp_train_setup(dev, rank, world, batch_points=2048, graph=False, capturable=False):
    """The VQ-stage trainer (train_nfr.Trainer: n_rays_per_step = 1024 pixel pairs = 2048 surface points per rank, Keras-Adam with
    amsgrad; under N ranks the [counts || dw] codebook statistics are summed in the middle of the forward pass and the gradient
    bucket after the backward pass, the loss normaliser is the global batch)."""
    from vqnerf_release_amd.decomp.nerfactor import train_nfr
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.nerfactor.util.io import config_from_dict
    rng = np.random.default_rng(1)
    model = get_model_class('vq_nfr')(config_from_dict(DECOMP_INI))
    model.build_nets(device=dev, seed=0).to(dev)
    cb = rng.uniform(0, 1, (15, 256)).astype(np.float32)
    model.set_codebook(cb / np.linalg.norm(cb, axis=1, keepdims=True))
    model.set_light(rng.uniform(0, 1, (16, 32, 3)).astype(np.float32))
    model.get_codebook(); _ = model.light
    if graph:
        opt, _, clip = train_nfr.make_optimizer(config_from_dict(DECOMP_INI), model.trainable_variables, capturable=True)
        tr = train_nfr.Trainer(model, opt, clip=clip, graph=True)
    else:
        opt, _, clip = train_nfr.make_optimizer(config_from_dict(DECOMP_INI), model.trainable_variables, capturable=capturable)
        tr = train_nfr.Trainer(model, opt, clip=clip)
    batch = synthetic_points(batch_points, dev, np.random.default_rng(100 + rank))      # this rank's points
    return model, tr, (lambda: tr.train_iter(batch, global_bs=(batch_points // 2) * world))


def synthetic_points(n, dev, rng):
    """SURVEY 8(d) surface points as the 10-tuple view batch of datasets/shape_unit.py:109-110 (data_type nerf)."""
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    xyz /= np.linalg.norm(xyz, axis=1, keepdims=True)
    nrm = xyz + 0.1 * rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    T = lambda a: torch.tensor(a, device=dev)
    one = torch.ones(n, 1, device=dev)
    lvis = T((rng.uniform(size=(n, 512)) < 0.7).astype(np.float32))
    return (['v'] * 1, torch.zeros(n, 2, device=dev), T(np.tile(np.array([[0, 0, 4.0]], np.float32), (n, 1))),
            torch.zeros(n, 3, device=dev), T(rng.uniform(0, 1, (n, 3)).astype(np.float32)), one, one.clone(),
            T(xyz * rng.uniform(0.5, 1.0, (n, 1)).astype(np.float32)), T(nrm), lvis)


def dp_graph_selfcheck(dev, rank, world, backend, steps=2):
    """Eager data-parallel reflectance steps against the graph-segment replay of the same steps (train_nfr.Trainer(graph=True) under
    N ranks: parallel.SegmentedCapture), from the same state, on this run's ranks and backend: GRAPH_WARMUP eager steps (both trainers
    take them eagerly), the capturing step, then `steps` replays -- parameters, codebook and EMA state compared bit for bit on every
    rank, the verdict reduced over ranks (MIN).  Never raises: an exception is part of the report."""
    import torch.distributed as dist
    rep = {'steps_compared': None, 'bit_identical': False}
    try:
        from vqnerf_release_amd.decomp.nerfactor import train_nfr
        n_calls = train_nfr.Trainer.GRAPH_WARMUP + 1 + steps
        m_e, tr_e, step_e = decomp_train_setup(dev, rank, world, graph=False, capturable=True)
        for _ in range(n_calls):
            step_e()
        m_g, tr_g, step_g = decomp_train_setup(dev, rank, world, graph=True)
        for _ in range(n_calls):
            step_g()
        torch.cuda.synchronize()
        same = tr_g._captured is not None
        worst = 0.0
        for a, b in zip([m_e._codebook] + list(m_e.trainable_variables) + [m_e.vq_layer.ema_dw.hidden, m_e.vq_layer.ema_cluster_size.hidden],
                        [m_g._codebook] + list(m_g.trainable_variables) + [m_g.vq_layer.ema_dw.hidden, m_g.vq_layer.ema_cluster_size.hidden]):
            if not torch.equal(a.detach(), b.detach()):
                same = False
                worst = max(worst, float((a.detach() - b.detach()).abs().max()))
        flag = torch.tensor([1.0 if same else 0.0], device=dev if backend == 'nccl' else 'cpu')
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        rep.update(steps_compared=n_calls, bit_identical=bool(flag.item() == 1.0), captured=tr_g._captured is not None,
                   graph_segments=len(tr_g._captured.graphs) if tr_g._captured is not None else 0, max_abs_diff_this_rank=worst)
        del m_e, tr_e, step_e, m_g, tr_g, step_g
    except Exception as e:                                      # noqa: BLE001
        rep['error'] = repr(e)[:300]
        try:                                                    # keep the ranks' collective sequences aligned
            flag = torch.tensor([0.0], device=dev if backend == 'nccl' else 'cpu')
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        except Exception:                                       # noqa: BLE001
            pass
    return rep


def dp_train_leg(dev, rank, world, backend, steps=10, warmup=3):
    """Both data-parallel training steps at the reference batch sizes, K timed steps each (max over ranks), with the device time
    of every collective.  All ranks call this; the dict is meaningful on rank 0."""
    import torch.distributed as dist
    out = {'n_ranks_seen': dist.get_world_size() if (world > 1 and dist.is_initialized()) else 1, 'backend': backend if world > 1 else None}
    runner, gstep = geo_train_setup(dev, rank)
    dt, clk = _timed_steps(gstep, steps, warmup, dev, world, backend)
    out['geo'] = {'rays_per_s': 2560 * world * steps / dt, 'ms_per_step': dt / steps * 1e3, 'batch_rays_per_rank': 2560,
                  'grad_bucket_bytes': int(runner.bucket.flat.numel() * 4), 'all_reduce': _collective_report(clk, steps),
                  'last_train_backend': runner.renderer.last_train_backend}
    del runner, gstep
    model, tr, dstep = decomp_train_setup(dev, rank, world)
    dt, clk = _timed_steps(dstep, steps, warmup, dev, world, backend)
    out['decomp'] = {'points_per_s': 2048 * world * steps / dt, 'ms_per_step': dt / steps * 1e3, 'batch_points_per_rank': 2048,
                     'grad_bucket_bytes': int(tr.bucket.flat.numel() * 4), 'vq_stats_bytes': int((256 + 1) * 15 * 4),
                     'all_reduce': _collective_report(clk, steps)}
    if world > 1:
        from vqnerf_release_amd import parallel
        parallel.assert_replicas_identical([model._codebook] + list(model.trainable_variables), 'decomp replicas')
        out['decomp']['replicas_bit_identical_after_steps'] = True
    del model, tr, dstep
    # the same step replayed from HIP graphs: under N ranks three graphs with the two all-reduces between them
    # (parallel.SegmentedCapture).  Multi-rank RCCL: the run validates that path ITSELF before timing it -- the eager DP trainer and the
    # graph-segment trainer step the same model from the same state on the same batches (same capturable Keras-Adam kernel on both
    # sides), and every rank's parameters + codebook must agree bit for bit afterwards; only then are the graph legs timed, otherwise the
    # line reports why not (the eager legs above are the fallback, the exit code stays 0).  VQN_BENCH_DP_GRAPH=0 skips the graph legs.
    if world > 1 and backend != 'gloo' and os.environ.get('VQN_BENCH_DP_GRAPH') == '0':
        out['dp_graph_selfcheck'] = {'skipped': 'VQN_BENCH_DP_GRAPH=0'}
        return out
    if world > 1:
        out['dp_graph_selfcheck'] = dp_graph_selfcheck(dev, rank, world, backend)
        if not out['dp_graph_selfcheck'].get('bit_identical'):
            out['decomp_graph'] = {'skipped': 'dp_graph_selfcheck did not pass: eager data-parallel legs only'}
            return out
    try:
        model, tr, gstep2 = decomp_train_setup(dev, rank, world, graph=True)
        from vqnerf_release_amd.decomp.nerfactor import train_nfr
        dt, clk = _timed_steps(gstep2, steps, train_nfr.Trainer.GRAPH_WARMUP + 2, dev, world, backend)
        out['decomp_graph'] = {'points_per_s': 2048 * world * steps / dt, 'ms_per_step': dt / steps * 1e3,
                               'graph_segments': len(tr._captured.graphs) if tr._captured is not None else 0,
                               'all_reduce': _collective_report(clk, steps)}
    except Exception as e:                                      # noqa: BLE001
        out['decomp_graph'] = {'error': repr(e)[:300]}
    try:
        del model, tr, gstep2
    except Exception:                                           # noqa: BLE001
        pass
    # the geo step the same way (Runner(graph=True): under N ranks three graph segments around the loss-normaliser and gradient-bucket
    # all-reduces; tests/test_gpu_parallel.py: bit-identical to the eager DP step on two gloo ranks)
    try:
        runner, gstep3 = geo_train_setup(dev, rank, graph=True)
        dt, clk = _timed_steps(gstep3, steps, runner.GRAPH_WARMUP + 2, dev, world, backend)
        out['geo_graph'] = {'rays_per_s': 2560 * world * steps / dt, 'ms_per_step': dt / steps * 1e3,
                            'graph_segments': len(runner._cap.graphs) if runner._cap is not None else 0,
                            'all_reduce': _collective_report(clk, steps)}
    except Exception as e:                                      # noqa: BLE001
        out['geo_graph'] = {'error': repr(e)[:300]}
    return out


def decomp_cpu_leg(dev, cores, N=16384):
    """CPU-baseline leg of the reflectance model (R_dec,render next to its CPU figure, PSNR(build, oracle) on rgb and
    albedo, VQ index match %): one vali-mode call of vq_nfr.Model on N synthetic surface points, the oracle (oracle/decomp.py,
    test infrastructure) on the same points and weights on the host cores."""
    from oracle import decomp as od
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.nerfactor.util.io import config_from_dict
    p, specs = od.make_model_params(seed=0, K=15)
    model = get_model_class('vq_nfr')(config_from_dict(DECOMP_INI))
    model.build_nets(device=dev, seed=0)
    with torch.no_grad():
        for name, net in model.net.items():
            for layer, (W, b) in zip(net.layers, p[name]):
                layer.kernel.copy_(torch.as_tensor(np.asarray(W)))
                layer.bias.copy_(torch.as_tensor(np.asarray(b)))
    model.to(dev)
    model.set_codebook(np.asarray(p['codebook_raw']).T)
    model.set_light(np.asarray(p['light']))
    pts = od.make_points(N, seed=3)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)
    one = torch.ones(N, 1, device=dev)
    batch = (['v'], torch.zeros(N, 2, device=dev), T(pts['rayo']), torch.zeros(N, 3, device=dev), T(pts['rgb']), one, one.clone(),
             T(pts['xyz']), T(pts['normal']), T(pts['lvis']))
    with torch.no_grad():
        model.call(batch, mode='vali')
        gdt = _time_gpu(lambda: model.call(batch, mode='vali'), 5)
        pred, _, lk, _ = model.call(batch, mode='vali')
    pt = {k: ([(od.T(W), od.T(b)) for W, b in v] if isinstance(v, list) else od.T(v)) for k, v in p.items()}
    lxyz, lareas = od.gen_light_xyz(16, 32)
    lxyz, lareas = od.T(lxyz.reshape(-1, 3)), od.T(lareas.reshape(-1))
    ob = {k: od.T(v) for k, v in pts.items()}
    torch.set_num_threads(cores)
    with torch.no_grad():
        od.model_call(pt, specs, {k: v[:256] for k, v in ob.items()}, lxyz, lareas, od.EMA(0.999, (15,)), od.EMA(0.999, (256, 15)), mode='vali')
        t0 = time.perf_counter()
        want = od.model_call(pt, specs, ob, lxyz, lareas, od.EMA(0.999, (15,)), od.EMA(0.999, (256, 15)), mode='vali')
        cdt = time.perf_counter() - t0
    psnr = lambda a, b: -10.0 * math.log10(float(((a.cpu() - b) ** 2).mean()) + 1e-20)
    # nearest-code indices must agree wherever the fp64 top-2 distance gap is not a rounding tie
    d64 = od.vq_distances(want['z_norm'].double(), want['codebook'].double())
    top2 = torch.topk(-d64, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-6
    same = pred['embed'][:, 0].cpu() == want['embed']
    return {'value': N / cdt, 'unit': 'points/s', 'cores': cores, 'kind': 'port',
            'sample': f'{N} surface points (512 lights, visibility rows), one oracle.decomp.model_call(vali), {cdt:.1f} s',
            'gpu_points_per_s_same_sample': N / gdt, 'psnr_rgb_vs_oracle_db': psnr(lk['rgb'], want['rgb']),
            'psnr_albedo_vs_oracle_db': psnr(pred['albedo'], want['albedo']),
            'vq_idx_match_pct': 100.0 * float(same[clear].float().mean()), 'vq_idx_match_pct_all_rows': 100.0 * float(same.float().mean()),
            'near_tie_fraction': 1.0 - float(clear.float().mean())}


# the fine render kernel as rocprofv3 names it (spaces removed): template arguments <FINE, TRAIN>
FINE_KERNEL = 'neus_points2_kernel<true,false>'


def pmc_values(root, counter, kernel_substr):
    """Counter values of every dispatch of a kernel from the `*counter_collection.csv` files rocprofv3 --pmc leaves under `root`."""
    import csv
    import glob
    got = []
    for fn in glob.glob(os.path.join(root, '**', '*counter_collection.csv'), recursive=True):
        with open(fn) as fh:
            for r in csv.DictReader(fh):
                if kernel_substr in r.get('Kernel_Name', '').replace(' ', '') and r.get('Counter_Name') == counter:
                    got.append(float(r['Counter_Value']))
    return got


def live_traffic(rays, timeout_s=170):
    """Fabric-side bytes of ONE fine-kernel launch of the headline step, measured now: two child runs of this script (one 640,000-ray
    render each, no extras) under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` -- separate passes, kernel trace
    only, the program itself after `--` -- exactly scripts/pmc_traffic.sh.  Called BEFORE this process touches the GPU (the children
    are ordinary child processes).  Corrections of MI355X_MICROARCH.md (HBM section): counter values are KB; FETCH_SIZE reports half
    the bytes of 16-B-per-lane coalesced reads on gfx950 (x2), WRITE_SIZE is exact; both count fabric requests, Infinity-Cache hits
    included.  Returns (bytes per launch, note) or (None, reason)."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which('rocprofv3') is None:
        return None, 'rocprofv3 not on PATH'
    if any(k.startswith(('ROCPROF', 'ROCP_')) for k in os.environ) or 'rocprof' in os.environ.get('LD_PRELOAD', ''):
        return None, 'this run is itself under a profiler: no nested rocprofv3 passes'
    vals = {}
    for c in ('FETCH_SIZE', 'WRITE_SIZE'):
        d = tempfile.mkdtemp(prefix='vqn_pmc_', dir='/tmp')
        cmd = ['rocprofv3', '--kernel-trace', '--pmc', c, '--output-format', 'csv', '-d', d, '-o', 'c', '--', sys.executable,
               os.path.abspath(__file__), '--no-cpu-baseline', '--no-extras', '--no-traffic', '--no-detail', '--steps', '1', '--warmup', '0', '--rays', str(rays)]
        try:
            subprocess.run(cmd, timeout=timeout_s, env={**os.environ, 'TMPDIR': '/tmp'}, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           check=True, cwd='/tmp')
            got = pmc_values(d, c, FINE_KERNEL)
            if not got:
                return None, f'no {c} rows for the fine kernel in the rocprofv3 output'
            vals[c] = sum(got) / len(got)
        except Exception as e:                                  # noqa: BLE001
            return None, f'rocprofv3 --pmc {c} pass failed: {repr(e)[:160]}'
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return (2.0 * vals['FETCH_SIZE'] + vals['WRITE_SIZE']) * 1024.0, (
        'measured by THIS run: two child passes of this command under rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE '
        f'(mean over the fine-kernel launches of one {rays}-ray render each): 2*FETCH_SIZE + WRITE_SIZE (KB, gfx950 corrections of '
        'MI355X_MICROARCH.md); counts fabric requests incl. Infinity-Cache hits: the per-workgroup activation stash of the reverse sweep '
        '(8 x 32 KB per tile, written once and read once with streaming accesses) is ~all of it; algorithmic bytes are 32 B in + 28 B out '
        'per sample.  A 4x / 8x larger stash footprint (beyond the 256 MiB Infinity Cache) leaves the kernel time unchanged '
        '(DESIGN.md, round 3): the stream is not what bounds the kernel')


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays, rows, seed=0, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: each array of `arrays` as dirname/<name>.npy, float32 (float64 for float64 and integer outputs; None entries are
    skipped).  If the set would exceed `limit` bytes, every array whose leading dimension is `rows` keeps the same fixed, seeded, sorted
    sample of its rows -- as many as fit -- and the others are written whole.  Returns the names written."""
    def host_dtype(t):
        return torch.float64 if t.dtype == torch.float64 or not (t.is_floating_point() or t.dtype == torch.bool) else torch.float32
    ts = {k: (v.detach() if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in arrays.items() if v is not None}
    size = lambda t: t.numel() * host_dtype(t).itemsize
    per_row = {k: t for k, t in ts.items() if rows and t.dim() >= 1 and t.shape[0] == rows}
    fixed = sum(size(t) for k, t in ts.items() if k not in per_row)
    row_bytes = sum(size(t) for t in per_row.values()) // rows if per_row else 0
    sel = None
    if fixed + row_bytes * (rows or 0) > limit:
        n = (limit - fixed) // row_bytes if row_bytes else 0
        assert n >= 1, f'--dump-outputs: {fixed} bytes of outputs cannot be cut to {limit}'
        sel = np.sort(np.random.default_rng(seed).choice(rows, n, replace=False))
    os.makedirs(dirname, exist_ok=True)
    for k, t in ts.items():
        if sel is not None and k in per_row:
            t = t[torch.as_tensor(sel, device=t.device)]
        np.save(os.path.join(dirname, f'{k}.npy'), t.to(host_dtype(t)).cpu().numpy())
    return list(ts)


# ---- the ONE stdout line (driver contract) and its sidecar ----------------------------------------------------------------------------
# The line carries numbers and short identifiers only and stays under LINE_LIMIT bytes (round 4's 22 KB line was not captured by the
# driver); every note, sample description, window list and per-kernel table goes to the sidecar file `bench_detail.json`.
LINE_LIMIT = 8192
_PROSE_KEYS = frozenset(('note', 'traffic_note', 'sample', 'what', 'frac_note', 'peak_note', 'arithmetic', 'traceback', 'calls', 'kernel',
                         'flop_per_launch', 'macs_per_point'))
_TABLE_KEYS = frozenset(('kernel_ms_per_step', 'kernel_ms_per_view', 'kernel_roofline', 'kernel_launches_per_call', 'windows_ms_per_step',
                         'psnr_sample', 'wider', 'hbm', 'valu'))
# constants of a leg that the sidecar (and bench.py itself) state: not repeated on the line's `extra`
_EXTRA_CONST_KEYS = frozenset(('peak', 'unit', 'bound', 'flop_per_point', 'rows', 'D', 'points', 'batch_points', 'batch_rays', 'batch_rays_per_rank',
                               'batch_points_per_rank', 'surface_points', 'secondary_rays', 'mflop_per_ray', 'mflop_per_secondary_ray',
                               'issued_tflops', 'issued_f16_tflops', 'issued_bf16_tflops', 'frac_of_f32_mfma_peak_equiv'))
# legs of `extra` in the order they are given up if the line is still too long (least important first)
_DROP_ORDER = ('geo_train_wgrad_f32', 'decomp_render_f16s', 'geo_render_f16s', 'vq_ema_stats', 'vq_quantize_rows_k64', 'decomp_relight16',
               'compute_vis', 'geo_render_s64', 'decomp_render_x3', 'geo_render_x3', 'decomp_render_k64', 'decomp_train_256k', 'decomp_render',
               'vq_assign', 'vq_assign_k64', 'ref_nfr_train', 'decomp_train', 'geo_train', 'decomp_train_graph', 'geo_train_graph', 'dp_train')


def _sig(x, n=5):
    """floats to n significant digits (the line is a report, not a checkpoint)"""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float('inf'), float('-inf')):
        return None
    return float(f'{x:.{n}g}')


def _compact(obj, depth=0, max_str=48, drop=frozenset()):
    """numeric / boolean leaves and short identifier strings of a report dict; prose, tables and lists are left to the sidecar"""
    if isinstance(obj, dict):
        out = {}
        for k, v in obj.items():
            if k in _PROSE_KEYS or k in _TABLE_KEYS or k in drop:
                continue
            if k == 'error' and isinstance(v, str):
                out[k] = v[:96]
                continue
            c = _compact(v, depth + 1, max_str, drop)
            if c is not None and c != {}:
                out[k] = c
        return out
    if isinstance(obj, (list, tuple)):
        return None
    if isinstance(obj, str):
        return obj if len(obj) <= max_str else None
    if isinstance(obj, (bool, int)) or obj is None:
        return obj
    if isinstance(obj, float):
        return _sig(obj)
    try:
        return _sig(float(obj))
    except Exception:                                           # noqa: BLE001
        return None


def _first_sentence(s, limit=160):
    """a string cut at a word boundary to at most `limit` characters"""
    s = ' '.join(str(s).split())
    return s if len(s) <= limit else s[:limit].rsplit(' ', 1)[0]


def compact_line(result, limit=LINE_LIMIT, detail_path=None):
    """The stdout line of a full result dict: contract keys + `roofline` + `cpu_baseline` verbatim in meaning (numbers rounded to 5
    significant digits, strings cut to identifiers), `extra` reduced to its numeric leaves; never longer than `limit` bytes -- legs of
    `extra` are dropped (listed under `extra_dropped`) before anything of the headline is."""
    line = {}
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data'):
        if k in result:
            v = result[k]
            line[k] = _first_sentence(v, 120) if isinstance(v, str) else (_sig(v, 7) if isinstance(v, float) else v)
    cfg = result.get('config', {})
    line['config'] = {k: (_first_sentence(v, 200) if isinstance(v, str) else v) for k, v in cfg.items() if not isinstance(v, (dict, list))}
    rf = result.get('roofline')
    if rf is not None:
        line['roofline'] = {k: (_first_sentence(rf[k], 64) if isinstance(rf[k], str) else _sig(rf[k], 6) if isinstance(rf[k], float) else rf[k])
                            for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'avg_launch_ms', 'whole_step_frac',
                                      'frac_of_bf16_mfma_peak_at_6_mfma_per_product') if k in rf}
        line['roofline'].setdefault('traffic', None)
    cb = result.get('cpu_baseline')
    if cb is not None:
        line['cpu_baseline'] = {k: (_first_sentence(cb[k], 120) if isinstance(cb[k], str) else _sig(cb[k], 6) if isinstance(cb[k], float) else cb[k])
                                for k in ('value', 'unit', 'cores', 'kind', 'cpu_model', 'sample') if k in cb}
    for k in ('psnr_vs_oracle_db', 'speedup_vs_cpu', 'psnr_f16s_vs_oracle_db', 'psnr_x3_vs_oracle_db'):
        if k in result:
            line[k] = _sig(result[k], 6)
    for k in ('all_reduce', 'last_train_backend', 'error', 'exit_code'):
        if k in result:
            line[k] = _compact(result[k])
    if 'kernel_ms_per_step' in result:
        line['kernel_ms_per_step'] = {k: _sig(v, 4) for k, v in result['kernel_ms_per_step'].items()}
    if 'cpu_baseline_decomp' in result:
        line['cpu_baseline_decomp'] = _compact(result['cpu_baseline_decomp'])
    if detail_path:
        line['detail'] = detail_path
    extra = _compact(result.get('extra', {}), drop=_EXTRA_CONST_KEYS) or {}
    if extra:
        line['extra'] = extra
    dropped = []
    # (unknown legs go first: the ranked ones are the ones somebody asked to see)
    order = [k for k in extra if k not in _DROP_ORDER] + [k for k in _DROP_ORDER if k in extra]
    while len(json.dumps(line, separators=(',', ':'))) > limit and order:
        k = order.pop(0)
        extra.pop(k, None)
        dropped.append(k)
        line['extra_dropped'] = dropped
    if not extra:
        line.pop('extra', None)
    for k in ('cpu_baseline_decomp', 'kernel_ms_per_step', 'extra', 'extra_dropped'):
        if len(json.dumps(line, separators=(',', ':'))) <= limit:
            break
        line.pop(k, None)
    text = json.dumps(line, separators=(',', ':'))
    assert len(text) <= limit, f'bench line is {len(text)} bytes (limit {limit})'
    json.loads(text)
    return text


def detail_file():
    """where the sidecar goes: $VQN_BENCH_DETAIL, else gpurun_out/bench_detail.json under the repo (gpurun brings that directory back)"""
    p = os.environ.get('VQN_BENCH_DETAIL')
    if p:
        return p
    d = os.path.join(ROOT, 'gpurun_out')
    try:
        os.makedirs(d, exist_ok=True)
        return os.path.join(d, 'bench_detail.json')
    except OSError:
        return os.path.join('/tmp', 'bench_detail.json')


NO_DETAIL = False           # --no-detail: a profiler / counter pass of this command must not overwrite the real run's sidecar


def emit(result):
    """sidecar first (full result: prose, windows, kernel tables), then the ONE short stdout line"""
    if NO_DETAIL:
        print(compact_line(result), flush=True)
        return
    path = detail_file()
    rel = None
    try:
        with open(path, 'w') as f:
            json.dump(result, f, indent=1, default=lambda o: repr(o)[:200])
        rel = os.path.relpath(path, ROOT) if path.startswith(ROOT) else path
    except OSError as e:
        _log(f'could not write the detail sidecar {path}: {e!r}')
    print(compact_line(result, detail_path=rel), flush=True)


def self_launch(args):
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment: start the N ranks OURSELVES, as a child
    `python -m torch.distributed.run` of this very command (the reference splits its views the same way, one process per share:
    gen_geo.py:141-146, trainvali.py:436-447).  Nothing in this process has touched the GPU at this point (and nothing will: it only
    relays rank 0's line and exits with the child's code -- never an exec)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env['MASTER_ADDR'] = '127.0.0.1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    _log(f'--gpus {args.gpus} without WORLD_SIZE: launching {args.gpus} ranks as a child torch.distributed.run (port {port})')
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    for ln in child.stdout:                                      # rank 0's JSON line to stdout; anything else the ranks print (gloo's
        out = sys.stdout if ln.lstrip().startswith('{') else sys.stderr      # connection notes, library banners) to stderr: ONE line on stdout
        out.write(ln)
        out.flush()
    rc = child.wait()
    if rc != 0:
        _log(f'child torch.distributed.run exited with {rc}')
    sys.exit(rc)



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--mode', choices=('render', 'train'), default='render',
                    help='render: the headline (one whole 800x800 view per rank per step); train: the DP geo training step is the timed step')
    ap.add_argument('--rays', type=int, default=640000, help='rays per step per GPU (render mode); 640000 = one 800x800 view')
    ap.add_argument('--cpu-rays', type=int, default=2560, help='rays per call of the bounded CPU-baseline sample (SURVEY 8d: B = 2560)')
    ap.add_argument('--cpu-reps', type=int, default=3, help='timed CPU calls after one warm-up call (median is reported)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-extras', action='store_true', help='skip the secondary workloads (train steps, decomp, VQ)')
    ap.add_argument('--no-traffic', action='store_true', help='do not measure roofline.traffic with child rocprofv3 --pmc passes')
    ap.add_argument('--no-detail', action='store_true', help='do not write the sidecar bench_detail.json (profiler / counter passes of this command)')
    ap.add_argument('--full', action='store_true',
                    help='also run everything beyond the headline: traffic passes, CPU baselines, other precisions, secondary and '
                         'data-parallel legs, the sidecar (the --no-* options then deselect parts of it)')
    ap.add_argument('--dump-outputs', metavar='DIR', help='write the outputs of the last timed step as DIR/<name>.npy (rank 0)')
    args = ap.parse_args()
    if not args.full:                                           # a plain run: the headline only
        args.no_cpu_baseline = args.no_extras = args.no_traffic = args.no_detail = True
    global NO_DETAIL
    NO_DETAIL = bool(args.no_detail)

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return self_launch(args)                                # (before any GPU call; exits with the child's code)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run'
    # HBM-side traffic of the dominant kernel, measured live by child profiler passes -- before this process initialises the GPU
    measured_traffic = (None, 'not measured (no --full, --no-traffic, --mode train or a multi-rank run)')
    if world == 1 and not args.no_traffic and args.mode == 'render' and os.environ.get('VQN_BENCH_NO_TRAFFIC', '0') in ('', '0'):
        _log('roofline.traffic: two child rocprofv3 --pmc passes')
        measured_traffic = live_traffic(args.rays)
        _log('traffic passes done')
    assert torch.cuda.is_available(), 'bench.py needs an MI355X (no CPU fallback)'
    local_rank %= torch.cuda.device_count()        # (rehearsals put several ranks on one card; the driver gives one GPU per rank)
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    backend = os.environ.get('VQN_BENCH_BACKEND', 'nccl')      # 'gloo' only to rehearse the multi-rank path on a 1-GPU box
    if world > 1:
        import torch.distributed as dist
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev)
        else:
            dist.init_process_group(backend)

    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork, SingleVarianceNetwork
    from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
    _C.lib()

    if args.mode == 'train':
        return main_train(args, dev, rank, world, backend)

    _log('leg: random-init weights of the shipped architecture')
    # ---- random-init weights of the shipped architecture (same seed on every rank) ----
    torch.manual_seed(0)
    sdf = SDFNetwork(**FULL['sdf'])
    col = RenderingNetwork(**FULL['color'])
    var = SingleVarianceNetwork(0.3)
    state = {'sdf': {k: v.clone() for k, v in sdf.state_dict().items()},
             'col': {k: v.clone() for k, v in col.state_dict().items()}}
    sdf, col, var = sdf.to(dev), col.to(dev), var.to(dev)
    ren = NeuSRenderer(None, sdf, var, col, **FULL['renderer'])
    S_f = FULL['renderer']['n_samples'] + FULL['renderer']['n_importance']

    _log('leg: this ranks rays')
    # ---- this rank's rays: the rows of its own 800x800 view (camera turned by rank * 2 pi / world), resident in HBM ----
    n_rows = (args.rays + 799) // 800
    rows = np.arange(n_rows) % 800
    o_np, d_np = image_rays(rows, yaw=2.0 * math.pi * rank / world)
    o_np, d_np = o_np[:args.rays], d_np[:args.rays]
    o, d = torch.tensor(o_np, device=dev), torch.tensor(d_np, device=dev)
    near = torch.full((args.rays, 1), 2.0, device=dev)
    far = torch.full((args.rays, 1), 6.0, device=dev)
    bg = torch.ones(1, 3, device=dev)
    out_box = [None]

    def step():
        with torch.no_grad():
            out_box[0] = ren.render(o, d, near, far, 2.0, perturb_overwrite=0, background_rgb=bg, cos_anneal_ratio=1.0)

    _log('headline render: warm-up + timed steps')
    dt, clock = _timed_steps(step, args.steps, args.warmup, dev, world, backend)
    _log('headline render done')
    out = out_box[0]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out, args.rays)
    assert torch.isfinite(out['color_fine']).all()

    # every rank takes part in the data-parallel training legs (collectives); only rank 0 reports.  Those legs have run on two ranks
    # sharing a card, never on a multi-GPU RCCL node: a watchdog makes sure the headline line is printed whatever they do -- if they have
    # not returned after VQN_BENCH_DP_TIMEOUT seconds (default 420), rank 0 prints the line with the error under extra.dp_train and
    # every rank leaves (a rank stuck in a collective cannot be interrupted any other way); an exception in them is reported the same way
    def guarded_dp_legs(partial_line):
        import threading
        done = threading.Event()
        limit = float(os.environ.get('VQN_BENCH_DP_TIMEOUT', '420'))

        def watchdog():
            if not done.wait(limit):
                if rank == 0 and partial_line is not None:
                    partial_line.setdefault('extra', {})['dp_train'] = {'error': f'the data-parallel training legs did not return within {limit:.0f} s',
                                                                        'exit_code': WATCHDOG_EXIT}
                    partial_line['exit_code'] = WATCHDOG_EXIT
                    emit(partial_line)
                # a rank stuck in a collective has touched the GPU and cannot be unwound: every rank leaves NON-ZERO (the launcher and
                # the driver must see the hang), rank 0 after printing the complete render line
                os._exit(WATCHDOG_EXIT)
        threading.Thread(target=watchdog, daemon=True).start()
        try:
            return dp_train_leg(dev, rank, world, backend)
        except Exception as e:                                  # noqa: BLE001
            return {'error': repr(e)[:400]}
        finally:
            done.set()

    if rank != 0:
        if world > 1 and not args.no_extras:
            out_box[0] = None
            out = None
            guarded_dp_legs(None)
        if world > 1:
            dist.destroy_process_group()
        return

    total_rays = args.rays * world * args.steps
    value = total_rays / dt
    m_sdf, m_col = macs_per_point(sdf, col)
    # dominant kernel: one fine launch evaluates, per point, one SDF forward, one reverse (input-gradient)
    # sweep of the same MACs, and one colour forward
    n_fine, ms_fine = clock['vqn_neus_fine_points']
    flop_fine = 2.0 * (2 * m_sdf + m_col) * args.rays * S_f
    avg_ms = ms_fine / n_fine
    achieved = flop_fine / (avg_ms * 1e-3) / 1e12
    # fabric-side bytes per launch of the dominant kernel: NOT measured by this run (PMC counters need rocprofv3 around the
    # process) -- the builder's committed passes of this same command (scripts/pmc_traffic.sh: separate `rocprofv3 --pmc
    # FETCH_SIZE` / `--pmc WRITE_SIZE` runs), per ray, scaled to this launch; null if the file is absent
    traffic, traffic_note = measured_traffic
    for name in (() if traffic is not None else ('r02_pmc_render.json', 'r01_pmc_render.json')):
        try:
            with open(os.path.join(ROOT, 'profiles', name)) as f:
                pmc = json.load(f)
            traffic = pmc['dominant_kernel_traffic_bytes_per_launch'] * args.rays / pmc['rays_per_launch']
            traffic_note = (f'live measurement unavailable ({measured_traffic[1]}); from profiles/{name} (builder-run rocprofv3 PMC passes of this command): '
                            '2*FETCH_SIZE + WRITE_SIZE per launch; counts fabric requests incl. Infinity-Cache hits: the '
                            'per-workgroup activation stash of the reverse sweep (8 x 32 KB per tile, 134 MB in flight, '
                            'Infinity-Cache resident) is written once and read once per tile with streaming (nt) accesses; '
                            'algorithmic bytes are 32 B in + 28 B out per sample')
            break
        except Exception:
            continue
    result = {
        'metric': 'rays/sec (render) 800x800, 64+64 samples/ray, NeuS SDF 8x256 + colour 4x256',
        'value': value, 'unit': 'rays/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': dt / args.steps * 1e3, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': 'BASELINE configs[1], nerf/hotdog-shaped NeuS render: one whole 800x800 pin-hole view per rank per step '
                               '(camera at distance 4, fov 0.6911), n_samples=64, n_importance=64, up_sample_steps=4, '
                               'sdf 8x256 (skip 4, posenc 6), colour 4x256 (idr, posenc_view 4), random-init weights '
                               '(geometric-init sphere of radius 0.85: ~30 % of the rays hit)',
                   'rays_per_step_per_gpu': args.rays, 'parallelism': f'views x{world} (no data-path collective)'},
        'roofline': {'bound': 'mfma', 'kernel': 'neus_points2_kernel<FINE = true, TRAIN = false> (vqn_neus_fine_points)', 'achieved': achieved,
                     'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': achieved / F32_MFMA_PEAK_TFLOPS,
                     'traffic': traffic, 'traffic_note': traffic_note, 'avg_launch_ms': avg_ms, 'flop_per_launch': flop_fine,
                     'macs_per_point': {'sdf': m_sdf, 'colour': m_col}},
        'kernel_ms_per_step': {k: v[1] / args.steps for k, v in sorted(clock.items())},
    }

    # the rays the CPU leg will re-render, taken NOW: the training legs below step these same networks' weights
    sel = np.linspace(0, args.rays - 1, args.cpu_rays).astype(np.int64)      # spread over the whole view: hits and misses
    if world == 1 and not args.no_cpu_baseline:
        sel_t = torch.tensor(sel, device=dev)
        got, got_ws = out['color_fine'][sel_t].cpu(), out['weight_sum'][sel_t].cpu()[:, 0]
        ren.matrix_mode = 'f16s'                                  # the opt-in split-precision mode on the same rays
        try:
            step()
            got16 = out_box[0]['color_fine'][sel_t].cpu()
            ren.matrix_mode = 'x3'                                # the exact-split mode on the same rays
            step()
            got_x3 = out_box[0]['color_fine'][sel_t].cpu()
        finally:
            ren.matrix_mode = 'f32'
    del out
    out_box[0] = None

    extra = {}
    if world == 1 and not args.no_extras:
        # before the CPU legs: a spun-up host thread pool slows the launch-heavy training steps that follow it
        # (a secondary leg that raises must not take the headline line with it)
        try:
            extra = secondary_measurements(dev, sdf, col, var, ren, m_sdf, m_col)
        except Exception as e:                                  # noqa: BLE001
            import traceback
            extra = {'error': 'secondary_measurements raised: ' + repr(e)[:300], 'traceback': traceback.format_exc()[-1500:]}
        _log('dp_train legs')
        try:
            extra['dp_train'] = dp_train_leg(dev, 0, 1, backend, steps=6, warmup=2)      # the same legs a multi-rank run reports
        except Exception as e:                                  # noqa: BLE001
            extra['dp_train'] = {'error': repr(e)[:400]}
    if world > 1 and not args.no_extras:
        _log('dp_train legs (all ranks)')
        extra['dp_train'] = guarded_dp_legs(result)
    if world == 1 and not args.no_cpu_baseline:
        _log('CPU baseline (oracle) legs')
        from oracle import geo as og                      # CPU-baseline leg only (test infrastructure)
        cfg = dict(og.FULL_CFG)
        p_sdf = {k: v.float() for k, v in state['sdf'].items()}
        p_col = {k: v.float() for k, v in state['col'].items()}
        n_cpu = args.cpu_rays
        oc, dc = torch.tensor(o_np[sel]), torch.tensor(d_np[sel])
        nc, fc = torch.full((n_cpu, 1), 2.0), torch.full((n_cpu, 1), 6.0)
        cores = os.cpu_count() or 1
        try:
            cores = len(os.sched_getaffinity(0))
        except Exception:
            pass
        # Threads.  The affinity mask of a 1-GPU box of this pool lists the whole host (256 hardware threads) while the job's CPU share is 16
        # (the pool's own sizing rule; 8 such jobs share the host): a call with 256 threads did not finish in 7 minutes (round 4, measured --
        # oversubscription), so `value` is measured at the 16-thread share as in rounds 1-3, and one call at host / 8 = 32 threads is
        # reported beside it.  VQN_CPU_THREADS overrides the first figure.
        cores_all = cores
        cores = int(os.environ.get('VQN_CPU_THREADS', min(cores_all, 16)))
        cpu_call = lambda: og.render(p_sdf, p_col, torch.tensor(0.3), cfg, oc, dc, nc, fc, 2.0, background_rgb=torch.ones(1, 3),
                                     cos_anneal_ratio=1.0)
        wide = min(cores_all, max(32, cores_all // 8)) if cores_all > cores else 0
        t_wide = None
        if wide > cores:
            torch.set_num_threads(wide)
            _log(f'CPU baseline: one call at {wide} threads')
            cpu_call()
            t0 = time.perf_counter()
            cpu_call()
            t_wide = time.perf_counter() - t0
        torch.set_num_threads(cores)
        _log(f'CPU baseline: {cores} threads')
        cpu_call()                                                        # warm-up: one full call at the same batch
        times = []
        for _ in range(max(1, args.cpu_reps)):
            t0 = time.perf_counter()
            ref = cpu_call()
            times.append(time.perf_counter() - t0)
        cpu_dt = float(np.median(times))
        ws_ref = ref['weight_sum'].detach()[:, 0]
        mse = float(((got - ref['color_fine'].detach()) ** 2).mean())
        result['cpu_baseline'] = {'value': n_cpu / cpu_dt, 'unit': 'rays/s', 'cores': cores, 'kind': 'port',
                                  'cpu_model': cpu_model_string(),
                                  'sample': f'{n_cpu} rays spread over the whole 800x800 view (same weights) per oracle.geo.render call; '
                                            f'1 warm-up + {len(times)} timed calls, median {cpu_dt:.1f} s '
                                            f'(all: {", ".join("%.1f" % t for t in times)} s); torch {torch.__version__} CPU fp32, '
                                            f'{cores} threads (affinity mask: {cores_all})',
                                  'wider': ({'threads': wide, 'value': n_cpu / t_wide, 'calls': '1 warm-up + 1 timed'} if t_wide else None)}
        result['psnr_vs_oracle_db'] = -10.0 * math.log10(mse + 1e-20)
        result['psnr_sample'] = {'rays': n_cpu, 'frac_weight_sum_gt_0.5': float((ws_ref > 0.5).float().mean()),
                                 'frac_weight_sum_gt_0.9': float((ws_ref > 0.9).float().mean()),
                                 'colour_std_of_sample': float(ref['color_fine'].detach().std()),
                                 'max_abs_colour_diff': float((got - ref['color_fine'].detach()).abs().max()),
                                 'max_abs_weight_sum_diff': float((got_ws - ws_ref).abs().max())}
        result['speedup_vs_cpu'] = value / (n_cpu / cpu_dt)
        # the same check for the opt-in split-precision mode (reported under extra.geo_render_f16s)
        mse16 = float(((got16 - ref['color_fine'].detach()) ** 2).mean())
        result['psnr_f16s_vs_oracle_db'] = -10.0 * math.log10(mse16 + 1e-20)
        result['psnr_x3_vs_oracle_db'] = -10.0 * math.log10(float(((got_x3 - ref['color_fine'].detach()) ** 2).mean()) + 1e-20)
        if not args.no_extras:
            _log('CPU baseline of the reflectance model')
            # the reference batch (2048 points) and a 65,536-point view share
            try:
                result['cpu_baseline_decomp'] = decomp_cpu_leg(dev, cores, N=65536)
                result['cpu_baseline_decomp']['at_2048_points'] = {k: v for k, v in decomp_cpu_leg(dev, cores, N=2048).items()
                                                                    if k in ('value', 'sample', 'gpu_points_per_s_same_sample', 'vq_idx_match_pct')}
            except Exception as e:                              # noqa: BLE001
                result['cpu_baseline_decomp'] = {'error': repr(e)[:400]}
    if extra:
        result['extra'] = extra
    emit(result)
    if world > 1:
        dist.destroy_process_group()


def main_train(args, dev, rank, world, backend):
    """--mode train: the timed step is the data-parallel geo training step (2560 rays per rank; forward + backward on the HIP
    two-image kernels, one flat-bucket all-reduce of the 1.4 M gradients over RCCL, Adam).  `value` = training rays/s, whole job."""
    from vqnerf_release_amd import _C
    runner, gstep = geo_train_setup(dev, rank)
    dt, clock = _timed_steps(gstep, args.steps, args.warmup, dev, world, backend, prime=PRIME_LAUNCHES // 300)
    if args.dump_outputs and rank == 0:                         # the step's losses and the weights it leaves behind
        params = {f'{net}.{k}': v for net in ('sdf_network', 'deviation_network', 'color_network') for k, v in getattr(runner, net).named_parameters()}
        dump_outputs(args.dump_outputs, dict(runner.last_stats, **params), rows=None)
    sdf, col = runner.sdf_network, runner.color_network
    m_sdf, m_col = macs_per_point(sdf, col)
    B = 2560
    bucket_bytes = int(runner.bucket.flat.numel() * 4)
    dec = None
    if not args.no_extras:
        del gstep
        model, tr, dstep = decomp_train_setup(dev, rank, world)
        ddt, dclk = _timed_steps(dstep, args.steps, args.warmup, dev, world, backend, prime=PRIME_LAUNCHES // 300)
        dec = {'points_per_s': 2048 * world * args.steps / ddt, 'ms_per_step': ddt / args.steps * 1e3, 'batch_points_per_rank': 2048,
               'grad_bucket_bytes': int(tr.bucket.flat.numel() * 4), 'vq_stats_bytes': int((256 + 1) * 15 * 4),
               'all_reduce': _collective_report(dclk, args.steps)}
    if rank != 0:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
        return
    # algorithmic FLOPs of one rank's step: coarse SDF passes + [fwd, reverse sweep, tangent, reverse, 2 weight
    # contractions] of the SDF net + [fwd, reverse, weight contraction] of the colour net, per fine sample
    flop = 2.0 * B * ((64 + 48) * m_sdf + 128 * (6 * m_sdf + 3 * m_col))
    # (the per-point forward / backward kernels: vqn_neus_train_fwd + vqn_neus_train_bwd on the two-image engine since round 3, the
    # interpreted tile programs for networks those do not take)
    t_prog = sum(v[1] for k, v in clock.items() if k.startswith(('vqn_tile_program', 'vqn_neus_train_'))) / args.steps * 1e-3
    flop_prog = 2.0 * B * 128 * (4 * m_sdf + 2 * m_col)
    step_s = dt / args.steps
    import torch.distributed as dist
    result = {
        'metric': 'rays/sec (train) 2560 rays/step/GPU of 800x800 views, 64+64 samples/ray, NeuS SDF 8x256 + colour 4x256',
        'value': B * world / step_s, 'unit': 'rays/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': step_s * 1e3, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f32 (layer products as exact bf16 piece triples, six bf16 MFMAs each, f32 accumulation; VQN_TRAIN_FWD/BWD=fused: f32-input MFMA)',
        'data': 'synthetic',
        'config': {'workload': 'BASELINE configs[1] / configs[3] training step: nerf.conf batch of 2560 rays per rank (random pixels of '
                               'synthetic 800x800 views), L1 colour + 0.1 eikonal + 0.1 mask BCE, Adam; data parallel over ranks with ONE '
                               'flat-bucket all-reduce of the gradients per step', 'rays_per_step_per_gpu': B,
                   'parallelism': f'dp{world}', 'n_ranks_seen': dist.get_world_size() if world > 1 else 1},
        'roofline': {'bound': 'mfma', 'kernel': 'neus_points2_kernel<true, true> + neus_train_bwd2_kernel (vqn_neus_train_fwd / _bwd: forward, '
                                                'colour backward + SDF backward with the second-order terms)',
                     'achieved': flop_prog / t_prog / 1e12, 'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                     'frac': flop_prog / t_prog / 1e12 / F32_MFMA_PEAK_TFLOPS, 'traffic': None,
                     'frac_of_bf16_mfma_peak_at_6_mfma_per_product': 6.0 * flop_prog / t_prog / 1e12 / BF16_MFMA_PEAK_TFLOPS,
                     'note': 'f32-equivalent FLOPs over the f32-input MFMA peak (what the f32 kernels of rounds 1-2 were priced against); the default '
                             'kernels since round 3 run on the bf16 pipe at six MFMAs per product -- the second fraction is their share of THAT peak',
                     'whole_step_tflops': flop / step_s / 1e12, 'whole_step_frac': flop / step_s / 1e12 / F32_MFMA_PEAK_TFLOPS},
        'kernel_ms_per_step': {k: v[1] / args.steps for k, v in sorted(clock.items())},
        'all_reduce': dict(_collective_report(clock, args.steps), grad_bucket_bytes=bucket_bytes),
        'last_train_backend': runner.renderer.last_train_backend,
    }
    if dec is not None:
        result['extra'] = {'decomp_train_dp': dec}
    emit(result)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
