"""Measures the material-ball kernel on the device.

  --errors PATH   the yardstick of tests/test_gpu_material_balls.py: the shading kernel's and the new kernel's largest absolute error
                  against the float64 model on the foreground samples of that test's yardstick case -> PATH
                  (profiles/observed_errors_material_balls.json)
  --timing PATH   the palette shape (K = 64 codes, the model's light + 16 probes, 512 lights, 128^2 pixels at 4 spp): the new entry
                  against the baseline of the code before it -- the same foreground samples materialised once, [M S] rows, shaded by
                  vqn_brdf_shade_fwd with the probes in LDS, as ONE call over M S rows and as M calls of S rows; buffer construction
                  is outside the baseline's timed window.  Windows alternate between the candidates; every window ends in a device
                  synchronise -> PATH (profiles/material_balls.json)
A run without a device fails: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import material_balls_model as mb  # noqa: E402
from vqnerf_release_amd import _C  # noqa: E402


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device='cuda')


def errors(path):
    from tests import test_gpu_material_balls as t
    ims, spp, M, kind, probe_names, hw, white_bg, rot, gamma = t.CASES[t.YARDSTICK]
    lxyz, areas = mb.gen_light_xyz(*hw)
    lxyz, areas = lxyz.reshape(-1, 3).astype(np.float32), areas.reshape(-1).astype(np.float32)
    mats, probes = t._materials(kind, M, seed=len(t.YARDSTICK)), t._probes(probe_names, hw)
    fg, xyz, normal, cam = mb.geometry(ims, spp, cam_rot=rot)
    S, P = xyz.shape[0], probes.shape[0]
    want = mb.render(mats, probes, lxyz, areas, ims, spp, cam_rot=rot, white_bg=white_bg, gamma=gamma)[:, :, fg]
    got = _C.material_balls(_dev(mats), _dev(probes), _dev(lxyz), _dev(areas), ims, spp, cam_rot=rot, white_bg=white_bg)['f32']
    balls = float(np.abs(got.cpu().numpy().astype(np.float64)[:, :, fg] - want).max())
    rep = lambda a: _dev(np.repeat(a[None], M, 0).reshape(M * S, -1))
    rows = np.repeat(mats[:, None], S, 1).reshape(M * S, 7)
    out = _C.brdf_shade_fwd(rep(xyz), rep(normal), rep(np.broadcast_to(cam, xyz.shape)), None, _dev(lxyz), _dev(areas), _dev(probes[0]),
                            [(_dev(rows[:, :3]), _dev(rows[:, 3:6]), _dev(rows[:, 6:7]))], want_normal=False, probes=_dev(probes))
    shade = out['rgb_probes'].cpu().numpy().astype(np.float64).reshape(M, S, P, 3).transpose(0, 2, 1, 3)
    rec = {'device': torch.cuda.get_device_name(0), 'case': t.YARDSTICK, 'ims': ims, 'spp': spp, 'materials': M, 'probes': P,
           'lights': int(areas.size), 'foreground_samples': int(S),
           'shade_kernel_max_abs_err': float(np.abs(shade - want).max()), 'material_balls_max_abs_err': balls,
           'bound': 'material_balls_max_abs_err <= 2 * shade_kernel_max_abs_err',
           'note': 'largest absolute error of the displayed linear values (after the clip) against tests/material_balls_model.py in '
                   'float64, over the same foreground samples, materials and probes'}
    with open(path, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def matrix_engine_estimate(S, M, L, P):
    """arithmetic only, nothing here is measured: the light sum as the GEMM [2 M x L] . [L x 3 P] per sample on the f32-input MFMA"""
    peak = 157.3e12                                              # f32-input MFMA = f32 vector peak on gfx950
    gemm = 2.0 * (2 * M) * L * (3 * P) * S
    return {'measured': False, 'flop_gemm_all_lights': gemm, 'flop_gemm_front_lit_half': gemm / 2, 'flop_valu_form_front_lit_half': gemm / 4,
            'f32_mfma_peak_flop_per_s': peak, 'ms_at_peak_gemm_front_lit_half': gemm / 2 / peak * 1e3,
            'ms_at_peak_valu_form': gemm / 4 / peak * 1e3,
            'why_not_built': 'the f32-input MFMA runs at the f32 vector rate, and the GEMM form needs two rows per material (f0 DG and '
                             '(1 - f0) DG s_l: the per-channel Fresnel factor cannot sit inside the product) where the lane-per-material '
                             'VALU form needs one; the D G1 table would be VALU work either way'}


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def timing(path, windows=9, calls=5):
    M, P, hw, ims, spp = 64, 17, (16, 32), 128, 4
    rng = np.random.default_rng(0)
    lxyz, areas = mb.gen_light_xyz(*hw)
    lxyz, areas = _dev(lxyz.reshape(-1, 3)), _dev(areas.reshape(-1))
    mats_h = rng.uniform(0, 1, (M, 7)).astype(np.float32)
    mats_h[:, 6] = 0.05 + 0.95 * mats_h[:, 6]
    probes = _dev(rng.uniform(0, 2, (P, hw[0] * hw[1], 3)))
    mats = _dev(mats_h)
    fg, xyz, normal, cam = mb.geometry(ims, spp)
    S = xyz.shape[0]
    # the baseline's buffers, built once outside every timed window
    rep = lambda a: _dev(np.repeat(a[None], M, 0).reshape(M * S, -1))
    X, N, O = rep(xyz), rep(normal), rep(np.broadcast_to(cam, xyz.shape))
    rows = np.repeat(mats_h[:, None], S, 1).reshape(M * S, 7)
    A, F, R = _dev(rows[:, :3]), _dev(rows[:, 3:6]), _dev(rows[:, 6:7])
    light0 = probes[0].contiguous()

    def balls_f32():
        return _C.material_balls(mats, probes, lxyz, areas, ims, spp, want_f32=True, want_u8=False)

    def balls_all():
        return _C.material_balls(mats, probes, lxyz, areas, ims, spp, want_f32=True, want_u8=True, sheet=(None, 8, 8))

    def base_one():
        return _C.brdf_shade_fwd(X, N, O, None, lxyz, areas, light0, [(A, F, R)], want_normal=False, probes=probes)

    def base_m():
        for m in range(M):
            s = slice(m * S, (m + 1) * S)
            _C.brdf_shade_fwd(X[s], N[s], O[s], None, lxyz, areas, light0, [(A[s], F[s], R[s])], want_normal=False, probes=probes)

    cands = {'material_balls_f32': balls_f32, 'material_balls_f32_u8_sheet': balls_all, 'baseline_one_call': base_one, 'baseline_m_calls': base_m}
    # same values: the baseline's per-sample colours averaged per pixel against the new entry's image
    got = balls_f32()['f32'].cpu().numpy().astype(np.float64)
    per = base_one()['rgb_probes'].cpu().numpy().astype(np.float64).reshape(M, S, P, 3)
    img = np.ones(fg.shape + (M, P, 3))
    img[fg] = per.transpose(1, 0, 2, 3)
    same = float(np.abs(mb.average(img, spp).transpose(2, 3, 0, 1, 4) - got).max())
    for fn in cands.values():                                    # warm every shape
        fn()
    times = {k: [] for k in cands}
    for _ in range(windows):
        for k, fn in cands.items():                              # alternating
            times[k].append(_window(fn, calls))
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v)), 'max_ms': float(np.max(v))}
    res = {k: stat(v) for k, v in times.items()}
    best_base = min(res['baseline_one_call']['median_ms'], res['baseline_m_calls']['median_ms'])
    lit = 0.5 * hw[0] * hw[1]
    flops = 2.0 * S * M * lit * 3 * P                            # the fused multiply-adds of the light sum the kernel issues (front-lit lights)
    rec = {'device': torch.cuda.get_device_name(0), 'shape': {'materials': M, 'probes': P, 'lights': hw[0] * hw[1], 'ims': ims, 'spp': spp,
                                                               'foreground_samples': int(S)},
           'windows': windows, 'calls_per_window': calls, 'times': res,
           'max_abs_difference_new_vs_baseline': same,
           'baseline_over_new': best_base / res['material_balls_f32']['median_ms'],
           'new_no_slower_than_baseline_beyond_spread': res['material_balls_f32']['min_ms'] <= max(res['baseline_one_call']['max_ms'],
                                                                                                    res['baseline_m_calls']['max_ms'])
           and res['material_balls_f32']['median_ms'] <= best_base,
           'light_sum_flop': flops, 'light_sum_flop_per_s': flops / (res['material_balls_f32']['median_ms'] * 1e-3),
           'matrix_engine_estimate': matrix_engine_estimate(S, M, hw[0] * hw[1], P),
           'note': 'each time is a host clock around calls_per_window back-to-back calls ending in a device synchronise, per call; the '
                   'windows of the four candidates alternate; the baseline buffers ([M S] rows of xyz / normal / origin / material) '
                   'are built once outside the windows; light_sum_flop counts 2 * S * M * (L / 2 front-lit lights) * 3 P'}
    with open(path, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--errors')
    ap.add_argument('--timing')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_material_balls.py needs the device: no number here comes from a CPU run')
    _C.lib()
    if a.errors:
        errors(a.errors)
    if a.timing:
        timing(a.timing)
