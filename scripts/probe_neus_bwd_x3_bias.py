"""Is the backward of the NeuS training step odd in its adjoint, and how does its error grow with the point count?

Shipped shape of tests/neus_train_cases.py, loss <rgb, g_rgb> alone, through NeusCoreFunction.  Per P and engine setting (forward,
backward, weight-gradient contraction) and parameter gradient: rms / max error against the float64 statement over the tensor's largest
entry, the float32 statement's own rms (ref_rms), and even_rms = rms of (gradient(g) + gradient(-g)) / 2 over the same entry, which is
exactly 0 for an evaluation that is odd in g.  Then, at 644 points, the even part of every tensor the backward kernel writes.
VQN_X3_BWD_NACC (accumulators per image of vqn_neus_train_bwd_x3) is read once per process: run once per setting.
    python scripts/probe_neus_bwd_x3_bias.py OUT.json        (appends its rows to OUT.json)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import neus_train_cases as nc                                     # noqa: E402
from vqnerf_release_amd import wgrad                                       # noqa: E402
from vqnerf_release_amd.geo import train_programs as tp                     # noqa: E402

SHAPE = 'shipped'
SETTINGS = (('x3', 'x3', 'bf16x3'), ('fused', 'x3', 'bf16x3'), ('x3', 'x3', 'f32'), ('x3', 'fused', 'bf16x3'), ('fused', 'fused', 'f32'),
            ('prog', 'prog', 'bf16x3'))
TENSORS = ('db7', 'db0', 'dW7', 'dW3', 'dbc0', 'dWc0')
rms = lambda e: float(np.sqrt((e ** 2).mean()))
sig = lambda v: float('%.3g' % v)


def main(out_path):
    nacc = os.environ.get('VQN_X3_BWD_NACC', '')
    eng = nc.build_engine(SHAPE, 'cuda')
    params = [[t.cuda() for t in ts] for ts in nc.effective_params(SHAPE)]
    names = nc.grad_names(SHAPE)

    def run(x, dirs, g):
        leaves = [t.clone().requires_grad_(True) for ts in params for t in ts]
        sdf, n, rgb = tp.NeusCoreFunction.apply(eng, x, dirs, *leaves)
        (rgb * g).sum().backward()
        return {k: t.grad.detach().double().cpu().numpy() for k, t in zip(names, leaves)}

    rows = []
    for P in (161, 644, 2576):
        ref = nc.reference(SHAPE, P)
        x, dirs, g = ref['x'].cuda(), ref['dirs'].cuda(), ref['g_rgb'].cuda()
        r64, r32 = ref['f64']['grads']['rgb'], ref['f32']['grads']['rgb']
        for fwd, bwd, wg in SETTINGS:
            os.environ['VQN_TRAIN_FWD'], os.environ['VQN_TRAIN_BWD'] = fwd, bwd
            wgrad.wgrad_mode(wg)
            a, b = run(x, dirs, g), run(x, dirs, -g)
            row = dict(P=P, fwd=fwd, bwd=bwd, wgrad=wg, VQN_X3_BWD_NACC=nacc)
            for k in TENSORS:
                top = np.abs(r64[k]).max()
                e = (a[k] - r64[k]) / top
                row[k] = dict(rms=sig(rms(e)), max=sig(np.abs(e).max()), ref_rms=sig(rms((r32[k] - r64[k]) / top)),
                              even_rms=sig(rms((a[k] + b[k]) / 2 / top)))
            rows.append(row)
            print(row, flush=True)
    # the tensors the backward kernel itself writes, in the order it writes them
    P = 644
    ref = nc.reference(SHAPE, P)
    x, dirs, g = ref['x'].cuda(), ref['dirs'].cuda(), ref['g_rgb'].cuda()
    nL, nC = eng.nL, eng.nC
    outs = ['DC%d' % l for l in range(nC, -1, -1)] + ['GOUTF', 'ED'] + ['UD%d' % (l + 1) for l in range(nL)] + ['AB%d' % l for l in range(nL - 1, -1, -1)]
    with torch.no_grad():
        flat = eng.flat_weights(*params)
        res = {}
        for sgn in (1.0, -1.0):
            T = eng.alloc_tensors(P, x.device)
            T['X'].copy_(x)
            T['DIRS'].copy_(dirs)
            eng.run_fused_forward(flat, T, P)
            eng.run_fused_backward_x3(flat, T, P, (sgn * g).contiguous(), None, None)
            res[sgn] = {n: T[n].double().cpu() for n in outs}
    kernel = dict(P=P, VQN_X3_BWD_NACC=nacc, tensors={})
    for n in outs:
        ev, top = (res[1.0][n] + res[-1.0][n]) / 2, res[1.0][n].abs().max().item()
        kernel['tensors'][n] = dict(even_max=sig(ev.abs().max() / top), even_rms=sig((ev ** 2).mean().sqrt() / top), even_mean=sig(ev.mean() / top))
    print(kernel, flush=True)
    old = json.load(open(out_path)) if os.path.exists(out_path) else dict(rows=[], backward_tensors=[])
    old['rows'] += rows
    old['backward_tensors'].append(kernel)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(old, open(out_path, 'w'))


if __name__ == '__main__':
    main(sys.argv[1])
