"""Old against new, bit for bit, for a change of the training HOST side (the Python that packs, allocates, launches and contracts --
no kernel): two trees -- `--old` (a checkout of the parent commit) and `--new` (default: this tree) -- each run in a fresh child
process, one at a time, against the SAME library (VQN_LIB, default: this tree's), on the same seeded inputs.  Per case the sha256
of every output and parameter gradient and the table of C-ABI entry-point counts (tests/gpu_util.launches) are compared:

  * geometry     the 'full' nets of tests/test_gpu_neus_render._build and its 'small' ones (interpreter only) on 24 rays, the loss of
                 test_batched_weight_gradients_are_the_per_weight_sequence_bit_for_bit;
                 (VQN_TRAIN_FWD, VQN_TRAIN_BWD) in ENGINES x VQN_WGRAD_BATCH in {1, 0} x VQN_WGRAD in {bf16x3, f32}
  * reflectance  Trainer.train_iter on 300 points: VQN_REFL_TRAIN=prog with VQN_WGRAD_BATCH in {1, 0}, and the default engine

Expected verdict: every array byte-equal, every count equal.  Writes {verdict, n_arrays, n_cases, different, missing, cases, counts}
as JSON (--out).

    python scripts/compare_train_host.py --old /tmp/parent_checkout --out /tmp/train_host_same_bits.json"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENGINES = (('x3', 'x3'), ('fused', 'fused'), ('prog', 'prog'), ('x3', 'prog'))


def child(tree, out_path):
    sys.path.insert(0, tree)
    import hashlib
    import numpy as np          # noqa: F401
    import torch
    from oracle import decomp as od
    from oracle import geo as og
    from tests.decomp_util import make_config, load_oracle_params, make_batch
    from tests.gpu_util import launches
    from tests.test_gpu_neus_render import _build
    tp = importlib.import_module('vqnerf_release_amd.geo.train_programs')
    assert os.path.abspath(tp.__file__).startswith(os.path.abspath(tree) + os.sep), tp.__file__
    sw = tp if hasattr(tp, 'BATCHED_WGRAD') else importlib.import_module('vqnerf_release_amd.wgrad')      # where the tree keeps the switch

    def sha(t):
        a = t.detach().cpu().contiguous().numpy()
        return hashlib.sha256(a.tobytes()).hexdigest()[:24] + f':{a.dtype}{list(a.shape)}'

    H, C = {}, {}

    def record(tag, rec, arrays):
        C[tag] = {k: v for k, v in sorted(rec.counts.items()) if k.startswith('vqn_')}
        for k, t in arrays:
            H[f'{tag}/{k}'] = sha(t)

    for net in ('full', 'small'):
        cfg, sdf, col, var, ren = _build(net)
        o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(24, 5)]
        named = [(f'{m}.{k}', q) for m, mod in (('sdf', sdf), ('col', col), ('var', var)) for k, q in mod.named_parameters()]
        for fwd, bwd in ENGINES:
            os.environ['VQN_TRAIN_FWD'], os.environ['VQN_TRAIN_BWD'] = fwd, bwd
            for batched in (True, False):
                sw.BATCHED_WGRAD[0] = batched
                for wg in ('bf16x3', 'f32'):
                    tp.wgrad_mode(wg)
                    for _, q in named:
                        q.grad = None
                    with launches() as rec:
                        rr = ren.render(o, d, near, far, 2.0, perturb_overwrite=0, background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=1.0)
                        (rr['color_fine'].sum() + rr['gradient_error']).backward()
                    record(f'geo/{net}/fwd={fwd},bwd={bwd}/batch={int(batched)}/{wg}', rec,
                           [('color_fine', rr['color_fine']), ('gradient_error', rr['gradient_error'])] +
                           [('grad.' + k, q.grad) for k, q in named if q.grad is not None])
        os.environ.pop('VQN_TRAIN_FWD')
        os.environ.pop('VQN_TRAIN_BWD')
    tp.wgrad_mode(os.environ.get('VQN_WGRAD', 'bf16x3'))

    from vqnerf_release_amd.decomp.nerfactor import train_nfr
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    for engine, batched in (('prog', True), ('prog', False), (None, True)):
        if engine is None:
            os.environ.pop('VQN_REFL_TRAIN', None)
        else:
            os.environ['VQN_REFL_TRAIN'] = engine
        sw.BATCHED_WGRAD[0] = batched
        p, specs = od.make_model_params(seed=0, K=15)
        model = load_oracle_params(get_model_class('vq_nfr')(make_config(n_rays_per_step=256)), p, 'cuda')
        batch = make_batch(od.make_points(300, seed=11), 'cuda')
        model.get_codebook()
        _ = model.light
        tr = train_nfr.Trainer(model, torch.optim.SGD(model.trainable_variables, lr=0.0))
        with launches() as rec:
            tr.train_iter(batch, global_bs=300)
        record(f'refl/engine={engine or "default"}/batch={int(batched)}', rec,
               [(f'grad{i}', v.grad) for i, v in enumerate(model.trainable_variables) if v.grad is not None])
    torch.cuda.synchronize()
    with open(out_path, 'w') as f:
        json.dump(dict(arrays=H, counts=C), f, indent=0, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', required=True, help='a checkout of the parent commit')
    ap.add_argument('--new', default=ROOT)
    ap.add_argument('--lib', default=os.path.join(ROOT, 'vqnerf_release_amd', 'lib', 'libvqnerf_hip.so'), help='the one library both trees load')
    ap.add_argument('--out', default=os.path.join(tempfile.gettempdir(), 'train_host_same_bits.json'))
    ap.add_argument('--child')
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.old), args.child)
    args.out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    got = {}
    for which, tree in (('old', args.old), ('new', args.new)):
        tree = os.path.abspath(tree)
        env = dict(os.environ, VQN_LIB=os.path.abspath(args.lib))
        for k in ('VQN_TRAIN_FWD', 'VQN_TRAIN_BWD', 'VQN_WGRAD', 'VQN_WGRAD_BATCH', 'VQN_REFL_TRAIN', 'PYTHONPATH'):
            env.pop(k, None)
        path = args.out + f'.{which}.json'
        subprocess.run([sys.executable, os.path.abspath(__file__), '--old', tree, '--child', path], env=env, cwd=tree, check=True, timeout=540)
        got[which] = json.load(open(path))
    old, new = got['old']['arrays'], got['new']['arrays']
    keys = sorted(set(old) | set(new))
    missing = [k for k in keys if k not in old or k not in new]
    different = [k for k in keys if k not in missing and old[k] != new[k]]
    cases = sorted(set(got['old']['counts']) | set(got['new']['counts']))
    counts_differ = [c for c in cases if got['old']['counts'].get(c) != got['new']['counts'].get(c)]
    verdict = 'byte-equal, same entry-point counts' if not (missing or different or counts_differ) else 'DIFFERENT'
    res = dict(verdict=verdict, n_arrays=len(keys), n_cases=len(cases), different=different, missing=missing, counts_differ=counts_differ,
               cases=cases, counts=got['new']['counts'], counts_old={c: got['old']['counts'].get(c) for c in counts_differ})
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(verdict=verdict, n_arrays=len(keys), n_cases=len(cases), different=different[:20], missing=missing[:20],
                          counts_differ=counts_differ[:20])))
    return 0 if not (missing or different or counts_differ) else 1


if __name__ == '__main__':
    sys.exit(main())
