"""Old against new, bit for bit, for a change that must not move a result of the reflectance inference kernels: two builds of the
library -- `--old` (e.g. the parent commit's) and `--new` (default: the tree's) -- are loaded through VQN_LIB in a child process each,
on the same seeded inputs, and the sha256 of every output is compared:

  * vqn_mlp_chain_fwd / _f16s     the shipped encoder, head and encoder + heads programs, as 4-wave and as 8-wave programs, N in CHAIN_N
  * vqn_mlp_chain_vq_fwd          encoder + main heads -> VQ step -> VQ heads, K in FRONT_K, N in FRONT_N, with and without z / ste
  * vqn_vq_assign                 D x K x N of VQ_D, VQ_K, VQ_N; plain, with a code mask (the MAXONLY pass, K > 16 on the f32 kernel),
                                  with the distance output
  * vqn_vq_quantize_rows(_train)  the same shapes (D <= 256), plain and masked, the train form with and without the normalised rows

Expected verdict: byte-equal.  Writes {verdict, n_arrays, n_cases, cases, different, missing} as JSON (--out).

    python scripts/compare_chain_kernels.py --old /tmp/libvqnerf_hip_parent.so --out /tmp/chain_same_bits.json"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.compare_train_kernels import sha  # noqa: E402

CHAIN_N = (1, 31, 33, 257)
FRONT_K, FRONT_N = (15, 16, 33, 64), (31, 4097)
VQ_D, VQ_K, VQ_N = (16, 60, 256), (15, 16, 17, 33, 64), (1, 17, 4097)


def child(out_path):
    import numpy as np
    import torch
    from tests.decomp_util import make_config, shipped_chain_programs
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    H = {}
    model = get_model_class('vq_nfr')(make_config())
    model.build_nets(device='cuda', seed=5).to('cuda')
    gen = torch.Generator(device='cuda').manual_seed(5)
    with torch.no_grad():                                         # (biases start at zero: move every parameter)
        for prm in model.parameters():
            prm.add_(0.05 * torch.randn(prm.shape, device='cuda', generator=gen))
    rng = np.random.default_rng(11)
    xyz = torch.tensor(rng.uniform(-1, 1, (max(CHAIN_N + FRONT_N), 3)).astype(np.float32)).cuda()
    rows = torch.tensor(rng.uniform(0, 1, (max(CHAIN_N), 256)).astype(np.float32)).cuda()

    # ---- the plain chain kernels, both engines: the model's own programs
    programs = {(mode, name): (pack, ws) for mode, name, pack, ws in shipped_chain_programs(model)}
    for (mode, name), ((wbuf, desc), ws) in programs.items():
        x = xyz if int(desc[1]) == 1 else rows
        for n_waves in (4, 8):
            d = desc.copy()
            if n_waves == 4 and d[7] != 4:
                continue                                          # (a program that needs the whole CU's LDS)
            d[7] = n_waves
            for N in CHAIN_N:
                for i, t in enumerate(_C.mlp_chain_fwd(d, wbuf, x[:N].contiguous(), ws, mode=mode)):
                    H[f'chain_{mode}/{name}/waves{n_waves}/N{N}/out{i}'] = sha(t)

    # ---- the fused front
    ((wa, da), widths_a), ((wb, db), widths_b) = programs['f32', 'enc_heads_main'], programs['f32', 'heads_vq']
    for K in FRONT_K:
        C = torch.tensor(np.random.default_rng(K).uniform(-1, 1, (256, K)).astype(np.float32)).cuda()
        C = (C / C.norm(dim=0, keepdim=True)).contiguous()
        frags = _C.vq_codebook_frags(C)
        for N in FRONT_N:
            for opt in (False, True):
                oa, ob, idx, ste, loss, counts = _C.mlp_chain_vq_fwd(da, wa, widths_a, db, wb, widths_b,
                                                                     xyz[:N].contiguous(), frags, K, want_z=opt, want_ste=opt)
                tag = f'front/K{K}/N{N}/{"z+ste" if opt else "plain"}'
                for k, t in [(f'a{i}', t) for i, t in enumerate(oa)] + [(f'b{i}', t) for i, t in enumerate(ob)] + \
                        [('idx', idx), ('ste', ste), ('loss', loss), ('counts', counts)]:
                    if t is not None:
                        H[f'{tag}/{k}'] = sha(t)

    # ---- the VQ entry points
    for D in VQ_D:
        for K in VQ_K:
            g = np.random.default_rng(1000 * D + K)
            C = torch.tensor(g.uniform(-1, 1, (D, K)).astype(np.float32)).cuda()
            mask = torch.tensor((np.arange(K) % 3 != 1).astype(np.float32)).cuda()
            for N in VQ_N:
                x = torch.tensor(g.normal(size=(N, D)).astype(np.float32)).cuda()
                tag = f'vq/D{D}/K{K}/N{N}'
                for how, kw in (('plain', {}), ('mask', dict(sel_mask=mask)), ('dist', dict(want_dist=True))):
                    for k, t in zip(('idx', 'quant', 'dist'), _C.vq_assign(x, C, **kw)):
                        if t is not None:
                            H[f'{tag}/assign.{how}/{k}'] = sha(t)
                for how, kw in (('plain', {}), ('mask', dict(sel_mask=mask))):
                    for form, kw2 in (('rows', {}), ('train', dict(want_xnorm=True)), ('train_no_ste', dict(want_xnorm=True, want_ste=False))):
                        for k, t in zip(('idx', 'ste', 'loss', 'counts', 'xnorm'), _C.vq_quantize_rows(x, C, **kw, **kw2)):
                            if t is not None:
                                H[f'{tag}/quantize_{form}.{how}/{k}'] = sha(t)
    torch.cuda.synchronize()
    with open(out_path, 'w') as f:
        json.dump(H, f, indent=0, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', required=True)
    ap.add_argument('--new', default=os.path.join(ROOT, 'vqnerf_release_amd', 'lib', 'libvqnerf_hip.so'))
    ap.add_argument('--out', default=os.path.join(tempfile.gettempdir(), 'chain_same_bits.json'))
    ap.add_argument('--child')
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    got = {}
    for which, lib in (('old', args.old), ('new', args.new)):
        env = dict(os.environ, VQN_LIB=os.path.abspath(lib))
        path = args.out + f'.{which}.json'
        subprocess.run([sys.executable, os.path.abspath(__file__), '--old', args.old, '--child', path], env=env, cwd=ROOT, check=True, timeout=240)
        got[which] = json.load(open(path))
    keys = sorted(set(got['old']) | set(got['new']))
    missing = [k for k in keys if k not in got['old'] or k not in got['new']]
    different = [k for k in keys if k not in missing and got['old'][k] != got['new'][k]]
    verdict = 'byte-equal' if not missing and not different else 'DIFFERENT'
    cases = sorted({k.rsplit('/', 1)[0] for k in keys})
    res = dict(old=args.old, new=args.new, verdict=verdict, n_arrays=len(keys), n_cases=len(cases), different=different, missing=missing, cases=cases)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(verdict=verdict, n_arrays=len(keys), n_cases=len(cases), different=different[:20], missing=missing[:20])))
    return 0 if verdict == 'byte-equal' else 1


if __name__ == '__main__':
    sys.exit(main())
