"""Old against new, bit for bit, for a change that must not move a result of the training kernels: two builds of the library -- `--old`
(e.g. the parent commit's, built beside the tree as lib/libvqnerf_hip_parent.so) and `--new` (default: the tree's) -- are loaded through
VQN_LIB in a child process each, on the same seeded inputs, and the sha256 of every output is compared:

  * vqn_neus_sdf_points_x3 / vqn_neus_fine_points_x3                          tests/neus_train_cases.py: shapes x POINTS
  * vqn_neus_train_fwd(_x3), vqn_neus_train_bwd(_x3), the batched contraction  the same, engines x3 and fused, every tensor of the engine
  * vqn_refl_train_fwd_x3 / _bwd_x3, one and two images per workgroup          the stacks and batch sizes of tests/test_gpu_refl_train.py
  * vqn_wgrad_partials / _x3 / _batched                                        tests/wgrad_cases.py: PARTIAL_CASES, real operands
  * optionally (--bench-dump) `bench.py --mode train --dump-outputs` at the workload's size

Expected verdict: byte-equal.  Writes {verdict, n_arrays, different, missing, arrays} as JSON (--out).

    python scripts/compare_train_kernels.py --old vqnerf_release_amd/lib/libvqnerf_hip_parent.so --out /tmp/same_bits.json"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sha(t):
    import numpy as np
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, 'detach') else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()[:24] + f':{a.dtype}{list(a.shape)}'


def child(out_path):
    import numpy as np
    import torch
    from tests import neus_train_cases as nc
    from tests import wgrad_cases as wc
    from tests.decomp_util import make_config
    from vqnerf_release_amd import _C
    H = {}

    # ---- NeuS point kernels and training kernels
    from vqnerf_release_amd.geo.train_programs import NeusCoreFunction
    for shape, engines in nc.SHAPE_ENGINES.items():
        if 'x3' not in engines:
            continue
        sdf, col = nc.build_modules(shape, 'cuda')
        wb_s, d_s = sdf.packs(max_tiles=col.max_tiles(), mode='x3')
        wb_c, d_c = col.packs(feat_tiles=sdf.plan(mode='x3').tiles[-1], mode='x3')
        for P in nc.POINTS:
            ref = nc.reference(shape, P)
            x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
            H[f'points_x3/{shape}/P{P}/sdf_points'] = sha(_C.neus_sdf_points(d_s, wb_s, pts=x, mode='x3'))
            for k, t in zip(('sdf', 'grad', 'rgb'), _C.neus_fine_points(d_s, wb_s, d_c, wb_c, pts=x, dirs=dirs, mode='x3')):
                H[f'points_x3/{shape}/P{P}/fine.{k}'] = sha(t)
        for engine in ('x3', 'fused'):
            for k, v in nc.ENGINES[engine].items():
                os.environ[k] = v
            eng = nc.build_engine(shape, 'cuda')
            assert (eng.forward_mode(), eng.backward_mode()) == nc.MODES[engine]
            params = [[t.cuda() for t in ts] for ts in nc.effective_params(shape)]
            alloc, seen = eng.alloc_tensors, []

            def zeroed(P, device):                               # (torch.empty memory: what no kernel writes must not enter a hash)
                T = alloc(P, device)
                for k, t in T.items():
                    if k not in ('X', 'DIRS', 'ONES'):
                        t.zero_()
                seen.append(T)
                return T

            eng.alloc_tensors = zeroed
            for P in nc.POINTS:
                ref = nc.reference(shape, P)
                x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
                adj = tuple(ref[k].cuda() for k in ('g_rgb', 'g_n', 'g_sdf'))
                leaves = [t.clone().requires_grad_(True) for ts in params for t in ts]
                del seen[:]
                sdf_o, n_o, rgb_o = NeusCoreFunction.apply(eng, x, dirs, *leaves)
                nc.loss_of(sdf_o, n_o, rgb_o, adj).backward()
                tag = f'train_{engine}/{shape}/P{P}'
                for k, t in (('sdf', sdf_o), ('n', n_o), ('rgb', rgb_o)):
                    H[f'{tag}/{k}'] = sha(t)
                for k, t in zip(nc.grad_names(shape), leaves):
                    H[f'{tag}/grad.{k}'] = sha(t.grad)
                for i, T in enumerate(seen):                     # every tensor of the engine: saved tensors, adjoints, stashes
                    for k, t in T.items():
                        H[f'{tag}/T{i}.{k}'] = sha(t)
            for k in nc.ENGINES[engine]:
                os.environ.pop(k, None)

    # ---- reflectance stacks, both image forms
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.refl_train import ReflStackEngine, ReflStackFunction

    def model(seed):
        m = get_model_class('vq_nfr')(make_config())
        m.build_nets(device='cuda', seed=seed).to('cuda')
        g = torch.Generator(device='cuda').manual_seed(seed)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05 * torch.randn(p.shape, device='cuda', generator=g))
        return m

    def pts(N, seed):
        rng = np.random.default_rng(seed)
        x = rng.uniform(-1, 1, (N, 3))
        return torch.tensor(x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(0.4, 1.0, (N, 1)), dtype=torch.float32, device='cuda')

    for nimg in ('1', '2'):
        os.environ['VQN_REFL_NIMG'] = nimg
        for split in ('0', '1'):
            os.environ['VQN_REFL_SPLIT'] = split
            m = model(5)
            names = ['diff_main', 'spec_main', 'rough_main']
            eng = ReflStackEngine([m.net['fine_enc'], m.net['bottleneck']], m.embedder['xyz'].n_freqs, [m.net[n] for n in names], m.z_dim, 'cuda')
            for N in (1, 33, 600, 4113):
                g = torch.Generator(device='cuda').manual_seed(2)
                w_z = torch.randn(N, 256, device='cuda', generator=g)
                w_o = [torch.randn(N, m.net[n].widths[2], device='cuda', generator=g) for n in names]
                m.zero_grad(set_to_none=True)
                res = ReflStackFunction.apply(eng, pts(N, 1), *eng.params())
                ((res[0] * w_z).sum() + sum((o * w).sum() for o, w in zip(res[1:], w_o))).backward()
                tag = f'refl_A/nimg{nimg}/split{split}/N{N}'
                for i, t in enumerate(res):
                    H[f'{tag}/out{i}'] = sha(t)
                for i, p in enumerate(eng.params()):
                    H[f'{tag}/grad{i}'] = sha(p.grad)
            m = model(7)
            names = ['diff_vq', 'spec_vq', 'rough_vq']
            eng = ReflStackEngine(None, 0, [m.net[n] for n in names], m.z_dim, 'cuda')
            for N in (2, 95, 2048):
                g = torch.Generator(device='cuda').manual_seed(3)
                z0 = torch.nn.functional.normalize(torch.rand(N, 256, device='cuda', generator=g), dim=-1)
                w_o = [torch.randn(N, m.net[n].widths[2], device='cuda', generator=g) for n in names]
                m.zero_grad(set_to_none=True)
                z_b = z0.clone().requires_grad_(True)
                res = ReflStackFunction.apply(eng, z_b, *eng.params())
                sum((o * w).sum() for o, w in zip(res, w_o)).backward()
                tag = f'refl_B/nimg{nimg}/split{split}/N{N}'
                for i, t in enumerate(res):
                    H[f'{tag}/out{i}'] = sha(t)
                H[f'{tag}/grad_rows'] = sha(z_b.grad)
                for i, p in enumerate(eng.params()):
                    H[f'{tag}/grad{i}'] = sha(p.grad)
    os.environ.pop('VQN_REFL_NIMG')
    os.environ.pop('VQN_REFL_SPLIT')

    # ---- weight-gradient partial blocks: every case through the three entries, real operands
    for case, _ in wc.PARTIAL_CASES:
        a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt, npt, n_split, rowsum = case
        A, B = wc.real_operands(npt, a_tiles, b_tiles, seed=100 * a_nt + b_nt)
        A, B = A.cuda(), B.cuda()
        n = wc.n_blocks(npt, n_split)
        for x3 in (False, True):
            for batched in (False, True):
                ws = torch.zeros((n, a_nt * 32, b_nt * 32), device='cuda')
                rs = torch.zeros((n, a_nt * 32), device='cuda') if rowsum else None
                if batched:
                    got = _C.wgrad_partials_batched([A], [a_tiles], [a_t0], [a_nt], [B], [b_tiles], [b_t0], [b_nt], npt, n_split, [ws.data_ptr()],
                                                    [rs.data_ptr() if rowsum else None], x3)
                else:
                    got = _C.wgrad_partials(A, a_tiles, a_t0, a_nt, B, b_tiles, b_t0, b_nt, npt, n_split, ws.data_ptr(),
                                            rs.data_ptr() if rowsum else None, x3=x3)
                assert got == n
                tag = f'wgrad/{wc.case_id(case)}/{"x3" if x3 else "f32"}/{"batched" if batched else "single"}'
                H[f'{tag}/ws'] = sha(ws)
                if rowsum:
                    H[f'{tag}/rs'] = sha(rs)
    for x3 in (False, True):                                     # the 40-problem batched call of the tests, both point counts
        for npt in (7, 1025):
            probs, _ = wc.batched_problems(x3, npt)
            A, B = wc.real_operands(npt, wc.BATCH_A_TILES, wc.BATCH_B_TILES, seed=npt)
            A, B = A.cuda(), B.cuda()
            n = wc.n_blocks(npt, 3)
            ws = [torch.zeros((n, p[1] * 32, p[3] * 32), device='cuda') for p in probs]
            rs = [torch.zeros((n, p[1] * 32), device='cuda') if p[4] else None for p in probs]
            got = _C.wgrad_partials_batched([A] * len(probs), [wc.BATCH_A_TILES] * len(probs), [p[0] for p in probs], [p[1] for p in probs],
                                            [B] * len(probs), [wc.BATCH_B_TILES] * len(probs), [p[2] for p in probs], [p[3] for p in probs],
                                            npt, 3, [w.data_ptr() for w in ws], [r.data_ptr() if r is not None else None for r in rs], x3)
            assert got == n
            for i, (w, r) in enumerate(zip(ws, rs)):
                H[f'wgrad_batch40/{"x3" if x3 else "f32"}/npt{npt}/{i}/ws'] = sha(w)
                if r is not None:
                    H[f'wgrad_batch40/{"x3" if x3 else "f32"}/npt{npt}/{i}/rs'] = sha(r)
    torch.cuda.synchronize()
    with open(out_path, 'w') as f:
        json.dump(H, f, indent=0, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', required=True)
    ap.add_argument('--new', default=os.path.join(ROOT, 'vqnerf_release_amd', 'lib', 'libvqnerf_hip.so'))
    ap.add_argument('--out', default=os.path.join(tempfile.gettempdir(), 'same_bits.json'))
    ap.add_argument('--bench-dump', action='store_true', help='also compare bench.py --mode train --dump-outputs (two more bench runs)')
    ap.add_argument('--child')
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    got = {}
    for which, lib in (('old', args.old), ('new', args.new)):
        env = dict(os.environ, VQN_LIB=os.path.abspath(lib))
        path = args.out + f'.{which}.json'
        subprocess.run([sys.executable, os.path.abspath(__file__), '--old', args.old, '--child', path], env=env, cwd=ROOT, check=True, timeout=420)
        got[which] = json.load(open(path))
        if args.bench_dump:
            import numpy as np
            d = args.out + f'.{which}.dump'
            subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--mode', 'train', '--steps', '3', '--warmup', '1',
                            '--dump-outputs', d], env=env, cwd=ROOT, check=True, timeout=300, stdout=subprocess.DEVNULL)
            for name in sorted(os.listdir(d)):
                if name.endswith('.npy'):
                    got[which][f'bench_train_dump/{name[:-4]}'] = sha(np.load(os.path.join(d, name)))
    keys = sorted(set(got['old']) | set(got['new']))
    missing = [k for k in keys if k not in got['old'] or k not in got['new']]
    different = [k for k in keys if k not in missing and got['old'][k] != got['new'][k]]
    verdict = 'byte-equal' if not missing and not different else 'DIFFERENT'
    res = dict(old=args.old, new=args.new, verdict=verdict, n_arrays=len(keys), different=different, missing=missing, arrays=keys)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(verdict=verdict, n_arrays=len(keys), different=different[:20], missing=missing[:20])))
    return 0 if verdict == 'byte-equal' else 1


if __name__ == '__main__':
    sys.exit(main())
