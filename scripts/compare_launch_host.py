"""Old against new, bit for bit, for a change of the kernels' HOST sides (grid sizing, the dynamic-LDS opt-in, the dispatch of a runtime int
to a template argument; csrc/launch.h, csrc/vq_plan.h) that must not move a result: two builds of the library -- `--old` (e.g. the
parent commit's) and `--new` (default: the tree's) -- are loaded through VQN_LIB in a fresh child process each, on the same seeded
inputs, and the sha256 of every output is compared:

  * everything scripts/compare_chain_kernels.py hashes   vqn_mlp_chain_fwd(_f16s), vqn_mlp_chain_vq_fwd, vqn_vq_assign, vqn_vq_quantize_rows(_train)
  * everything scripts/compare_train_kernels.py hashes   the NeuS x3 point kernels, vqn_neus_train_fwd / _bwd (both engines),
                                                         vqn_refl_train_fwd_x3 / _bwd_x3 at VQN_REFL_NIMG = 1 and 2, the contractions
  * vqn_vq_assign above the LDS opt-in, the split kernel at both tile counts, vqn_vq_ema_stats in every form, code usage alone,
    vqn_vq_ste_loss, vqn_l2_normalize_rows, vqn_vq_codebook_frags                 the small shapes of tests/test_gpu_vq.py
    (the single-pass form of the statistics adds with float atomics in no fixed order: its counts are hashed, its sums are
    compared with their float64 values to 1e-5, as tests/test_gpu_vq.py does)
  * vqn_tile_program (the 'prog' training engine of tests/neus_train_cases.py) and vqn_tile_program_grid
  * vqn_neus_sdf_points / vqn_neus_fine_points of the f32 and the f16s engines (the x3 ones: above), vqn_neus_upsample
  * vqn_brdf_shade_fwd / _bwd at L in {256, 512, 1024}, one and two material sets, with and without probes
  * vqn_decomp_loss_fwd / _bwd, vqn_clip_preserve, vqn_ks_split_fwd / _bwd, vqn_loss_total, vqn_linear2srgb
  * the integers of vqn_vq_ema_stats_ws_bytes, vqn_vq_assign_variant, vqn_brdf_shade_bwd_partials, vqn_tile_program_grid and the
    scratch-size queries over a sweep of shapes

Expected verdict: byte-equal.  Writes {verdict, n_arrays, n_cases, cases, different, missing, compared_to_tolerance_not_hashed,
tolerance_verdicts} as JSON (--out).

    python scripts/compare_launch_host.py --old /tmp/libvqnerf_hip_parent.so --out /tmp/launch_host_same_bits.json"""
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

ASSIGN = ((17, 256, 64, True), (17, 256, 128, True), (17, 64, 17, False), (17, 256, 33, False), (1, 256, 15, False))     # N, D, K, want_dist
EMA = ((1, 64, 5), (17, 64, 20), (4099, 64, 40), (1, 20, 40), (500, 20, 40), (333, 252, 64), (0, 256, 15), (2048, 256, 64))
SHADE_N = (1, 37)
ELEMENTWISE_N = (1, 1000, 70001)


def child(out_path):
    import numpy as np
    import torch
    from scripts import compare_chain_kernels, compare_train_kernels
    from tests import neus_train_cases as nc
    from vqnerf_release_amd import _C
    H = {}

    def say(what):                                   # (progress: the two borrowed children alone take minutes)
        print(f'[{os.path.basename(os.environ.get("VQN_LIB", "tree"))}] {what}', file=sys.stderr, flush=True)

    for mod in (compare_chain_kernels, compare_train_kernels):
        say(mod.__name__)
        mod.child(out_path + '.part')
        H.update({f'{mod.__name__.rsplit(".", 1)[-1]}/{k}': v for k, v in json.load(open(out_path + '.part')).items()})
        os.remove(out_path + '.part')
    lib = _C.lib()

    def rand(gen, *shape):
        return torch.rand(shape, device='cuda', generator=gen)

    say('VQ')
    # ---- VQ
    for N, D, K, want_dist in ASSIGN:
        gen = torch.Generator(device='cuda').manual_seed(N + D + K)
        x, C = rand(gen, N, D), rand(gen, D, K)
        idx, quant, dist = _C.vq_assign(x, C, want_quant=True, want_dist=want_dist)
        tag = f'vq_assign/N{N}_D{D}_K{K}_dist{int(want_dist)}'
        H[f'{tag}/idx'], H[f'{tag}/quant'] = sha(idx), sha(quant)
        if want_dist:
            H[f'{tag}/dist'] = sha(dist)
        H[f'{tag}/variant'] = str(_C.vq_assign_variant(D, K, has_dist=want_dist))
        if D <= 256:
            for k, t in enumerate(_C.vq_quantize_rows(x, C, want_xnorm=True)):
                if t is not None:
                    H[f'{tag}/quantize_rows_train.{k}'] = sha(t)
    for N, D, K in EMA:
        gen = torch.Generator(device='cuda').manual_seed(N + D + K)
        x = rand(gen, N, D)
        idx = torch.randint(0, K, (N,), device='cuda', generator=gen)
        counts, dw = _C.vq_ema_stats(x, idx, K)
        tag = f'vq_ema_stats/N{N}_D{D}_K{K}'
        H[f'{tag}/counts'], H[f'{tag}/counts_only'] = sha(counts), sha(_C.vq_counts(idx, K))
        if lib.vqn_vq_ema_stats_ws_bytes(N, D, K) > 0 or N == 0:
            H[f'{tag}/dw'] = sha(dw)
        else:               # the single-pass form sums with float atomics, in no fixed order: the same sums, not the same bits
            want = torch.zeros((K, D), dtype=torch.float64, device='cuda').index_add_(0, idx, x.double()).t()
            H[f'{tag}/dw_within_1e-5_of_float64'] = str(bool(torch.allclose(dw.double(), want, rtol=1e-5, atol=1e-6)))
        q = rand(gen, N, D)
        if N:
            ste, loss = _C.vq_ste_loss(x, q)
            H[f'{tag}/ste'], H[f'{tag}/loss'], H[f'{tag}/l2_normalize_rows'] = sha(ste), sha(loss), sha(_C.l2_normalize_rows(x))
    for K in (5, 20, 64):
        gen = torch.Generator(device='cuda').manual_seed(K)
        H[f'vq_codebook_frags/K{K}/frags'] = sha(_C.vq_codebook_frags(rand(gen, 256, K)))

    say('tile programs')
    # ---- the tile-program interpreter: the 'prog' training engine
    from vqnerf_release_amd.geo.train_programs import NeusCoreFunction
    for k, v in nc.ENGINES['prog'].items():
        os.environ[k] = v
    for shape in ('w64', 'w200'):
        eng = nc.build_engine(shape, 'cuda')
        params = [[t.cuda() for t in ts] for ts in nc.effective_params(shape)]
        for P in nc.POINTS:
            ref = nc.reference(shape, P)
            x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
            adj = tuple(ref[k].cuda() for k in ('g_rgb', 'g_n', 'g_sdf'))
            leaves = [t.clone().requires_grad_(True) for ts in params for t in ts]
            sdf_o, n_o, rgb_o = NeusCoreFunction.apply(eng, x, dirs, *leaves)
            nc.loss_of(sdf_o, n_o, rgb_o, adj).backward()
            tag = f'tile_program/{shape}/P{P}'
            for k, t in (('sdf', sdf_o), ('n', n_o), ('rgb', rgb_o)):
                H[f'{tag}/{k}'] = sha(t)
            for k, t in zip(nc.grad_names(shape), leaves):
                H[f'{tag}/grad.{k}'] = sha(t.grad)
    for k in nc.ENGINES['prog']:
        os.environ.pop(k, None)

    say('NeuS points')
    # ---- NeuS point kernels, f32 and f16s (the x3 engine: compare_train_kernels), and the up-sampling step
    for shape in ('shipped',):
        sdf, col = nc.build_modules(shape, 'cuda')
        for mode in ('f32', 'f16s'):
            wb_s, d_s = sdf.packs(max_tiles=col.max_tiles(), mode=mode)
            wb_c, d_c = col.packs(feat_tiles=sdf.plan(mode=mode).tiles[-1], mode=mode)
            for P in nc.POINTS:
                ref = nc.reference(shape, P)
                x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
                H[f'points_{mode}/{shape}/P{P}/sdf_points'] = sha(_C.neus_sdf_points(d_s, wb_s, pts=x, mode=mode))
                for k, t in zip(('sdf', 'grad', 'rgb'), _C.neus_fine_points(d_s, wb_s, d_c, wb_c, pts=x, dirs=dirs, mode=mode)):
                    H[f'points_{mode}/{shape}/P{P}/fine.{k}'] = sha(t)
    for B in (1, 24, 5000):
        gen = torch.Generator(device='cuda').manual_seed(B)
        o, d = rand(gen, B, 3) - 0.5, torch.nn.functional.normalize(rand(gen, B, 3) - 0.5, dim=1)
        z = torch.sort(rand(gen, B, 64) * 2.0, dim=1).values.contiguous()
        sdf_v = (rand(gen, B, 64) - 0.5).contiguous()
        u = torch.linspace(1.0 / 32, 1.0 - 1.0 / 32, 16, device='cuda')
        H[f'neus_upsample/B{B}/z_new'] = sha(_C.neus_upsample(o.contiguous(), d.contiguous(), z, sdf_v, 1.0, 64.0, u))

    say('shading')
    # ---- shading, forward and backward
    for L in (256, 512, 1024):
        for N in SHADE_N:
            gen = torch.Generator(device='cuda').manual_seed(L + N)
            xyz, rayo = rand(gen, N, 3) - 0.5, rand(gen, N, 3) + 1.0
            normal = torch.nn.functional.normalize(rand(gen, N, 3) - 0.5, dim=1).contiguous()
            lvis, lxyz, lareas, light = rand(gen, N, L), (rand(gen, L, 3) - 0.5) * 20.0, rand(gen, L) * 0.01, rand(gen, L, 3)
            mats = [(rand(gen, N, 3), rand(gen, N, 3) * 0.2, rand(gen, N, 1) * 0.8 + 0.1) for _ in range(2)]
            probes = rand(gen, 3, L, 3)
            for n_sets in (1, 2):
                for pr in (None, probes):
                    out = _C.brdf_shade_fwd(xyz, normal, rayo, lvis, lxyz, lareas, light, mats[:n_sets], raw=True, probes=pr)
                    tag = f'brdf_shade/L{L}_N{N}_sets{n_sets}_probes{int(pr is not None)}'
                    for i, t in enumerate(out['rgb']):
                        H[f'{tag}/rgb{i}'] = sha(t)
                    H[f'{tag}/normal'] = sha(out['normal'])
                    if pr is not None:
                        H[f'{tag}/rgb_probes'] = sha(out['rgb_probes'])
                g_sums = [rand(gen, N, 3) for _ in range(n_sets)]
                outs, g_light = _C.brdf_shade_bwd(xyz, normal, rayo, lvis, lxyz, lareas, light, mats[:n_sets], g_sums)
                for i, o3 in enumerate(outs):
                    for j, t in enumerate(o3):
                        H[f'brdf_shade_bwd/L{L}_N{N}_sets{n_sets}/g{i}.{j}'] = sha(t)
                H[f'brdf_shade_bwd/L{L}_N{N}_sets{n_sets}/g_light'] = sha(g_light)

    say('loss, element-wise')
    # ---- the loss pass and the element-wise pieces
    w = dict(rgb=1.0, chr=0.5, smooth=0.1, alpha=60.0, thres=0.02, lambert=0.01)
    for N in ELEMENTWISE_N:
        gen = torch.Generator(device='cuda').manual_seed(N)
        pred, vq, gt, z, spec, rough = rand(gen, N, 3), rand(gen, N, 3), rand(gen, N, 3), rand(gen, N, 32), rand(gen, N, 3), rand(gen, N, 1)
        terms = _C.decomp_loss_fwd(pred, vq, gt, z, spec, rough, False, w)
        H[f'decomp_loss/N{N}/terms'] = sha(terms)
        for k, t in enumerate(_C.decomp_loss_bwd(pred, vq, gt, z, spec, rough, False, w, rand(gen, N, 5))):
            H[f'decomp_loss/N{N}/g{k}'] = sha(t)
        H[f'elementwise/N{N}/clip_preserve'] = sha(_C.clip_preserve(pred * 3.0 - 1.0, 0.0, 1.0))
        H[f'elementwise/N{N}/linear2srgb'] = sha(_C.linear2srgb(pred * 1.5 - 0.25))
        ks = rand(gen, N, 1)
        for k, t in enumerate(_C.ks_split_fwd(pred, ks)):
            H[f'elementwise/N{N}/ks_split_fwd.{k}'] = sha(t)
        for k, t in enumerate(_C.ks_split_bwd(pred, ks, vq, gt)):
            H[f'elementwise/N{N}/ks_split_bwd.{k}'] = sha(t)
        H[f'elementwise/N{N}/loss_total'] = sha(_C.loss_total(terms, rand(gen, 1), rand(gen, 1), True, True, True))

    say('integers')
    # ---- the integers
    ints = {}
    for N in (0, 1, 17, 333, 500, 2048, 4099, 5000, 100003, 3000000):
        ints[f'shade_bwd_partials/N{N}'] = int(lib.vqn_brdf_shade_bwd_partials(N))
        for D in (4, 20, 32, 64, 128, 252, 256, 320, 1024):
            for K in (1, 5, 15, 16, 17, 32, 33, 40, 64, 65, 128):
                ints[f'ema_ws_bytes/N{N}_D{D}_K{K}'] = int(lib.vqn_vq_ema_stats_ws_bytes(N, D, K))
    for D in (4, 64, 252, 256, 260, 512):
        for K in (1, 16, 17, 32, 33, 64, 65, 128, 129):
            for f in range(4):
                ints[f'assign_variant/D{D}_K{K}_f{f}'] = int(lib.vqn_vq_assign_variant(D, K, f & 1, f >> 1))
    for k, v in nc.ENGINES['prog'].items():
        os.environ[k] = v
    for shape in ('w64', 'w200'):
        eng = nc.build_engine(shape, 'cuda')
        for name, (desc, _) in eng._static(torch.device('cuda'))[2].items():
            for N in (1, 33, 5000, 16384, 1000000):
                ints[f'tile_program_grid/{shape}/{name}/N{N}'] = int(_C.tile_program_grid(desc, N))
    for k in nc.ENGINES['prog']:
        os.environ.pop(k, None)
    for shape in ('shipped', 'w200'):
        sdf, col = nc.build_modules(shape, 'cuda')
        _, d_s = sdf.packs(max_tiles=col.max_tiles())
        ints[f'scratch_bytes/{shape}/neus_fine'] = int(_C._scratch_bytes('vqn_neus_fine_scratch_bytes', _C._host(d_s)))

    def host_desc(d):
        return _C._host(d.cpu().numpy() if torch.is_tensor(d) else d)

    for shape in ('shipped', 'w200'):
        eng = nc.build_engine(shape, 'cuda')
        dev = torch.device('cuda', torch.cuda.current_device())
        ints[f'scratch_bytes/{shape}/neus_train_bwd'] = int(_C._scratch_bytes('vqn_neus_train_bwd_scratch_bytes', host_desc(eng._bwd_static(dev)[-1])))
        ints[f'scratch_bytes/{shape}/neus_train_bwd_x3'] = int(_C._scratch_bytes('vqn_neus_train_bwd_x3_scratch_bytes',
                                                                                 host_desc(eng._bwd_static(dev, 'x3')[-1])))
    from tests.decomp_util import make_config
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.refl_train import ReflStackEngine
    m = get_model_class('vq_nfr')(make_config())
    m.build_nets(device='cuda', seed=5).to('cuda')
    for tag, reng in (('enc_heads', ReflStackEngine([m.net['fine_enc'], m.net['bottleneck']], m.embedder['xyz'].n_freqs,
                                                    [m.net[n] for n in ('diff_main', 'spec_main', 'rough_main')], m.z_dim, 'cuda')),
                      ('heads', ReflStackEngine(None, 0, [m.net[n] for n in ('diff_vq', 'spec_vq', 'rough_vq')], m.z_dim, 'cuda'))):
        ints[f'scratch_bytes/refl_{tag}/refl_train_bwd_x3'] = int(_C._scratch_bytes('vqn_refl_train_bwd_x3_scratch_bytes', host_desc(reng._static()[-1])))
    H.update({f'ints/{k}': str(v) for k, v in ints.items()})
    torch.cuda.synchronize()
    with open(out_path, 'w') as f:
        json.dump(H, f, indent=0, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', required=True)
    ap.add_argument('--new', default=os.path.join(ROOT, 'vqnerf_release_amd', 'lib', 'libvqnerf_hip.so'))
    ap.add_argument('--out', default=os.path.join(tempfile.gettempdir(), 'launch_host_same_bits.json'))
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
    keys = sorted(set(got['old']) | set(got['new']))
    missing = [k for k in keys if k not in got['old'] or k not in got['new']]
    different = [k for k in keys if k not in missing and got['old'][k] != got['new'][k]]
    verdict = 'byte-equal' if not missing and not different else 'DIFFERENT'
    cases = sorted({k.rsplit('/', 1)[0] for k in keys if not k.startswith('ints/')}) + ['ints']
    # not hashed: sums of float atomics, held in each child to 1e-5 of their float64 values (the recorded value is that verdict)
    tolerance = [k for k in keys if k.endswith('_within_1e-5_of_float64')]
    res = dict(old=os.path.basename(args.old), new=os.path.basename(args.new), verdict=verdict, n_arrays=len(keys), n_cases=len(cases),
               different=different, missing=missing, compared_to_tolerance_not_hashed=tolerance,
               tolerance_verdicts={k: [got['old'][k], got['new'][k]] for k in tolerance if k not in missing}, cases=cases)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(verdict=verdict, n_arrays=len(keys), n_cases=len(cases), different=different[:20], missing=missing[:20])))
    return 0 if verdict == 'byte-equal' else 1


if __name__ == '__main__':
    sys.exit(main())
