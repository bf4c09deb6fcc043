"""Dev probe: per-kernel breakdown of one geo training step (not the bench contract).
`probe_train.py --host`: wall time per call at the smallest sizes, where the host side dominates -- the NeuS point kernels of the three
engines, the training forward + backward of the x3, fused and interpreted engines, the reflectance stack at one and two images per
workgroup, the fused reflectance front, the loss pass, the element-wise pieces and the up-sampling step."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def host_legs():
    from tests import neus_train_cases as nc
    from tests.decomp_util import make_config
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo.train_programs import NeusCoreFunction
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.refl_train import ReflStackEngine, ReflStackFunction

    def t_host(name, fn, n):
        """wall time per call, microseconds: n calls back to back, one synchronisation at the end"""
        for _ in range(3): fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n): fn()
        torch.cuda.synchronize()
        print(f'host {name}: {(time.perf_counter() - t0) / n * 1e6:.2f} us/call', flush=True)

    shape, P = 'shipped', 1
    ref = nc.reference(shape, P)
    x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
    sdf, col = nc.build_modules(shape, 'cuda')
    for mode in ('f32', 'f16s', 'x3'):
        wb_s, d_s = sdf.packs(max_tiles=col.max_tiles(), mode=mode)
        wb_c, d_c = col.packs(feat_tiles=sdf.plan(mode=mode).tiles[-1], mode=mode)
        t_host(f'neus_sdf_points {mode} P={P}', lambda: _C.neus_sdf_points(d_s, wb_s, pts=x, mode=mode), 300)
        t_host(f'neus_fine_points {mode} P={P}', lambda: _C.neus_fine_points(d_s, wb_s, d_c, wb_c, pts=x, dirs=dirs, mode=mode), 300)
    adj = tuple(ref[k].cuda() for k in ('g_rgb', 'g_n', 'g_sdf'))
    for engine in ('x3', 'fused', 'prog'):
        for k, v in nc.ENGINES[engine].items():
            os.environ[k] = v
        eng = nc.build_engine(shape, 'cuda')
        leaves = [t.cuda().clone().requires_grad_(True) for ts in nc.effective_params(shape) for t in ts]

        def step():
            for t in leaves:
                t.grad = None
            nc.loss_of(*NeusCoreFunction.apply(eng, x, dirs, *leaves), adj).backward()
        t_host(f'neus train fwd+bwd {engine} P={P}', step, 30)
        for k in nc.ENGINES[engine]:
            os.environ.pop(k, None)
    m = get_model_class('vq_nfr')(make_config())
    m.build_nets(device='cuda', seed=5).to('cuda')
    names = ['diff_main', 'spec_main', 'rough_main']
    pts = torch.tensor([[0.3, -0.4, 0.5]], device='cuda')
    for nimg in ('1', '2'):
        os.environ['VQN_REFL_NIMG'] = nimg
        reng = ReflStackEngine([m.net['fine_enc'], m.net['bottleneck']], m.embedder['xyz'].n_freqs, [m.net[n] for n in names], m.z_dim, 'cuda')

        def rstep():
            m.zero_grad(set_to_none=True)
            sum(o.sum() for o in ReflStackFunction.apply(reng, pts, *reng.params())).backward()
        t_host(f'refl_train fwd+bwd nimg={nimg} N=1', rstep, 30)
    os.environ.pop('VQN_REFL_NIMG')
    from tests.decomp_util import shipped_chain_programs
    programs = {(mode, name): (pack, ws) for mode, name, pack, ws in shipped_chain_programs(m)}
    ((wa, da), widths_a), ((wb, db), widths_b) = programs['f32', 'enc_heads_main'], programs['f32', 'heads_vq']
    row = torch.rand(1, 256, device='cuda')
    for (mode, name), ((wbuf, desc), ws) in programs.items():          # (input mode 1: positions; else rows of 256 features)
        xin = pts if int(desc[1]) == 1 else row
        t_host(f'mlp_chain_fwd {mode} {name} N=1', lambda: _C.mlp_chain_fwd(desc, wbuf, xin, ws, mode=mode), 300)
    for K in (15, 64):
        C = torch.nn.functional.normalize(torch.rand(256, K, device='cuda'), dim=0).contiguous()
        frags = _C.vq_codebook_frags(C)
        t_host(f'mlp_chain_vq_fwd K={K} N=1', lambda: _C.mlp_chain_vq_fwd(da, wa, widths_a, db, wb, widths_b, pts, frags, K), 300)
    g = torch.Generator(device='cuda').manual_seed(0)
    R = lambda *s: torch.rand(s, device='cuda', generator=g)
    w = dict(rgb=1.0, chr=0.5, smooth=0.1, alpha=60.0, thres=0.02, lambert=0.01)
    pred, vq, gt, z, spec, rough, ks = R(1, 3), R(1, 3), R(1, 3), R(1, 32), R(1, 3), R(1, 1), R(1, 1)
    terms = _C.decomp_loss_fwd(pred, vq, gt, z, spec, rough, False, w)
    t_host('decomp_loss_fwd N=1', lambda: _C.decomp_loss_fwd(pred, vq, gt, z, spec, rough, False, w), 1000)
    t_host('decomp_loss_bwd N=1', lambda: _C.decomp_loss_bwd(pred, vq, gt, z, spec, rough, False, w, terms), 1000)
    t_host('clip_preserve N=1', lambda: _C.clip_preserve(pred, 0.0, 1.0), 1000)
    t_host('ks_split_fwd N=1', lambda: _C.ks_split_fwd(pred, ks), 1000)
    t_host('linear2srgb N=1', lambda: _C.linear2srgb(pred), 1000)
    o, d = R(1, 3) - 0.5, torch.nn.functional.normalize(R(1, 3) - 0.5, dim=1).contiguous()
    zz, sv = torch.sort(R(1, 64) * 2.0, dim=1).values.contiguous(), R(1, 64) - 0.5
    u = torch.linspace(1.0 / 32, 1.0 - 1.0 / 32, 16, device='cuda')
    t_host('neus_upsample B=1', lambda: _C.neus_upsample(o, d, zz, sv, 1.0, 64.0, u), 1000)


if '--host' in sys.argv:
    host_legs()
    sys.exit(0)
import bench
from vqnerf_release_amd import _C
from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork, SingleVarianceNetwork
from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
from vqnerf_release_amd.geo.nerf_runner import SyntheticDataset

dev = torch.device('cuda')
torch.manual_seed(0)
sdf, col, var = SDFNetwork(**bench.FULL['sdf']).to(dev), RenderingNetwork(**bench.FULL['color']).to(dev), SingleVarianceNetwork(0.3).to(dev)
ren = NeuSRenderer(None, sdf, var, col, **bench.FULL['renderer'])
B = int(sys.argv[1]) if len(sys.argv) > 1 else 2560
ds = SyntheticDataset(device=dev, n_images=8)
opt = torch.optim.Adam(list(sdf.parameters()) + list(var.parameters()) + list(col.parameters()), lr=5e-4)
bg = torch.ones(1, 3, device=dev)

def step():
    data = ds.gen_random_rays_at(0, B)
    o, d, rgb, mask = data[:, :3].contiguous(), data[:, 3:6].contiguous(), data[:, 6:9], data[:, 9:10]
    near, far = ds.near_far_from_sphere(o, d)
    opt.zero_grad(set_to_none=True)
    r = ren.render(o, d, near, far, 2.0, background_rgb=bg, cos_anneal_ratio=1.0)
    loss = ((r['color_fine'] - rgb) * mask).abs().sum() / (mask.sum() + 1e-5) + 0.1 * r['gradient_error'] \
        + 0.1 * torch.nn.functional.binary_cross_entropy(r['weight_sum'].clip(1e-3, 1 - 1e-3), mask)
    loss.backward()
    opt.step()

for _ in range(2):
    step()
torch.cuda.synchronize()
_C.KernelClock.reset(True)
t0 = time.perf_counter()
n = 5
for _ in range(n):
    step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
clk = _C.KernelClock.summary()
print(f'B={B}: {dt*1e3:.2f} ms/step  {B/dt:.0f} rays/s')
tot = 0
for k, (c, ms) in sorted(clk.items(), key=lambda kv: -kv[1][1]):
    print(f'  {k:40s} {c//n:4d} launches/step  {ms/n:8.3f} ms/step')
    tot += ms / n
print(f'  sum of timed kernels {tot:.2f} ms; rest (torch ops, host) {dt*1e3 - tot:.2f} ms')
