"""GPU: the weight-derived caches in front of the kernels (weight packs of every matrix mode, the x3 handle of a geo training render,
the codebook's MFMA fragments) against every kind of weight write.

A cache whose key misses a write makes the kernel compute a correct answer for the OLD weights: finite, plausible, and invisible to
every parity test that builds its model once.  So each cell of the model x writer matrix below takes a model with weights W, runs the
cached HIP path (`out0`), moves the weights to W' with one writer, runs the path again (`out1`) and asserts
  (a) `out1` equals, bit for bit, the output of a FRESH model given W' through `load_state_dict` (no cache ever built);
  (b) that fresh output agrees with the float64 oracle of the same operation (oracle/geo.py, oracle/decomp.py) at the tolerance the
      path's own parity test uses (cited per path) -- so a cell cannot pass with both sides stale or both sides wrong;
  (c) `out1` differs from `out0` by more than 10x that tolerance -- the weights really moved;
  (d) the path's cached kernel ran for `out1` -- a silent fall-back to torch ops cannot pass.

Writers: an in-place torch op; `p.data.copy_` (no `_version` bump) + `weights_changed()`; a raw-pointer device write
(`parallel.multi_copy`, vqn_multi_copy) + `weights_changed()`; a fused capturable `torch.optim.Adam` step; the package's `HipAdam`
(vqn_adam_step); `load_state_dict` from another model; replacing the parameter objects (vq_nfr: `set_codebook` twice with the old
objects dropped, so that the allocator and `id()` may hand the freed identity to the new one); and the two `weights_changed()` writers
again with every parameter frozen (`requires_grad_(False)` before the first run: the packs of frozen nets key on the rewrite epoch).
The trainer re-capture after a change of the per-call arguments is checked at the end."""
import gc

import numpy as np
import pytest
import torch

import vqnerf_release_amd
from tests.decomp_util import make_config, load_oracle_params, make_batch
from tests.gpu_util import launches

pytestmark = pytest.mark.gpu

WRITERS = ['inplace', 'data_copy', 'multi_copy', 'torch_adam', 'hip_adam', 'load_state_dict', 'replace',
           'data_copy_frozen', 'multi_copy_frozen']


def _np(t):
    return t.detach().cpu().numpy()


def _perturbed(t, rng, rel=0.05):
    """t + a perturbation of ~5 % of the tensor's spread (of its magnitude when constant)"""
    a = t.detach().double().cpu()
    s = float(a.std()) if a.numel() > 1 else 0.0
    s = s if s > 0 else float(a.abs().mean()) + 1e-2
    d = torch.tensor(rng.normal(0.0, rel * s, tuple(a.shape)))
    return (a + d).to(dtype=t.dtype, device=t.device).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# paths: build() -> holder with .nets_written (what the writers write) ; run(h) -> {name: tensor} ; oracle(h) -> {name: (want, tol, rows)}
# ---------------------------------------------------------------------------------------------------------------------------------
class _GeoPath:
    """NeuS on the full-size networks (oracle.geo.FULL_CFG, 24 rays as in smoke()).  Tolerances: sdf 2e-5 and gradients 2e-4 are the
    f32 kernels' bounds (tests/test_gpu_neus_x3.py docstring); the rendered colour 1e-3 is smoke()'s bound for all three modes."""
    B = 24

    def __init__(self, kind, mode='f32'):
        self.kind, self.mode = kind, mode
        self.kernel = {'sdf': 'vqn_neus_sdf_points', 'render': {'f32': 'vqn_neus_fine_points', 'x3': 'vqn_neus_fine_points_x3',
                                                                'f16s': 'vqn_neus_fine_points_f16s'}[mode],
                       'train': 'vqn_neus_train_fwd_x3'}[kind]

    def build(self):
        from oracle import geo as og
        from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork, SingleVarianceNetwork
        from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
        cfg = og.FULL_CFG
        c, cc = cfg['sdf'], cfg['color']
        sdf = SDFNetwork(d_in=3, d_out=c['d_out'], d_hidden=c['d_hidden'], n_layers=c['n_layers'], skip_in=tuple(c['skip_in']),
                         multires=c['multires'], bias=c['bias'], scale=c['scale'])
        sdf.load_state_dict({k: torch.tensor(v) for k, v in og.make_sdf_params(cfg, 0).items()})
        col = RenderingNetwork(d_feature=cc['d_feature'], mode=cc['mode'], d_in=cc['d_in'], d_out=cc['d_out'], d_hidden=cc['d_hidden'],
                               n_layers=cc['n_layers'], multires_view=cc['multires_view'], squeeze_out=cc['squeeze_out'])
        col.load_state_dict({k: torch.tensor(v) for k, v in og.make_color_params(cfg, 1).items()})
        var = SingleVarianceNetwork(0.3).cuda()
        ren = NeuSRenderer(None, sdf.cuda(), var, col.cuda(), **cfg['renderer'])
        ren.matrix_mode = self.mode
        h = type('Geo', (), {})()
        h.sdf, h.col, h.ren, h.cfg, h.nets_written = sdf, col, ren, cfg, [sdf, col]
        return h

    def load(self, h, src):
        h.sdf.load_state_dict(src.sdf.state_dict())
        h.col.load_state_dict(src.col.state_dict())

    def _rays(self):
        from oracle import geo as og
        return [torch.tensor(a, dtype=torch.float64) for a in og.make_rays(self.B, 2)]

    def _pts(self):
        return torch.tensor(np.random.default_rng(3).uniform(-1.2, 1.2, (300, 3)), dtype=torch.float64)

    def run(self, h):
        if self.kind == 'sdf':
            x = self._pts().float().cuda()
            with torch.no_grad():
                return {'sdf': h.sdf.sdf(x).reshape(-1), 'grad': h.sdf.gradient(x).reshape(-1, 3)}
        o, d, near, far = [t.float().cuda() for t in self._rays()]
        kw = dict(perturb_overwrite=0, background_rgb=torch.ones(1, 3, device='cuda'), cos_anneal_ratio=1.0)
        if self.kind == 'train':                                      # the forward of a training render (graph built, HIP backend)
            assert any(p.requires_grad for p in h.sdf.parameters())
            r = h.ren.render(o, d, near, far, 2.0, **kw)
            assert h.ren.last_train_backend == 'hip'
            return {'rgb': r['color_fine'].detach()}
        with torch.no_grad():
            return {'rgb': h.ren.render(o, d, near, far, 2.0, **kw)['color_fine']}

    def oracle(self, h):
        from oracle import geo as og
        p_sdf = {k: v.detach().double().cpu() for k, v in h.sdf.state_dict().items()}
        if self.kind == 'sdf':
            x = self._pts()
            with torch.no_grad():
                s = og.sdf_only(p_sdf, h.cfg, x)[:, 0]
            g = og.sdf_gradient(p_sdf, h.cfg, x).detach()
            return {'sdf': (s.numpy(), 2e-5, None), 'grad': (g.numpy(), 2e-4, None)}
        p_col = {k: v.detach().double().cpu() for k, v in h.col.state_dict().items()}
        o, d, near, far = self._rays()
        w = og.render(p_sdf, p_col, torch.tensor(0.3, dtype=torch.float64), h.cfg, o, d, near, far, 2.0,
                      background_rgb=torch.ones(1, 3, dtype=torch.float64), cos_anneal_ratio=1.0)
        return {'rgb': (w['color_fine'].detach().numpy(), 1e-3, None)}


def _p64(model):
    """the model's parameters in oracle.decomp's layout, float64"""
    c = lambda t: t.detach().double().cpu()
    p = {name: [(c(l.kernel), c(l.bias)) for l in net.layers] for name, net in model.net.items()}
    if model._light is not None:
        p['light'] = c(model._light)
    if getattr(model, '_codebook', None) is not None:
        p['codebook_raw'] = c(model._codebook)
    return p


def _decomp_scene(N=400, seed=9, ref=False, device='cuda'):
    """-> (batch on `device`, foreground mask on `device`, the oracle's float64 foreground rows, light positions, light areas)"""
    from oracle import decomp as od
    pts = od.make_points(N, seed=seed)
    if ref:
        pts['ref'] = np.random.default_rng(seed + 1).uniform(0, 1, (N, 3)).astype(np.float32)
    batch = make_batch({k: v for k, v in pts.items() if k != 'ref'}, device, bg_every=5)
    if ref:
        batch = batch[:9] + (torch.tensor(pts['ref'], device=device),) + batch[9:]
    keep = np.ones(N, bool)
    keep[::5] = False
    ob = {k: torch.tensor(v[keep], dtype=torch.float64) for k, v in pts.items()}
    lxyz, lareas = od.gen_light_xyz(16, 32)
    return (batch, torch.tensor(keep, device=device), ob, torch.tensor(lxyz, dtype=torch.float64),
            torch.tensor(lareas, dtype=torch.float64))


def _clear_rows(dist):
    d = np.sort(dist, 1)
    clear = (d[:, 1] - d[:, 0]) > 1e-5                                 # (tests/test_gpu_vq_entrypoints.py: near-ties go either way)
    assert clear.mean() > 0.9
    return clear


class _VqPath:
    """vq_nfr.Model.  Tolerances of tests/test_gpu_decomp.py::test_model_call_vs_oracle (materials 5e-6, linear colour 2e-5, indices
    exact on rows without an fp32 near-tie); 3x those in the x3 / f16s modes (test_ref_nfr_call_and_fast_render_vs_oracle's factor for
    its non-f32 mode)."""

    def __init__(self, kind, K=15, mode='f32'):
        self.kind, self.K, self.mode = kind, K, mode
        self.kernel = 'vqn_mlp_chain_vq_fwd' if (kind == 'call' and mode == 'f32') else \
            {'f32': 'vqn_mlp_chain_fwd', 'x3': 'vqn_refl_train_fwd_x3', 'f16s': 'vqn_mlp_chain_fwd_f16s'}[mode]

    def build(self):
        from oracle import decomp as od
        from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
        p, _ = od.make_model_params(seed=0, K=self.K)
        m = load_oracle_params(get_model_class('vq_nfr')(make_config(num_embed=self.K)), p, 'cuda')
        m.get_codebook()
        _ = m.light
        m.matrix_mode = self.mode
        m.nets_written = [m]
        return m

    def load(self, h, src):
        h.load_state_dict(src.state_dict())

    def run(self, m):
        batch, mk, _, _, _ = _decomp_scene()
        with torch.no_grad():
            if self.kind == 'call':
                pred, gt, lk, _ = m.call(batch, mode='vali')
                return {'rgb': lk['rgb'], 'albedo': pred['albedo'][mk], 'rough': pred['rough'][mk], 'vq_rgb': lk['vqrgb'],
                        'vq_albedo': pred['vq_albedo'][mk], 'embed': pred['embed'][mk][:, 0].float()}
            pred, _, _, _ = m.fast_render(batch, mode='test', gen_embed=True)
            return {k: pred[k][mk] for k in ('albedo', 'spec', 'rough', 'basecolor')} | {'embed': pred['embed'][mk][:, 0].float()}

    def oracle(self, m):
        from oracle import decomp as od
        _, specs = od.make_model_params(seed=0, K=self.K)
        _, _, ob, lxyz, lareas = _decomp_scene(device='cpu')
        p = _p64(m)
        t = 1 if self.mode == 'f32' else 3
        with torch.no_grad():
            vq = od._vq_step(p, specs, od.pred_enc(p, specs, ob['xyz']), 'vali', None, None)
            clear = _clear_rows(vq['distances'].numpy())
            embed = (vq['encoding_indices'] + 1).double().numpy()
            if self.kind == 'call':
                w = od.model_call(p, specs, ob, lxyz, lareas, None, None, mode='vali')
                return {'rgb': (w['rgb'].numpy(), t * 2e-5, None), 'albedo': (w['albedo'].numpy(), t * 5e-6, None),
                        'rough': (w['rough'].numpy(), t * 5e-6, None), 'vq_rgb': (w['vq_rgb'].numpy(), t * 2e-5, clear),
                        'vq_albedo': (w['vq_albedo'].numpy(), t * 5e-6, clear), 'embed': (embed, 0.0, clear)}
            w = od.fast_render(p, specs, ob, lxyz, lareas, gen_embed=True, mode='test')
            return {k: (w[k].numpy(), t * 5e-6, None) for k in ('albedo', 'spec', 'rough', 'basecolor')} | {'embed': (embed, 0.0, clear)}


class _NfrUnitPath:
    """nfr_unit.Model inference: encoder + the three `_out` heads in one launch (`enc_and_heads`).  Tolerances of
    tests/test_gpu_decomp.py::test_encoder_and_heads_vs_oracle (3e-6: z and the sigmoid heads)."""
    kernel = 'vqn_mlp_chain_fwd'
    HEADS = {'diff_out': 'diff_main', 'spec_out': 'spec_main', 'rough_out': 'rough_main'}

    def build(self):
        from oracle import decomp as od
        from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
        p, _ = od.make_model_params(seed=0, K=15)
        m = get_model_class('nfr_unit')(make_config(model='nfr_unit'))
        m.build_nets(device='cuda', seed=0)
        with torch.no_grad():
            for name in ('fine_enc', 'bottleneck') + tuple(self.HEADS):
                for layer, (W, b) in zip(m.net[name].layers, p[self.HEADS.get(name, name)]):
                    layer.kernel.copy_(torch.as_tensor(W))
                    layer.bias.copy_(torch.as_tensor(b))
        m.to('cuda')
        m.nets_written = [m]
        return m

    def load(self, h, src):
        h.load_state_dict(src.state_dict())

    def run(self, m):
        from oracle import decomp as od
        xyz = torch.tensor(od.make_points(333, seed=13)['xyz']).cuda()
        with torch.no_grad():
            z, a, s, r = m.enc_and_heads(xyz, 'out')
        return {'z': z, 'diff': a, 'spec': s, 'rough': r}

    def oracle(self, m):
        from oracle import decomp as od
        _, specs = od.make_model_params(seed=0, K=15)
        p = _p64(m)
        xyz = torch.tensor(od.make_points(333, seed=13)['xyz'], dtype=torch.float64)
        with torch.no_grad():
            z = od.pred_enc(p, specs, xyz)
            out = {'z': (z.numpy(), 3e-6, None)}
            for key, name in (('diff', 'diff_out'), ('spec', 'spec_out'), ('rough', 'rough_out')):
                out[key] = (od.mlp_forward(p[name], specs[self.HEADS[name]], z).numpy(), 3e-6, None)
        return out


class _RefPath:
    """ref_nfr.Model with the stage-2 parts frozen as `load_stage2` leaves them (fine_enc, bottleneck, spec_out: requires_grad False;
    as tests/test_gpu_decomp.py::test_ref_nfr_training_grads_vs_oracle sets them up).  Tolerances of
    test_ref_nfr_call_and_fast_render_vs_oracle (f32: linear colour 2e-5, displayed colour 1e-4, materials 5e-6)."""
    kernel = 'vqn_mlp_chain_fwd'

    def __init__(self, kind):
        self.kind = kind

    def build(self):
        from oracle import decomp as od
        from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
        p, _ = od.make_ref_params(seed=5)
        m = load_oracle_params(get_model_class('ref_nfr')(make_config(model='ref_nfr', data_type='nerf')), p, 'cuda')
        for name in ('fine_enc', 'bottleneck', 'spec_out'):
            for q in m.net[name].parameters():
                q.requires_grad_(False)
        m.nets_written = [m]
        return m

    def load(self, h, src):
        h.load_state_dict(src.state_dict())

    def run(self, m):
        batch, mk, _, _, _ = _decomp_scene(ref=True, seed=21)
        with torch.no_grad():
            if self.kind == 'call':
                pred, _, lk, _ = m.call(batch, mode='vali')
                return {'rgb': lk['rgb']} | {k: pred[k][mk] for k in ('albedo', 'spec', 'rough', 'basecolor')}
            pred, _, lk, _ = m.fast_render(batch, mode='test')
            return {'rgb': lk['rgb'], 'pred_rgb': pred['rgb'][mk]}

    def oracle(self, m):
        from oracle import decomp as od
        _, specs = od.make_ref_params(seed=5)
        _, _, ob, lxyz, lareas = _decomp_scene(ref=True, seed=21, device='cpu')
        p = _p64(m)
        with torch.no_grad():
            if self.kind == 'call':
                w = od.ref_nfr_call(p, specs, ob, lxyz, lareas, mode='vali')
                return {'rgb': (w['rgb'].numpy(), 2e-5, None)} | {k: (w[k].numpy(), 5e-6, None) for k in ('albedo', 'spec', 'rough', 'basecolor')}
            w = od.ref_nfr_fast_render(p, specs, ob, lxyz, lareas)
            return {'rgb': (w['rgb'].numpy(), 2e-5, None), 'pred_rgb': (w['pred_rgb'].numpy(), 1e-4, None)}


PATHS = {
    'geo-sdf-gradient': lambda: _GeoPath('sdf'),
    'geo-render-f32': lambda: _GeoPath('render', 'f32'),
    'geo-render-x3': lambda: _GeoPath('render', 'x3'),
    'geo-render-f16s': lambda: _GeoPath('render', 'f16s'),
    'geo-train-x3': lambda: _GeoPath('train'),
    'vq-call-K15': lambda: _VqPath('call', 15),
    'vq-call-K64': lambda: _VqPath('call', 64),
    'vq-call-x3': lambda: _VqPath('call', 15, 'x3'),
    'vq-call-f16s': lambda: _VqPath('call', 15, 'f16s'),
    'vq-fast_render-embed': lambda: _VqPath('fast_render', 15),
    'nfr_unit-infer': lambda: _NfrUnitPath(),
    'ref_nfr-call': lambda: _RefPath('call'),
    'ref_nfr-fast_render': lambda: _RefPath('fast_render'),
}

# cells that make no sense: a training render needs trainable parameters (frozen nets render on the inference kernels -- the
# geo-render-* rows); the geo f16s mode has no training path (nothing to parametrise).
SKIP = {('geo-train-x3', 'data_copy_frozen'): 'a frozen net has no training render (that is the inference path of the geo-render rows)',
        ('geo-train-x3', 'multi_copy_frozen'): 'a frozen net has no training render (that is the inference path of the geo-render rows)'}


# ---------------------------------------------------------------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------------------------------------------------------------
def _named(h):
    return [(mod, name, p) for mod in h.nets_written for name, p in mod.named_parameters()]


def _targets(h, seed):
    rng = np.random.default_rng(seed)
    return [_perturbed(p, rng) for _, _, p in _named(h)]


def _write(path, h, writer):
    named = _named(h)
    params = [p for _, _, p in named]
    if writer == 'inplace':
        with torch.no_grad():
            for p, t in zip(params, _targets(h, 1)):
                p.copy_(t)
    elif writer.startswith('data_copy'):
        for p, t in zip(params, _targets(h, 1)):
            p.data.copy_(t)                                           # (bumps no `_version`)
        vqnerf_release_amd.weights_changed()
    elif writer.startswith('multi_copy'):
        from vqnerf_release_amd import parallel
        with launches() as rec:
            parallel.multi_copy(params, _targets(h, 1))               # a raw-pointer device write: torch sees nothing
        assert rec.ran('vqn_multi_copy')
        vqnerf_release_amd.weights_changed()
    elif writer in ('torch_adam', 'hip_adam'):
        from vqnerf_release_amd import optim
        train = [p for p in params if p.requires_grad]
        rng = np.random.default_rng(2)
        for p in train:
            p.grad = torch.tensor(rng.normal(size=tuple(p.shape)), dtype=p.dtype, device=p.device)
        opt = (torch.optim.Adam(train, lr=1e-2, fused=True, capturable=True) if writer == 'torch_adam'
               else optim.HipAdam(train, lr=1e-2))
        with launches() as rec:
            opt.step()
        assert rec.ran('vqn_adam_step') == (writer == 'hip_adam')
        for p in train:
            p.grad = None
    elif writer == 'load_state_dict':
        other = path.build()
        for (_, _, p), t in zip(_named(other), _targets(h, 1)):
            with torch.no_grad():
                p.copy_(t)
        path.load(h, other)
        del other
    elif writer == 'replace':
        if isinstance(path, _VqPath):
            # B, then C, with the old objects dropped in between: C's storage (and id) may be A's
            cb = h._codebook.detach().t().cpu().numpy()
            rng = np.random.default_rng(4)
            h.set_codebook(cb + rng.normal(0, 0.05, cb.shape).astype(np.float32))
            gc.collect()
            torch.cuda.synchronize()
            h.set_codebook(np.clip(cb + rng.normal(0, 0.08, cb.shape), 0, 1).astype(np.float32))
        else:
            for (mod, name, p), t in zip(named, _targets(h, 1)):
                owner = mod.get_submodule(name.rsplit('.', 1)[0]) if '.' in name else mod
                setattr(owner, name.rsplit('.', 1)[-1], torch.nn.Parameter(t.clone(), requires_grad=p.requires_grad))
            del named, params, p
            gc.collect()
            torch.cuda.synchronize()
    else:
        raise AssertionError(writer)


@pytest.mark.parametrize('writer', WRITERS)
@pytest.mark.parametrize('path_name', list(PATHS))
def test_cached_path_after_a_weight_write(path_name, writer):
    if (path_name, writer) in SKIP:
        pytest.skip(SKIP[(path_name, writer)])
    path = PATHS[path_name]()
    h = path.build()
    if writer.endswith('_frozen'):
        for mod in h.nets_written:
            for p in mod.parameters():
                p.requires_grad_(False)
    out0 = {k: v.clone() for k, v in path.run(h).items()}           # builds the caches from W
    _write(path, h, writer)
    with launches() as rec:
        out1 = path.run(h)
    assert rec.ran(path.kernel), (path.kernel, sorted(rec.names))    # (d)
    fresh = path.build()
    path.load(fresh, h)
    out_fresh = path.run(fresh)
    want = path.oracle(fresh)
    moved = 0.0
    for k, (w, tol, rows) in want.items():
        a, f = out1[k], out_fresh[k]
        assert torch.equal(a, f), (k, float((a.double() - f.double()).abs().max()))                        # (a)
        got = _np(f).astype(np.float64)
        sel = slice(None) if rows is None else rows
        np.testing.assert_allclose(got[sel], w.reshape(got.shape)[sel], rtol=0, atol=tol, err_msg=k)      # (b)
        d = float((a.double() - out0[k].double()).abs().max())
        moved = max(moved, d / tol if tol > 0 else (np.inf if d > 0 else 0.0))
    assert moved > 10.0, moved                                                                             # (c)


def test_recapture_after_a_kwargs_change_runs_one_eager_step_first():
    """Trainer(graph=True) whose per-call arguments change after the capture (stage 1: `pretrain` True -> False, as fit_stage does when
    the pretraining epochs end): the first call under the new arguments runs EAGERLY (no replay, no capture) -- lazily built host-side
    state is then built outside stream capture -- and the step captured after it equals an eager trainer's step bit for bit (as
    test_gpu_train.py::test_captured_step_is_the_eager_step_for_every_stage_and_data_type)."""
    from oracle import decomp as od
    from vqnerf_release_amd.decomp.nerfactor import train_nfr
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    cfg = make_config(model='nfr_unit', n_rays_per_step=128, lr=2e-3)

    def build():
        m = get_model_class('nfr_unit')(cfg)
        m.build_nets(device='cuda', seed=4).to('cuda')
        return m

    batches = [make_batch(od.make_points(128, seed=70 + i), 'cuda') for i in range(7)]
    kw = [dict(pretrain=True)] * 4 + [dict(pretrain=False)] * 3
    params = {}
    for graph in (False, True):
        m = build()
        opt, _, clip = train_nfr.make_optimizer(cfg, m.trainable_variables, capturable=True)
        tr = train_nfr.Trainer(m, opt, clip=clip, graph=graph)
        for i, (b, k) in enumerate(zip(batches, kw)):
            captured_before = tr._captured
            tr.train_iter(b, global_bs=128, **k)
            if graph and i == 3:
                assert tr._captured is not None                       # steps 0, 1 eager, 2 captured, 3 replayed
            if graph and i == 4:                                      # the first step under the new arguments: eager
                assert captured_before is not None and tr._captured is None
            if graph and i == 5:
                assert tr._captured is not None                       # recorded under the new arguments
        params[graph] = [p.detach().clone() for p in m.trainable_variables]
    for a, b in zip(params[False], params[True]):
        assert torch.equal(a, b)
