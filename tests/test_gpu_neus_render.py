"""GPU parity: per-ray kernels and the NeuSRenderer boundary class against fixtures produced by the
REAL reference (tests/golden/geo_{full,small}.npz, see oracle/gen_golden_geo.py).

Tolerances (fp32, stated per quantity): z samples 2e-5 abs (inverse-CDF lerp of values ~[2,6]);
colour / weights / cdf 1e-3 abs end to end (the up-sampled z feed a steep sigmoid, inv_s up to 512);
stage-isolated checks (reference state fed in) are much tighter."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# relative bound of the gradient goldens (largest |difference| over the tensor's largest |entry|) = 2x the largest value observed over the
# three engines and both contractions (profiles/r05_observed_errors.json: full-size nets 1.80e-4 under x3, 8.9e-5 under the f32-input
# kernels; small nets 2.2e-6); rounds 1-4 asserted 5e-3
GRAD_BOUNDS = {'full': 3.6e-4, 'small': 5e-6}

CASES = [('full', 16), ('small', 64)]


def _cfg(name):
    from oracle import geo as og
    return og.FULL_CFG if name == 'full' else og.SMALL_CFG


def _build(name, dev='cuda'):
    from oracle import geo as og
    from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork, SingleVarianceNetwork
    from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
    cfg = _cfg(name)
    c, cc = cfg['sdf'], cfg['color']
    sdf = SDFNetwork(d_in=3, d_out=c['d_out'], d_hidden=c['d_hidden'], n_layers=c['n_layers'], skip_in=tuple(c['skip_in']),
                     multires=c['multires'], bias=c['bias'], scale=c['scale'], geometric_init=True, weight_norm=True)
    sdf.load_state_dict({k: torch.tensor(v) for k, v in og.make_sdf_params(cfg, 0).items()})
    col = RenderingNetwork(d_feature=cc['d_feature'], mode=cc['mode'], d_in=cc['d_in'], d_out=cc['d_out'],
                           d_hidden=cc['d_hidden'], n_layers=cc['n_layers'], weight_norm=True,
                           multires_view=cc['multires_view'], squeeze_out=cc['squeeze_out'])
    col.load_state_dict({k: torch.tensor(v) for k, v in og.make_color_params(cfg, 1).items()})
    var = SingleVarianceNetwork(0.3)
    sdf, col, var = sdf.to(dev), col.to(dev), var.to(dev)
    ren = NeuSRenderer(None, sdf, var, col, **cfg['renderer'])
    return cfg, sdf, col, var, ren


@pytest.fixture(scope='module', params=CASES, ids=[c[0] for c in CASES])
def case(request, golden_dir):
    from oracle import geo as og
    name, B = request.param
    g = dict(np.load(os.path.join(golden_dir, f'geo_{name}.npz')))
    cfg, sdf, col, var, ren = _build(name)
    o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(B, 2)]
    return dict(name=name, B=B, g=g, cfg=cfg, sdf=sdf, col=col, var=var, ren=ren, o=o, d=d, near=near, far=far)


def _np(t):
    return t.detach().cpu().numpy()


def test_upsample_and_merge_stagewise(case):
    g, ren, o, d = case['g'], case['ren'], case['o'], case['d']
    n0 = case['cfg']['renderer']['n_samples']
    z0 = (case['near'] + (case['far'] - case['near']) * torch.linspace(0, 1, n0, device='cuda')[None]).contiguous()
    with torch.no_grad():
        for i in range(4):
            zz = torch.tensor(g[f'up_z_{i - 1}']).cuda() if i else z0
            ss = torch.tensor(g[f'up_sdf_{i - 1}']).cuda() if i else torch.tensor(g['coarse_sdf']).cuda()
            new_z = ren.up_sample(o, d, zz, ss, 2.0, 16, 64 * 2 ** i)
            np.testing.assert_allclose(_np(new_z), g[f'up_new_z_{i}'], rtol=0, atol=2e-5)
            z2, s2 = ren.cat_z_vals(o, d, zz, torch.tensor(g[f'up_new_z_{i}']).cuda(), ss, last=(i == 3))
            np.testing.assert_array_equal(_np(z2), g[f'up_z_{i}'])          # merge is exact
            np.testing.assert_allclose(_np(s2), g[f'up_sdf_{i}'], rtol=0, atol=2e-5)


def test_merge_ties_are_stable():
    from vqnerf_release_amd import _C
    z = torch.tensor([[1.0, 2.0, 2.0, 3.0]]).cuda()
    s = torch.tensor([[10.0, 20.0, 21.0, 30.0]]).cuda()
    zn = torch.tensor([[2.0, 0.5, 3.0]]).cuda()        # unsorted new samples, with ties against old ones
    sn = torch.tensor([[99.0, 5.0, 98.0]]).cuda()
    zo, so = _C.neus_merge(z, s, zn, sn)
    assert zo.tolist() == [[0.5, 1.0, 2.0, 2.0, 2.0, 3.0, 3.0]]
    assert so.tolist() == [[5.0, 10.0, 20.0, 21.0, 99.0, 30.0, 98.0]]   # old before new on equal keys


@pytest.mark.parametrize('matrix_mode', ['f32', 'x3'])       # x3: the exact-split engine at the SAME bounds (VERDICT r02 #3 gate)
@pytest.mark.parametrize('car', [0.0, 0.5, 1.0])
def test_render_core_all_keys(case, car, matrix_mode):
    from tests.gpu_util import launches
    g, ren = case['g'], case['ren']
    n0 = case['cfg']['renderer']['n_samples']
    z_in = torch.tensor(g['core_z_in']).cuda()
    ren.matrix_mode = matrix_mode
    try:
        with torch.no_grad(), launches() as rec:
            rc = ren.render_core(case['o'], case['d'], z_in, 2 * 2.0 / n0, 2.0, case['sdf'], case['var'], case['col'],
                                 background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=car)
    finally:
        ren.matrix_mode = 'f32'
    assert rec.ran('vqn_neus_fine_points_x3') == (matrix_mode == 'x3')
    tol = dict(color=2e-4, sdf=2e-5, dists=0, gradients=3e-4, s_val=1e-7, mid_z_vals=0, weights=3e-4, cdf=3e-4,
               gradient_error=1e-5, inside_sphere=0, surf=5e-4, depth=5e-4)
    for k, t in tol.items():
        np.testing.assert_allclose(_np(rc[k]).reshape(g[f'core{car}_{k}'].shape), g[f'core{car}_{k}'], rtol=0, atol=t, err_msg=k)


@pytest.mark.parametrize('matrix_mode', ['f32', 'x3'])
@pytest.mark.parametrize('bg', ['white', 'none'])
@pytest.mark.parametrize('car', [0.0, 1.0])
def test_render_end_to_end_vs_reference(case, bg, car, matrix_mode):
    from tests.gpu_util import launches
    g, ren = case['g'], case['ren']
    ren.matrix_mode = matrix_mode
    try:
        with torch.no_grad(), launches() as rec:
            rr = ren.render(case['o'], case['d'], case['near'], case['far'], 2.0, perturb_overwrite=0,
                            background_rgb=torch.ones(1, 3).cuda() if bg == 'white' else None, cos_anneal_ratio=car)
    finally:
        ren.matrix_mode = 'f32'
    assert rec.ran('vqn_neus_fine_points_x3') == (matrix_mode == 'x3')
    assert not (matrix_mode == 'x3' and rec.ran('vqn_neus_sdf_points:'))      # (the small config has no up-sampling passes)
    assert set(rr.keys()) == {'color_fine', 's_val', 'cdf_fine', 'weight_sum', 'weight_max', 'gradients', 'weights',
                              'gradient_error', 'inside_sphere', 'surf', 'depth'}
    tol = dict(color_fine=1e-3, s_val=1e-7, cdf_fine=2e-3, weight_sum=1e-3, weight_max=1e-3, gradients=2e-3,
               weights=2e-3, gradient_error=1e-4, inside_sphere=0, surf=2e-3, depth=2e-3)
    for k, t in tol.items():
        ref = g[f'render_{bg}_{car}_{k}']
        np.testing.assert_allclose(_np(rr[k]).reshape(ref.shape), ref, rtol=0, atol=t, err_msg=k)
    psnr = -10 * np.log10(np.mean((_np(rr['color_fine']) - g[f'render_{bg}_{car}_color_fine']) ** 2) + 1e-20)
    print(f"{case['name']} {bg} car={car} {matrix_mode}: PSNR(hip, reference) = {psnr:.1f} dB")
    assert psnr > 70


def test_network_methods_hip_vs_autograd_path(case):
    """SDFNetwork.sdf / .gradient: HIP path (no graph) == torch path (graph) of the same module."""
    sdf = case['sdf']
    pts = torch.tensor(np.random.default_rng(5).uniform(-1, 1, (200, 3)).astype(np.float32)).cuda()
    with torch.no_grad():
        s_hip = sdf.sdf(pts)
        g_hip = sdf.gradient(pts)
    s_t = sdf.sdf(pts.clone().requires_grad_(True))
    g_t = sdf.gradient(pts.clone())
    assert s_hip.shape == s_t.shape == (200, 1) and g_hip.shape == g_t.shape == (200, 1, 3)
    np.testing.assert_allclose(_np(s_hip), _np(s_t), rtol=0, atol=2e-5)
    np.testing.assert_allclose(_np(g_hip), _np(g_t), rtol=0, atol=3e-4)


@pytest.fixture(params=['f32', 'bf16x3'])
def wgrad(request):
    """Both weight-gradient contractions against the reference's gradients: the f32 MFMA one (default) and the exact-split
    bf16x3 one (opt-in, `wgrad.wgrad_mode('bf16x3')`) -- same bound."""
    from vqnerf_release_amd import wgrad as tp
    old = tp.wgrad_mode()
    tp.wgrad_mode(request.param)
    yield request.param
    tp.wgrad_mode(old)


@pytest.fixture(params=['x3', 'fused', 'prog'])
def engine(request, monkeypatch):
    """The three forward / backward engines of the training step against the reference's gradients: the exact-split
    kernels (default), the f32-input MFMA two-image kernels, the interpreted tile programs -- same bound."""
    monkeypatch.setenv('VQN_TRAIN_FWD', request.param)
    monkeypatch.setenv('VQN_TRAIN_BWD', request.param)
    return request.param


def test_training_path_grads_vs_reference(case, wgrad, engine):
    """Training path of the boundary class (tile-program engine + compositing backward kernel): grads of L1(colour) +
    0.1 * eikonal wrt every parameter against the REAL reference's autograd, <= GRAD_BOUNDS of each tensor's largest entry (2x the observed error)."""
    from tests.gpu_util import launches
    g, ren, B = case['g'], case['ren'], case['B']
    for m in (case['sdf'], case['col'], case['var']):
        m.zero_grad()
    with launches() as rec:
        rr = ren.render(case['o'], case['d'], case['near'], case['far'], 2.0, perturb_overwrite=0,
                        background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=1.0)
        tgt = torch.tensor(np.random.default_rng(4).uniform(0, 1, (B, 3)).astype(np.float32)).cuda()
        loss = (rr['color_fine'] - tgt).abs().sum() / B + 0.1 * rr['gradient_error']
        loss.backward()
    assert ren.last_train_backend == 'hip' and (rec.ran('vqn_tile_program:prog_fwd') or rec.ran('vqn_neus_train_fwd')) and rec.ran('vqn_wgrad_partials')
    assert rec.ran('vqn_wgrad_partials_x3') == (wgrad == 'bf16x3')
    np.testing.assert_allclose(loss.item(), float(g['bwd_loss']), rtol=2e-4)
    worst, worst_at = 0.0, None
    for name, m in (('sdf', case['sdf']), ('col', case['col']), ('var', case['var'])):
        for k, p in m.named_parameters():
            ref = g[f'bwd_{name}.{k}']
            scale = max(np.abs(ref).max(), 1e-6)
            err = np.abs(_np(p.grad) - ref).max() / scale
            if err > worst:
                worst, worst_at = err, f'{name}.{k}'
            assert err <= GRAD_BOUNDS[case['name']], (name, k, err)
    from tests.gpu_util import record_observed
    record_observed('render_core_grads_vs_reference', f"{case['name']}/{engine}/{wgrad}/{worst_at}", worst, GRAD_BOUNDS[case['name']])
    for m in (case['sdf'], case['col'], case['var']):
        m.zero_grad()


def test_full_image_properties():
    """BASELINE-size batch (one 800x800 image row block): size-independent invariants."""
    from oracle import geo as og
    _, sdf, col, var, ren = _build('full')
    B = 8000
    o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(B, 11)]
    with torch.no_grad():
        rr = ren.render(o, d, near, far, 2.0, perturb_overwrite=0, background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=1.0)
        w = rr['weights']
        assert torch.isfinite(rr['color_fine']).all()
        assert (w >= 0).all() and (rr['weight_sum'] <= 1 + 1e-4).all()
        torch.testing.assert_close(w.sum(-1, keepdim=True), rr['weight_sum'], rtol=1e-5, atol=1e-5)
        assert torch.equal(w.max(-1, keepdim=True)[0], rr['weight_max'])
        assert (rr['color_fine'] >= 0).all() and (rr['color_fine'] <= 1 + 1e-4).all()
        # permutation equivariance over rays
        perm = torch.randperm(B, device='cuda')
        rp = ren.render(o[perm], d[perm], near[perm], far[perm], 2.0, perturb_overwrite=0,
                        background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=1.0)
        assert torch.equal(rp['color_fine'], rr['color_fine'][perm])
        # chunking independence (gen_geo.py:265-266 splits rays by batch_size)
        r1 = ren.render(o[:3001], d[:3001], near[:3001], far[:3001], 2.0, perturb_overwrite=0,
                        background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=1.0)
        assert torch.equal(r1['color_fine'], rr['color_fine'][:3001])


def test_full_view_640000_rays_properties():
    """The bench workload itself (BASELINE.json configs[1]: one 800 x 800 view = 640,000 rays x 128 samples in ONE render call): the
    size-independent invariants at the full size, and agreement of the one-call view with the same rays rendered in 80,000-ray chunks
    (gen_geo.py:265-266 splits a view by batch_size) and with a permuted ray order."""
    from oracle import geo as og
    _, sdf, col, var, ren = _build('full')
    B = 640000
    o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(B, 23)]
    bg = torch.ones(1, 3).cuda()
    kw = dict(perturb_overwrite=0, background_rgb=bg, cos_anneal_ratio=1.0)
    with torch.no_grad():
        rr = ren.render(o, d, near, far, 2.0, **kw)
        c, w, ws = rr['color_fine'], rr['weights'], rr['weight_sum']
        assert c.shape == (B, 3) and w.shape[0] == B
        assert torch.isfinite(c).all() and torch.isfinite(w).all()
        assert (w >= 0).all() and (ws <= 1 + 1e-4).all()
        assert (c >= 0).all() and (c <= 1 + 1e-4).all()
        torch.testing.assert_close(w.sum(-1, keepdim=True), ws, rtol=1e-5, atol=1e-5)
        assert torch.equal(w.max(-1, keepdim=True)[0], rr['weight_max'])
        assert float(ws.std()) > 0 and float(c.std()) > 0           # (not a constant image)
        # chunking independence at the reference's own chunk size, first / middle / ragged last chunk
        for a, b in ((0, 80000), (240000, 320000), (560000 + 37, 640000)):
            rc = ren.render(o[a:b], d[a:b], near[a:b], far[a:b], 2.0, **kw)
            assert torch.equal(rc['color_fine'], c[a:b])
            assert torch.equal(rc['weights'], w[a:b])
        del rc
        # a checksum of checksums: per-chunk sums in f64 add up to the view's
        tot = sum(float(c[i:i + 80000].double().sum()) for i in range(0, B, 80000))
        assert abs(tot - float(c.double().sum())) <= 1e-6 * abs(tot)
        # permutation equivariance over rays
        perm = torch.randperm(B, device='cuda')
        keep_c = c.clone()
        del rr, w, ws
        rp = ren.render(o[perm], d[perm], near[perm], far[perm], 2.0, **kw)
        assert torch.equal(rp['color_fine'], keep_c[perm])


def test_background_branch_runs_where_the_reference_raises():
    """n_outside > 0 (NeRF++ background, renderer.py:93-129, :309-331): dead in every shipped conf, and the reference's own
    render_core raises there (renderer.py:267 multiplies [B, n, 3] points by [B, n + n_outside] weights), so there are no
    values to match; the API is kept: this checks shapes, finiteness and that the inside / outside weights partition."""
    from oracle import geo as og
    from vqnerf_release_amd.geo.models.fields import NeRF
    cfg, sdf, col, var, ren = _build('small')
    ren.n_importance, ren.up_sample_steps, ren.n_outside = 16, 4, 8
    ren.nerf = NeRF(D=2, W=32, d_in=4, d_in_view=3, multires=4, multires_view=2, output_ch=4, skips=[], use_viewdirs=True).cuda()
    o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(24, 5)]
    n = ren.n_samples + ren.n_importance
    with torch.no_grad():
        r = ren.render(o, d, near, far, 2.0, perturb_overwrite=0, background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=0.6)
    assert r['weights'].shape == (24, n + 8) and r['gradients'].shape == (24, n, 3) and r['color_fine'].shape == (24, 3)
    assert all(torch.isfinite(v).all() for v in r.values() if torch.is_tensor(v))
    assert float(r['weights'].min()) >= 0 and float(r['weights'].sum(-1).max()) <= 1 + 1e-5


def test_render_after_a_fused_adam_step_uses_the_new_weights():
    """`torch._fused_adam_` moves the parameters without bumping their `_version` (measured): the weight packs of the render
    kernels key on the process-wide weights epoch as well (global optimiser post-step hook), so a render after such a step equals
    the render of a FRESH renderer loaded from the stepped parameters."""
    from oracle import geo as og
    _, sdf, col, var, ren = _build('small')
    o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(64, 5)]
    kw = dict(perturb_overwrite=0, background_rgb=torch.ones(1, 3).cuda(), cos_anneal_ratio=1.0)
    params = list(sdf.parameters()) + list(col.parameters()) + list(var.parameters())
    opt = torch.optim.Adam(params, lr=1e-2, fused=True)
    with torch.no_grad():
        before = ren.render(o, d, near, far, 2.0, **kw)['color_fine'].clone()          # fills the pack caches
    v0 = [p._version for p in params]
    rr = ren.render(o, d, near, far, 2.0, **kw)
    (rr['color_fine'].sum() + rr['gradient_error']).backward()
    opt.step()
    if [p._version for p in params] != v0:
        pytest.skip('this torch bumps _version in the fused Adam: nothing to guard')
    with torch.no_grad():
        after = ren.render(o, d, near, far, 2.0, **kw)['color_fine'].clone()
    _, sdf2, col2, var2, ren2 = _build('small')
    for dst, src in ((sdf2, sdf), (col2, col), (var2, var)):
        dst.load_state_dict(src.state_dict())
    with torch.no_grad():
        fresh = ren2.render(o, d, near, far, 2.0, **kw)['color_fine']
    assert not torch.equal(before, after)
    assert torch.equal(after, fresh)
