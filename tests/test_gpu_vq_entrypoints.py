"""Model-level GPU parity of the REMAINING `vq_nfr.Model` entry points (VERDICT r02 missing #1): the ones the drop-ranking
validation (train_nfr.py:292-334), the k-means initialisation (train_nfr.py:206-228) and the segmentation / edit passes of
test.py (:270-330) run on --
    vq_test (vq_nfr.py:467-532, incl. `usage`), fast_embed (:209-256), init_z / init_mat (:183-207), vis_mat (:400-465),
    fast_render with edit_mask / edit_material / gen_embed / thres / relight_olat (:262-398),
    call(mode='vali', thres=..., roll=...) -- code dropout at MODEL level (:566-583).
HIP path vs oracle/decomp.py (from-source restatement, PARITY UNPINNED against the TF reference: see DESIGN.md) on 'nerf' and
'hw' data with the 8- and 64-entry codebooks.  The codebook here is cut from encoder outputs of other points (what the
k-means init produces) and the bottleneck's last layer is widened, so that rows really spread over the codes -- with the
bare glorot parameters every row lands on one code and `usage` / `embed` would test nothing.

Tolerances: materials 5e-6, rendered colours 2e-5 (linear) / 1e-4 (after the display transfer); VQ indices EXACT on every row
whose top-2 distance gap exceeds 1e-5 in the oracle (the others are genuine fp32 near-ties between two summation orders; they
must still be one of the two nearest codes)."""
import numpy as np
import pytest
import torch

from tests.decomp_util import make_config, load_oracle_params, make_batch
from tests.gpu_util import launches

pytestmark = pytest.mark.gpu

GAMMA = (1.3, 0.8)
CASES = [('nerf', 8), ('nerf', 64), ('hw', 8), ('hw', 64)]
BG = 6            # every 6th ray is background


def _np(t):
    return t.detach().cpu().numpy()


def _build(data_type, K, seed=0):
    from oracle import decomp as od
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    p, specs = od.make_model_params(seed=seed, K=K)
    W, b = p['bottleneck'][-1]
    p['bottleneck'][-1] = (W * 25.0, b)                                # spread z over (0, 1)
    pt = {k: ([(od.T(W), od.T(b)) for W, b in v] if isinstance(v, list) else od.T(v)) for k, v in p.items()}
    zc = od.pred_enc(pt, specs, od.T(od.make_points(K, seed=77)['xyz'])).numpy()
    cb = (zc + np.random.default_rng(5).normal(0, 0.02, zc.shape)).astype(np.float32).T      # [z_dim, K], a little outside [0, 1]
    p['codebook_raw'] = cb
    pt['codebook_raw'] = od.T(cb)
    model = load_oracle_params(get_model_class('vq_nfr')(make_config(data_type=data_type, num_embed=K)), p, 'cuda')
    gamma = None
    if data_type != 'nerf':
        model.gamma
        with torch.no_grad():
            model._gamma_bias.fill_(GAMMA[0])
            model._gamma_index.fill_(GAMMA[1])
        gamma = od.gamma_param(torch.tensor([GAMMA[0]]), torch.tensor([GAMMA[1]]))
    lxyz, lareas = od.gen_light_xyz(16, 32)
    return od, pt, specs, model, gamma, od.T(lxyz), od.T(lareas)


def _points(od, data_type, N, seed):
    pts = od.make_points(N, seed=seed, lvis=(data_type == 'nerf'))
    batch = make_batch(pts, 'cuda', bg_every=BG)
    keep = np.ones(N, bool)
    keep[::BG] = False
    ob = {k: od.T(v[keep]) for k, v in pts.items()}
    return pts, batch, keep, ob


def _check_indices(got, want_vq, K):
    """got: 1-based indices of the foreground rows.  Exact on clear rows; one of the two nearest codes elsewhere.  Returns the
    clear-row mask."""
    dist = want_vq['distances'].numpy()
    order = np.argsort(dist, 1)
    d = np.take_along_axis(dist, order, 1)
    clear = (d[:, 1] - d[:, 0]) > 1e-5
    assert clear.mean() > 0.97
    want = want_vq['encoding_indices'].numpy() + 1
    np.testing.assert_array_equal(got[clear], want[clear])
    amb = ~clear
    assert np.all((got[amb] == order[amb, 0] + 1) | (got[amb] == order[amb, 1] + 1))
    assert got.min() >= 1 and got.max() <= K
    return clear


def _drop_thres(K, keep):
    """The drop-ranking validation's threshold vectors (train_nfr.py:253-262, test.py:285): 0 keeps a code, 1 drops it."""
    return np.array([0.0] * keep + [1.0] * (K - keep), np.float32)


@pytest.mark.parametrize('data_type,K', CASES)
@pytest.mark.parametrize('dropped', [False, True])
def test_vq_test_vs_oracle(data_type, K, dropped):
    od, pt, specs, model, gamma, lxyz, lareas = _build(data_type, K)
    pts, batch, keep, ob = _points(od, data_type, 700, 3)
    thres = _drop_thres(K, K // 2) if dropped else None
    want = od.vq_test(pt, specs, ob, lxyz, lareas, thres=thres, data_type=data_type, gamma=gamma)
    with torch.no_grad(), launches() as rec:
        pred, gt, lk, to_vis = model.vq_test(batch, mode='vali', thres=thres)
    assert rec.ran('vqn_vq_quantize_rows') or rec.ran('vqn_vq_assign')
    assert rec.ran('vqn_brdf_shade_fwd') or rec.ran('vqn_brdf_shade_fwd_rows')
    assert set(lk) == {'vqloss', 'vqrgb', 'mode', 'gtc', 'rgb', 'usage'} and lk['mode'] == 'vali'
    assert set(pred) == {'alpha'} and set(gt) == {'alpha'} and set(to_vis) == {'id', 'hw'}
    # the model does not return the indices here: recover the clear-row mask from the oracle, compare the rendered rows on it
    dist = np.sort(want['vq']['distances'].numpy(), 1)
    clear = (dist[:, 1] - dist[:, 0]) > 1e-5
    assert clear.mean() > 0.97
    np.testing.assert_allclose(_np(lk['vqrgb'])[clear], want['vq_rgb'].numpy()[clear], rtol=0, atol=2e-5)
    assert lk['rgb'] is lk['vqrgb'] or torch.equal(lk['rgb'], lk['vqrgb'])                      # :525
    np.testing.assert_array_equal(_np(lk['gtc']), ob['rgb'].numpy())
    np.testing.assert_allclose(float(lk['vqloss']), float(want['vqloss']), rtol=1e-4)
    # usage [1, K]: 1 where a code won at least one row (:505).  Codes that win only ambiguous rows may go either way.
    usage = _np(lk['usage'])
    assert usage.shape == (1, K) and set(np.unique(usage)) <= {0.0, 1.0}
    widx = want['vq']['encoding_indices'].numpy()
    sure = np.zeros(K, bool)
    sure[np.unique(widx[clear])] = True
    maybe = sure.copy()
    order = np.argsort(want['vq']['distances'].numpy(), 1)
    maybe[np.unique(order[~clear, :2])] = True
    assert np.all(usage[0][sure] == 1.0) and np.all(usage[0][~maybe] == 0.0)
    assert sure.sum() >= min(K // 2, 6)                                                          # the codes really are in use
    if dropped:
        assert np.all(usage[0][K // 2:] == 0.0)                                                  # dropped codes never win
    # and the loss the drop ranking reads (train_nfr.py:586-594 -> compute_loss in vali mode)
    loss, ld = model.compute_loss(pred, gt, **dict(lk))
    wl, wd = od.compute_loss(dict(rgb=want['vq_rgb'], vq_rgb=want['vq_rgb']), ob['rgb'], pt['codebook_raw'], mode='vali',
                             data_type=data_type)
    for k in ('vqrgb', 'chromaticity'):
        np.testing.assert_allclose(_np(ld[k])[clear], wd[k].numpy()[clear], rtol=1e-4, atol=2e-6, err_msg=k)


@pytest.mark.parametrize('data_type,K', CASES)
def test_fast_embed_and_vis_mat_vs_oracle(data_type, K):
    od, pt, specs, model, gamma, lxyz, lareas = _build(data_type, K)
    pts, batch, keep, ob = _points(od, data_type, 700, 4)
    m = torch.tensor(keep).cuda()
    for thres in (None, _drop_thres(K, 3)):
        want = od.fast_embed(pt, specs, ob, thres=thres)
        want_vq = od._vq_step(pt, specs, od.pred_enc(pt, specs, ob['xyz']), 'vali', thres, None)
        with torch.no_grad():
            pred, gt, lk, to_vis = model.fast_embed(batch, mode='vali', thres=thres)
        assert lk == {'mode': 'vali'} and set(pred) == {'alpha'}
        assert set(to_vis) == {'id', 'hw', 'embed', 'xyz', 'pred_alpha', 'gt_alpha'}
        emb = _np(to_vis['embed'])
        assert emb.shape == (700, 1)
        np.testing.assert_array_equal(emb[~keep], 0)                                             # background rows: 0 (:247)
        _check_indices(emb[keep, 0], want_vq, K)
        if thres is not None:
            assert emb.max() <= 3
        np.testing.assert_array_equal(_np(to_vis['xyz'])[keep], ob['xyz'].numpy())
        np.testing.assert_array_equal(_np(to_vis['xyz'])[~keep], 0)
        # vis_mat: the same indices + the CONTINUOUS-branch materials
        wm = od.vis_mat(pt, specs, ob, thres=thres)
        with torch.no_grad():
            pred, gt, lk, to_vis = model.vis_mat(batch, mode='vali', thres=thres)
        assert set(pred) == {'alpha', 'albedo', 'spec', 'rough', 'embed'} and set(gt) == {'alpha'}
        _check_indices(_np(pred['embed'])[keep, 0], want_vq, K)
        for k in ('albedo', 'spec', 'rough'):
            np.testing.assert_allclose(_np(pred[k])[keep], wm[k].numpy(), rtol=0, atol=5e-6, err_msg=k)
            np.testing.assert_array_equal(_np(pred[k])[~keep], 0)
            assert to_vis['pred_' + k] is pred[k]


@pytest.mark.parametrize('data_type,K', [('nerf', 8), ('hw', 64)])
def test_init_z_and_init_mat_vs_oracle(data_type, K):
    od, pt, specs, model, gamma, lxyz, lareas = _build(data_type, K)
    pts, batch, keep, ob = _points(od, data_type, 500, 5)
    want_z = od.init_z(pt, specs, ob)
    with torch.no_grad(), launches() as rec:
        out = model.init_z(batch)
    assert rec.ran('vqn_mlp_chain_fwd')
    assert set(out) == {'id', 'hw', 'z_pred'} and out['z_pred'].shape == (int(keep.sum()), 256)
    np.testing.assert_allclose(_np(out['z_pred']), want_z.numpy(), rtol=0, atol=3e-6)
    want_m = od.init_mat(pt, specs, want_z)
    with torch.no_grad():
        mat = model.init_mat(out['z_pred'])
    assert mat.shape == (int(keep.sum()), 7)
    np.testing.assert_allclose(_np(mat), want_m.numpy(), rtol=0, atol=5e-6)


@pytest.mark.parametrize('data_type,K', CASES)
def test_fast_render_edit_embed_olat_vs_oracle(data_type, K):
    od, pt, specs, model, gamma, lxyz, lareas = _build(data_type, K)
    N = 600
    pts, batch, keep, ob = _points(od, data_type, N, 6)
    m = torch.tensor(keep).cuda()
    rng = np.random.default_rng(8)
    probes = [rng.uniform(0, 2, (16, 32, 3)).astype(np.float32) for _ in range(3)]
    model.novel_probes = {f'probe{i}': torch.tensor(a).cuda() for i, a in enumerate(probes)}
    # an edit mask over a third of the image (3 channels like the PNG the reference reads; only channel 0 counts, :290)
    em = np.zeros((N, 3), np.float32)
    em[rng.uniform(size=N) < 0.35, 0] = 1.0
    em[:, 1] = 1.0                                                     # must be ignored
    material = {'diff': [0.7, 0.2, 0.1], 'spec': [-1.0, 0.0, 0.0], 'rough': [0.35]}            # spec < 0: left alone (:323)
    thres = _drop_thres(K, 5)
    olat = od.novel_olat(white_bg=True, ambient_inten=0.0)
    assert list(olat) == list(model.novel_olat)
    for a, b_ in zip(olat.values(), model.novel_olat.values()):
        np.testing.assert_array_equal(a.numpy(), _np(b_))
    want = od.fast_render(pt, specs, ob, lxyz, lareas, data_type=data_type, gamma=gamma, probes=[od.T(a) for a in probes],
                          edit_mask=od.T(em[keep]), edit_material=material, gen_embed=True, thres=thres, relight_olat=True,
                          olat_maps=list(olat.values()))
    want_vq = od._vq_step(pt, specs, od.pred_enc(pt, specs, ob['xyz']), 'test', thres, None)
    kw = dict(mode='test', relight_olat=True, relight_probes=True, edit_mask=torch.tensor(em).cuda(), edit_material=material,
              gen_embed=True, thres=thres)
    with torch.no_grad():
        pred, gt, lk, to_vis = model.fast_render(batch, **kw)
    # reference behaviour: the flag is accepted, no OLAT render comes back (vq_nfr.py:733 returns None for it)
    assert 'rgb_olat' not in pred and 'pred_rgb_olat' not in to_vis
    assert set(pred) == {'alpha', 'basecolor', 'albedo', 'spec', 'rough', 'embed', 'rgb_probes'}
    assert set(lk) == {'mode', 'gtc'}
    edited = em[keep, 0] > 0
    got_alb = _np(pred['albedo'])[keep]
    np.testing.assert_array_equal(got_alb[edited], np.tile(np.float32(material['diff']), (edited.sum(), 1)))
    np.testing.assert_allclose(got_alb, want['albedo'].numpy(), rtol=0, atol=5e-6)
    np.testing.assert_allclose(_np(pred['spec'])[keep], want['spec'].numpy(), rtol=0, atol=5e-6)       # untouched by the edit
    np.testing.assert_allclose(_np(pred['rough'])[keep], want['rough'].numpy(), rtol=0, atol=5e-6)
    np.testing.assert_array_equal(_np(pred['rough'])[keep][edited], np.float32(0.35))
    np.testing.assert_allclose(_np(pred['basecolor'])[keep], want['basecolor'].numpy(), rtol=0, atol=5e-6)
    _check_indices(_np(pred['embed'])[keep, 0], want_vq, K)
    assert _np(pred['embed']).max() <= 5
    np.testing.assert_allclose(_np(pred['rgb_probes'])[keep], want['rgb_probes'].numpy(), rtol=0, atol=2e-4)
    np.testing.assert_array_equal(_np(pred['rgb_probes'])[~keep], 0)
    # the build's opt-in: OLAT maps rendered in the same pass, equal to the oracle's map-by-map integration
    model.render_olat = True
    with torch.no_grad():
        pred2, _, _, to_vis2 = model.fast_render(batch, **kw)
    assert pred2['rgb_olat'].shape == (N, 4, 3) and to_vis2['pred_rgb_olat'] is pred2['rgb_olat']
    np.testing.assert_allclose(_np(pred2['rgb_olat'])[keep], want['rgb_olat'].numpy(), rtol=0, atol=2e-4)
    np.testing.assert_array_equal(_np(pred2['rgb_probes']), _np(pred['rgb_probes']))
    # an all-negative edit is no edit at all (:321-326)
    with torch.no_grad():
        pred3, _, _, _ = model.fast_render(batch, mode='test', edit_mask=torch.tensor(em).cuda(),
                                           edit_material={'diff': [-1, 0, 0], 'spec': [-1, 0, 0], 'rough': [-1]})
        pred4, _, _, _ = model.fast_render(batch, mode='test')
    for k in ('albedo', 'spec', 'rough'):
        np.testing.assert_array_equal(_np(pred3[k]), _np(pred4[k]))


@pytest.mark.parametrize('data_type,K', CASES)
def test_call_with_code_dropout_vs_oracle(data_type, K):
    """`call(mode='vali', thres=..., roll=...)` at model level: thresholds strictly inside (0, 1) against an explicit draw, so
    that some codes are masked to the global maximum distance (vq_layers.py:284-290) and the rest compete."""
    od, pt, specs, model, gamma, lxyz, lareas = _build(data_type, K)
    pts, batch, keep, ob = _points(od, data_type, 700, 7)
    m = torch.tensor(keep).cuda()
    rng = np.random.default_rng(11)
    thres = rng.uniform(0.2, 0.8, (K,)).astype(np.float32)
    roll = rng.uniform(0.0, 1.0, (1, K)).astype(np.float32)
    n_kept = int((roll[0] >= thres).sum())
    assert 0 < n_kept < K
    want = od.model_call(pt, specs, ob, lxyz, lareas, od.EMA(0.999, (K,)), od.EMA(0.999, (256, K)), mode='vali',
                         thres=od.T(thres).reshape(1, K), roll=od.T(roll), data_type=data_type, gamma=gamma)
    with torch.no_grad(), launches() as rec:
        pred, gt, lk, to_vis = model.call(batch, mode='vali', thres=thres, roll=torch.tensor(roll).cuda())
    assert not rec.ran('vqn_mlp_chain_vq_fwd')                        # code dropout takes the quantiser launch, not the fused front
    assert rec.ran('vqn_vq_quantize_rows') or rec.ran('vqn_vq_assign')
    # the masked distances tie at the global maximum: only the kept codes can be the argmin (unless none is closer -- not here)
    got = _np(pred['embed'])[keep, 0]
    kept_codes = np.nonzero(roll[0] >= thres)[0] + 1
    assert set(np.unique(got)) <= set(kept_codes.tolist())
    dist = want['vq']['distances'].numpy()                            # (already masked)
    order = np.argsort(dist, 1, kind='stable')
    d = np.take_along_axis(dist, order, 1)
    clear = (d[:, 1] - d[:, 0]) > 1e-5
    assert clear.mean() > 0.97
    np.testing.assert_array_equal(got[clear], want['embed'].numpy()[clear])
    np.testing.assert_allclose(_np(lk['rgb']), want['rgb'].numpy(), rtol=0, atol=2e-5)            # continuous branch: no dropout
    np.testing.assert_allclose(_np(lk['vqrgb'])[clear], want['vq_rgb'].numpy()[clear], rtol=0, atol=2e-5)
    np.testing.assert_allclose(_np(lk['z'])[clear], want['z_vq'].numpy()[clear], rtol=0, atol=1e-6)
    np.testing.assert_allclose(float(lk['vqloss']), float(want['vq']['loss']), rtol=1e-4)
    np.testing.assert_allclose(_np(pred['vq_albedo'])[keep][clear], want['vq_albedo'].numpy()[clear], rtol=0, atol=5e-6)
    np.testing.assert_allclose(_np(pred['vq_rgb'])[keep][clear], od.displayed(want['vq_rgb'], data_type).numpy()[clear], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(_np(pred['embed'])[~keep], 0)
    # without dropout the same rows take more codes (the test really dropped something)
    with torch.no_grad():
        pred0, _, _, _ = model.call(batch, mode='vali')
    assert len(np.unique(_np(pred0['embed'])[keep])) > len(np.unique(got))


@pytest.mark.parametrize('data_type,K', [('nerf', 8), ('hw', 64)])
def test_entry_points_at_their_default_mode_vs_oracle(data_type, K):
    """`fast_embed(batch)`, `vis_mat(batch)` and `fast_render(batch, gen_embed=True)` without `mode`: the default is 'train', as in the
    reference (vq_nfr.py:209, :262, :400).  There the quantiser runs with `is_training=True` (vq_layers.py:314-320): the code map is the
    same nearest-code argmin as in 'vali', and every call ALSO advances the layer's two moving averages once (cluster sizes and dw, zero
    debiased) -- while the codebook itself stays where it is: only `call` copies `update` into it (vq_nfr.py:582-583).  Checked against
    oracle.decomp's `fast_embed` / `vis_mat` / `fast_render` in mode 'train', whose EMA objects advance in step with the model's."""
    od, pt, specs, model, gamma, lxyz, lareas = _build(data_type, K)
    pts, batch, keep, ob = _points(od, data_type, 700, 12)
    z_enc = od.pred_enc(pt, specs, ob['xyz'])
    want_vq = od._vq_step(pt, specs, z_enc, 'vali', None, None)
    ema = (od.EMA(0.999, (K,)), od.EMA(0.999, (256, K)))
    cb0 = model._codebook.detach().clone()
    vql = model.vq_layer

    def check_ema(calls, clear):
        want_cs, want_dw = ema[0].hidden.numpy(), ema[1].hidden.numpy()
        assert int(vql.ema_cluster_size.counter) == calls and int(vql.ema_dw.counter) == calls
        got_cs, got_dw = _np(vql.ema_cluster_size.hidden), _np(vql.ema_dw.hidden)
        # a near-tie row may sit in the other of its two nearest codes: each such row moves one count (times the decay weights)
        n_amb = int((~clear).sum())
        assert np.abs(got_cs - want_cs).sum() <= 2 * n_amb * (1 - 0.999) * calls + 1e-4, (got_cs, want_cs)
        if n_amb == 0:
            np.testing.assert_allclose(got_cs, want_cs, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(got_dw, want_dw, rtol=0, atol=2e-5 * max(1.0, float(np.abs(want_dw).max())))
        assert float(vql.ema_cluster_size.hidden.sum()) > 0                                       # the state really moved
        assert torch.equal(model._codebook.detach(), cb0)                                         # no codebook move outside `call`

    # fast_embed
    want = od.fast_embed(pt, specs, ob, mode='train', ema=ema)
    with torch.no_grad():
        pred, gt, lk, to_vis = model.fast_embed(batch)
    assert lk == {'mode': 'train'} and set(pred) == {'alpha'}
    emb = _np(to_vis['embed'])
    np.testing.assert_array_equal(emb[~keep], 0)
    clear = _check_indices(emb[keep, 0], want_vq, K)
    np.testing.assert_array_equal(want['embed'].numpy(), want_vq['encoding_indices'].numpy() + 1)  # same argmin as 'vali'
    check_ema(1, clear)
    # vis_mat
    wm = od.vis_mat(pt, specs, ob, mode='train', ema=ema)
    with torch.no_grad():
        pred, gt, lk, to_vis = model.vis_mat(batch)
    assert lk == {'mode': 'train'}
    _check_indices(_np(pred['embed'])[keep, 0], want_vq, K)
    for k in ('albedo', 'spec', 'rough'):
        np.testing.assert_allclose(_np(pred[k])[keep], wm[k].numpy(), rtol=0, atol=5e-6, err_msg=k)
    check_ema(2, clear)
    # fast_render(gen_embed=True)
    wf = od.fast_render(pt, specs, ob, lxyz, lareas, data_type=data_type, gamma=gamma, gen_embed=True, mode='train', ema=ema)
    with torch.no_grad():
        pred, gt, lk, to_vis = model.fast_render(batch, gen_embed=True)
    assert lk['mode'] == 'train' and set(pred) == {'alpha', 'basecolor', 'albedo', 'spec', 'rough', 'embed'}
    _check_indices(_np(pred['embed'])[keep, 0], want_vq, K)
    np.testing.assert_array_equal(_np(pred['embed'])[~keep], 0)
    for k in ('albedo', 'spec', 'rough', 'basecolor'):
        np.testing.assert_allclose(_np(pred[k])[keep], wf[k].numpy(), rtol=0, atol=5e-6, err_msg=k)
    check_ema(3, clear)
