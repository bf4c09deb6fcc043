"""GPU: the material selection and edit kernel (csrc/material_edit.hip) against its numpy statement (tests/material_edit_model.py) on the
cases of tests/material_edit_cases.py, EXACTLY: the mask, the counts and the bits of the edited and scaled tensors.  Exactness is derived,
not measured: comparisons are exact, and the only arithmetic is one correctly rounded add, one divide and one multiply, each stated the
same way in float32 numpy.  Then the refusals, the launch count (ONE: the counts row is zeroed on the stream by the entry, integer atomics,
no finalize launch), the two models' new keywords, and the scene driver."""
import json
import os

import numpy as np
import pytest
import torch

from tests import material_edit_cases as cases
from tests import material_edit_model as model
from tests.gpu_util import launches
from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.util import material_edit as me

pytestmark = pytest.mark.gpu
ENTRY = 'vqn_material_select_edit'


def _dev(a, offset=0):
    """numpy -> device tensor; offset: as a view starting `offset` rows into a larger tensor (a misaligned base)"""
    if a is None:
        return None
    t = torch.tensor(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    big = torch.empty((len(t) + offset,) + tuple(t.shape[1:]), dtype=t.dtype, device='cuda')
    big[offset:] = t.cuda()
    return big[offset:]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(name):
    c = cases.case(name)
    off = c['offset']
    props = {k: _dev(v, off) for k, v in c['props'].items()}
    embed, mask_in = _dev(c['embed'], off), _dev(c['mask_in'], off)
    sel = me.Selection(c['codes'], c['conds'], c['ops']) if c['mode'] != 'edit' else None
    scale = None if c['opt_scale'] is None else torch.tensor(c['opt_scale'], dtype=torch.float32, device='cuda')
    with launches() as rec:
        if c['mode'] == 'select':
            got, out = me.select(props, sel, embed=embed, mask=mask_in), None
        elif c['mode'] == 'edit':
            got, out = None, me.apply(props['diff'], props['spec'], props['rough'], mask_in, c['dst'], scale)
        else:
            got, out = me.select_apply(props, sel, props['diff'], props['spec'], props['rough'], c['dst'], embed=embed, mask=mask_in, opt_scale=scale)
    assert rec.counts == {ENTRY: 1}
    return c, props, got, out


@pytest.mark.parametrize('name', cases.ALL_CASES)
def test_kernel_equals_the_statement(name):
    c, props, got, out = _run(name)
    want_sel, want_out = cases.expected(name)
    if c['offset']:
        assert all(t.data_ptr() % 16 != 0 for k, t in props.items() if k != 'rough')       # the row-by-row path really ran
    if got is not None:
        assert got['mask'].dtype == torch.uint8 and got['mask'].is_cuda and got['per_code'].dtype == torch.int64
        assert np.array_equal(got['mask'].cpu().numpy(), want_sel['mask'].astype(np.uint8))
        assert int(got['selected']) == want_sel['selected'] and int(got['invalid']) == want_sel['invalid']
        assert np.array_equal(got['per_code'].cpu().numpy(), want_sel['per_code'])
    if want_out is not None:
        assert len(out) == len(want_out)
        for g, w in zip(out, want_out):
            assert g.shape == w.shape and torch.equal(_bits(g), _bits(torch.as_tensor(w).cuda()))
    else:
        assert out is None


def test_counts_row_and_embed_absent():
    """the raw row: selected, rows, invalid, 65 per-code counts; without embed the per-code counts are zero"""
    c = cases.case('conds_only')
    props = {k: _dev(v) for k, v in c['props'].items()}
    sel = me.Selection(None, c['conds'], c['ops'])
    mask, counts, out = _C.material_select_edit(c['n'], [props.get(p) if p in sel.needs() else None for p in me.PLANES], None, None, sel.terms(),
                                                [me._OPS[o] for o in sel.ops], len(sel.conds), None)
    want = model.select(c['props'], None, c['conds'], c['ops'])
    assert counts.shape == (_C.MATEDIT_HEAD_WORDS + _C.MATEDIT_CODES,) and out is None
    assert counts.tolist() == [want['selected'], c['n'], 0] + [0] * 65
    assert np.array_equal(mask.cpu().numpy(), want['mask'].astype(np.uint8))


def test_refusals():
    n = 64
    rough = torch.rand(n, 1, device='cuda')
    diff, spec = torch.rand(n, 3, device='cuda'), torch.rand(n, 3, device='cuda')
    embed = torch.randint(0, 5, (n,), device='cuda', dtype=torch.int32)
    term = lambda cond: (4, 0, -1, 0.2, 0.8, cond)
    planes = [None, None, None, None, rough]
    with pytest.raises(_C.VqnError, match='at most 8 conditions, got 9'):
        _C.material_select_edit(n, planes, terms=[term(i) for i in range(9)], ops=[0] * 8, n_conds=9)
    with pytest.raises(_C.VqnError, match='at most 32 terms, got 33'):
        _C.material_select_edit(n, planes, terms=[term(0)] * 33, n_conds=1)
    with pytest.raises(_C.VqnError, match='names plane 2, which is null'):
        _C.material_select_edit(n, planes, terms=[(2, 0, -1, 0.2, 0.8, 0)], n_conds=1)
    with pytest.raises(_C.VqnError, match='channel 1 / denominator -1 out of range for plane 4 of 1 channels'):
        _C.material_select_edit(n, planes, terms=[(4, 1, -1, 0.2, 0.8, 0)], n_conds=1)
    with pytest.raises(_C.VqnError, match='a condition without a term'):
        _C.material_select_edit(n, planes, terms=[term(1)], ops=[0], n_conds=2)
    with pytest.raises(_C.VqnError, match='nothing selects'):
        _C.material_select_edit(n, planes)
    with pytest.raises(_C.VqnError, match='a code set needs embed'):
        _C.material_select_edit(n, planes, codes=[1])
    # aliasing: an output that is an input, or overlaps one
    kw = dict(embed=embed, codes=[1, 2], edit=(diff, spec, rough), dst=[0.1] * 7)
    with pytest.raises(_C.VqnError, match='aliases an input'):
        _C.material_select_edit(n, planes, out=[diff, torch.empty_like(spec), torch.empty_like(rough)], **kw)
    big = torch.empty(2 * n, 3, device='cuda')
    big[:n] = spec
    with pytest.raises(_C.VqnError, match='aliases an input'):
        _C.material_select_edit(n, planes, embed=embed, codes=[1], edit=(diff, big[:n], rough), dst=[0.1] * 7,
                                out=[torch.empty_like(diff), big[n // 2:n // 2 + n], torch.empty_like(rough)])
    with pytest.raises(_C.VqnError, match='contiguous'):
        _C.material_select_edit(n, [None, None, None, None, torch.rand(n, 2, device='cuda')[:, :1]], terms=[term(0)], n_conds=1)
    with pytest.raises(ValueError, match='does not hold'):
        me.select({'rough': rough}, me.Selection(None, [('rgb', 0.1, 0.9)]))
    with pytest.raises(ValueError, match='needs `embed`'):
        me.select({'rough': rough}, me.Selection([1]))
    # after the refusals the entry still works
    got = me.select({'rough': rough}, me.Selection([1, 2], [('rough', 0.2, 0.8)]), embed=embed)
    want = model.select({'rough': rough.cpu().numpy()}, (1, 2), [('rough', 0.2, 0.8)], [], embed=embed.cpu().numpy())
    assert int(got['selected']) == want['selected']


def test_no_rows_no_launch():
    z = lambda ch: torch.empty(0, ch, device='cuda')
    with launches() as rec:
        got, out = me.select_apply({'rough': z(1)}, me.Selection([1], [('rough', 0.2, 0.8)]), z(3), z(3), z(1), cases.DST,
                                   embed=torch.empty(0, dtype=torch.int32, device='cuda'), opt_scale=cases.OPT_SCALE)
    assert rec.counts == {} and not rec.ran('vqn_')
    assert got['mask'].shape == (0,) and int(got['selected']) == 0 and int(got['invalid']) == 0 and got['per_code'].tolist() == [0] * 65
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3), (0, 1), (0, 3), (0, 3)]


# ---- the models ------------------------------------------------------------------------------------------------------------------
H, W, BG = 6, 5, 6                                               # a 6 x 5 view; every 6th row is background
MATERIAL = {'diff': [0.7, 0.2, 0.1], 'spec': [-1.0, 0.0, 0.0], 'rough': [0.35]}          # spec: first component negative, left alone
SCALE = [1.2, 0.9, 0.8]


def _probes(model, n=2):
    rng = np.random.default_rng(8)
    model.novel_probes = {f'probe{i}': torch.tensor(rng.uniform(0, 2, (16, 32, 3)).astype(np.float32)).cuda() for i in range(n)}


def _with_hw(batch):
    batch = list(batch)
    batch[1] = torch.tensor([[H, W]] * (H * W)).cuda()
    return tuple(batch)


@pytest.fixture(scope='module')
def vq():
    from tests.test_gpu_vq_entrypoints import _build, _points
    od, pt, specs, model, gamma, lxyz, lareas = _build('nerf', 8)
    _probes(model)
    views = [_with_hw(_points(od, 'nerf', H * W, seed)[1]) for seed in (6, 7)]
    return model, views


@pytest.fixture(scope='module')
def ref():
    from tests.test_gpu_decomp import _ref_setup, _ref_batch
    od, p, pt, specs, model, gamma = _ref_setup('nerf')
    _probes(model)
    views = [_with_hw(_ref_batch(od, H * W, 'nerf', seed, BG)[1]) for seed in (6, 7)]
    return model, views


def _rows_mask(seed=3):
    m = (np.random.default_rng(seed).uniform(size=H * W) < 0.4)
    m[1] = True
    return m


def _same(a, b, skip=()):
    assert set(a) - set(skip) == set(b) - set(skip)
    for k in set(a) - set(skip):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('which', ['vq', 'ref'])
@pytest.mark.parametrize('scale', [None, 'host', 'device'])
def test_edit_rows_equals_edit_mask(which, scale, request):
    model, views = request.getfixturevalue(which)
    m = _rows_mask()
    em = torch.tensor(np.repeat(m[:, None], 3, 1).astype(np.float32)).cuda()
    rows = torch.tensor(m.astype(np.uint8)).cuda()
    opt = None if scale is None else SCALE if scale == 'host' else torch.tensor([SCALE], device='cuda')
    opt_t = None if scale is None else torch.tensor([SCALE], device='cuda')
    kw = dict(mode='test', relight_probes=True, edit_material=MATERIAL)
    if which == 'vq':
        kw['gen_embed'] = True
    with torch.no_grad():
        want, _, _, _ = model.fast_render(views[0], edit_mask=em, opt_scale=opt_t, **kw)
        with launches() as rec:
            got, _, _, vis_d = model.fast_render(views[0], edit_rows=rows, opt_scale=opt, **kw)
    assert rec.counts[ENTRY] == 1
    assert 'rgb_probes' in got and 'edit_mask' not in got
    _same(got, want)
    if which == 'vq':                                            # the edit really took place
        sel = torch.tensor(m).cuda() & (views[0][5][:, 0] > 0)
        assert torch.equal(got['albedo'][sel], torch.tensor(MATERIAL['diff']).cuda().expand(int(sel.sum()), 3))
        assert not torch.equal(got['albedo'], model.fast_render(views[0], mode='test')[0]['albedo'])


def _statement_on(base, batch, sel, rgb=None):
    props = {'diff': base['albedo'].cpu().numpy(), 'spec': base['spec'].cpu().numpy(), 'rough': base['rough'].cpu().numpy(),
             'xyz': batch[7].cpu().numpy() * (batch[5].cpu().numpy() > 0)}
    if rgb is not None:
        props['rgb'] = rgb.cpu().numpy()
    return model.select(props, sel.codes, sel.conds, sel.ops, embed=base['embed'][:, 0].cpu().numpy())


def _selection_for(base, extra=()):
    """the two most frequent codes of the view and a bound at the median roughness of their rows: part of them is selected"""
    emb = base['embed'][:, 0].cpu().numpy().astype(np.int64)
    codes = [int(c) for c in np.argsort(-np.bincount(emb[emb > 0], minlength=9))[:2]]
    med = float(np.median(base['rough'].cpu().numpy()[np.isin(emb, codes), 0]))
    return me.Selection(codes, [('rough', med, 2.0), ('xyz', -10.0, 10.0)] + list(extra), ['and'] + ['and'] * len(extra))


def test_edit_select_in_the_model(vq):
    vq_model, views = vq
    batch = views[0]
    with torch.no_grad():
        base, _, _, _ = vq_model.fast_render(batch, mode='test', gen_embed=True)
        sel = _selection_for(base)
        want = _statement_on(base, batch, sel)
        fg = int((batch[5][:, 0] > 0).sum())
        assert 0 < want['selected'] < fg and not want['mask'][::BG].any()
        kw = dict(mode='test', relight_probes=True, edit_material=MATERIAL, gen_embed=True, opt_scale=SCALE)
        with launches() as rec:
            got, _, _, to_vis = vq_model.fast_render(batch, edit_select=sel, **kw)
        assert rec.counts[ENTRY] == 1
        assert got['edit_mask'].shape == (H * W, 1) and got['edit_mask'].dtype == torch.float32 and to_vis['pred_edit_mask'] is got['edit_mask']
        assert np.array_equal(got['edit_mask'][:, 0].cpu().numpy(), want['mask'].astype(np.float32))
        rows, _, _, _ = vq_model.fast_render(batch, edit_rows=torch.tensor(want['mask'].astype(np.uint8)).cuda(), **kw)
        _same(got, rows, skip=('edit_mask',))
        # a condition on the rendered colour: the caller supplies it
        rgb = torch.rand(H * W, 3, device='cuda')
        sel2 = _selection_for(base, extra=[('rgb_scale', [0.2, 0.2], [3.0, 3.0])])
        want2 = _statement_on(base, batch, sel2, rgb)
        got2, _, _, _ = vq_model.fast_render(batch, edit_select=sel2, edit_props={'rgb': rgb}, **kw)
        assert np.array_equal(got2['edit_mask'][:, 0].cpu().numpy(), want2['mask'].astype(np.float32)) and 0 < want2['selected'] < want['selected']


@pytest.mark.parametrize('which', ['vq', 'ref'])
def test_new_keywords_left_at_none_change_nothing(which, request):
    model, views = request.getfixturevalue(which)
    em = torch.tensor(np.repeat(_rows_mask()[:, None], 3, 1).astype(np.float32)).cuda()
    none = dict(edit_rows=None) if which == 'ref' else dict(edit_select=None, edit_rows=None, edit_props=None)
    with torch.no_grad():
        for kw in (dict(mode='test'), dict(mode='test', relight_probes=True, opt_scale=torch.tensor([SCALE], device='cuda'), edit_mask=em,
                                           edit_material=MATERIAL)):
            with launches() as rec:
                a = model.fast_render(views[1], **kw, **none)[0]
            assert ENTRY not in rec.counts
            _same(a, model.fast_render(views[1], **kw)[0])


def test_the_three_value_errors(vq, ref):
    sel = me.Selection([1])
    rows = torch.ones(H * W, dtype=torch.uint8, device='cuda')
    em = torch.ones(H * W, 3, device='cuda')
    for model, views in (vq, ref):
        with launches() as rec:
            with pytest.raises(ValueError, match='edit_mask together with'):
                model.fast_render(views[0], mode='test', edit_mask=em, edit_material=MATERIAL, edit_rows=rows)
            with pytest.raises(ValueError, match='without edit_material'):
                model.fast_render(views[0], mode='test', edit_rows=rows)
        assert rec.counts == {}                                  # refused before any launch
    model, views = vq
    with launches() as rec:
        with pytest.raises(ValueError, match='edit_mask together with'):
            model.fast_render(views[0], mode='test', edit_mask=em, edit_material=MATERIAL, edit_select=sel)
        with pytest.raises(ValueError, match='without edit_material'):
            model.fast_render(views[0], mode='test', edit_select=sel)
        with pytest.raises(ValueError, match="needs edit_props"):
            model.fast_render(views[0], mode='test', edit_material=MATERIAL, edit_select=me.Selection([1], [('rgb_scale', 0.1, 2.0)]))
    assert rec.counts == {}


# ---- the driver ------------------------------------------------------------------------------------------------------------------
class _Views:
    """what decomp/edit.py reads of a dataset: `files` and `view(f)`"""

    def __init__(self, views):
        self.views = {f'view{i}': v for i, v in enumerate(views)}
        self.files = list(self.views)

    def view(self, f):
        return self.views[f]


def _png(path, mode='RGB'):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert(mode))


def test_run_and_select_views(vq, ref, tmp_path):
    from vqnerf_release_amd.decomp import edit
    from vqnerf_release_amd.decomp.nerfactor.util.vis import _EMBED_COLOURS, to_uint8
    (vq_model, vq_views), (ref_model, ref_views) = vq, ref
    with torch.no_grad():
        bases = [vq_model.fast_render(b, mode='test', gen_embed=True)[0] for b in vq_views]
    sel = _selection_for(bases[0])
    dst = {'diff': [0.7, 0.2, 0.1], 'spec': [-1, -1, -1], 'rough': [0.35]}
    root = str(tmp_path / 'pd_edit')
    writer, counts = edit.run(vq_model, _Views(vq_views), root, sel, dst, ref_model=ref_model, ref_dataset=_Views(ref_views))
    writer.flush()
    assert json.load(open(os.path.join(root, 'auto_sel', 'dst.json'))) == {k: [float(x) for x in v] for k, v in dst.items()}
    assert list(counts) == ['batch000000000', 'batch000000001']
    for i, name in enumerate(counts):
        want = _statement_on(bases[i], vq_views[i], sel)
        m = np.load(os.path.join(root, 'auto_sel', name + '.npy'))
        assert m.dtype == bool and m.shape == (H, W, 3) and (m[..., 0] == m[..., 1]).all() and (m[..., 0] == m[..., 2]).all()
        assert np.array_equal(m[..., 0].reshape(-1), want['mask']) and counts[name] == want['selected']
        files = set(os.listdir(os.path.join(root, name)))
        assert {'pred_edit_mask.png', 'pred_albedo.png', 'pred_rough.png', 'embed_map.png', 'pred_rgb.png', 'pred_rgb_probes_probe0.png'} <= files
        assert np.array_equal(_png(os.path.join(root, name, 'pred_edit_mask.png'), 'L') > 0, m[..., 0])
        alb = _png(os.path.join(root, name, 'pred_albedo.png'))
        assert m[..., 0].any() and (alb[m[..., 0]] == to_uint8(np.float32(dst['diff']))).all()
    assert sum(counts.values()) > 0
    # the file form, on the files `run` wrote: codes and a roughness bound, against the statement on the quantised (byte / 255) values
    sel_f = me.Selection(sel.codes, [('rough', 0.3, 0.9)])
    got = edit.select_views(root, sel_f, dst=dst, src_view='batch000000001')
    out = os.path.join(str(tmp_path), 'auto_sel', 'pd_edit')
    assert sorted(got) == ['batch000000000', 'batch000000001'] and json.load(open(os.path.join(out, 'dst.json')))['rough'] == [0.35]
    for name in got:
        rough = (np.arange(256, dtype=np.float32) / np.float32(255))[_png(os.path.join(root, name, 'pred_rough.png'), 'L')].reshape(-1, 1)
        emb_rgb = _png(os.path.join(root, name, 'embed_map.png')).reshape(-1, 3)
        labels = np.zeros(len(emb_rgb), np.int32)
        for j, px in enumerate(emb_rgb):
            for c in range(len(_EMBED_COLOURS)):
                if tuple(px) == tuple(_EMBED_COLOURS[c][::-1]):
                    labels[j] = c + 1
                    break
        want = model.select({'rough': rough}, sel_f.codes, sel_f.conds, [], embed=labels)
        m = np.load(os.path.join(out, name + '.npy'))
        assert m.dtype == bool and m.shape == (H, W, 3) and np.array_equal(m[..., 0].reshape(-1), want['mask']) and got[name] == want['selected']
        if name == 'batch000000001':
            assert np.array_equal(_png(os.path.join(out, 'edit_mask.png')), m.astype(np.uint8) * 255)
    assert 0 < sum(got.values()) < 2 * H * W
    # a size mismatch between a view's files raises
    from PIL import Image
    Image.fromarray(np.zeros((H + 1, W), np.uint8)).save(os.path.join(root, 'batch000000000', 'pred_rough.png'))
    with pytest.raises(ValueError, match='sizes differ'):
        edit.select_views(root, sel_f)


def test_compute_rgb_scales(tmp_path):
    """float64 sums on the device, as metric_eval.albedo_scale: 1e-12 relative against the float64 numpy restatement"""
    from PIL import Image
    from vqnerf_release_amd.decomp import edit
    rng = np.random.default_rng(11)
    srgb = lambda t: np.where(np.clip(t, 0, 1) <= 0.0031308, np.clip(t, 0, 1) * 12.92, 1.055 * np.clip(t, 0, 1) ** (1.0 / 2.4) - 0.055)
    for with_spec in (False, True):
        roots = [str(tmp_path / f'{k}{int(with_spec)}') for k in ('pred', 'gt', 'vis')]
        want = []
        for i in (0, 3):
            img = {k: rng.integers(0, 256, (H, W, 4 if k == 'rgba' else 3)).astype(np.uint8) for k in ('pred_albedo', 'pred_spec', 'albedo', 'metal', 'rgba')}
            for k, a in img.items():
                d = os.path.join(roots[0], f'batch{i:09d}') if k.startswith('pred') else os.path.join(roots[1 if k == 'rgba' else 2], f'val_{i:03d}')
                os.makedirs(d, exist_ok=True)
                Image.fromarray(a).save(os.path.join(d, k + '.png'))
            f = {k: a.astype(np.float64) / 255.0 for k, a in img.items()}
            pred, gt = srgb(f['pred_albedo'] + f['pred_spec']), srgb(f['albedo'] + (f['metal'] if with_spec else 0.0))
            alpha = f['rgba'][..., 3]
            want.append([(np.sum(gt[..., c] * alpha) / np.sum(alpha)) / (np.sum(pred[..., c] * alpha) / np.sum(alpha)) for c in range(3)])
        got = edit.compute_rgb_scales(*roots, with_spec=with_spec)
        assert got.dtype == torch.float64 and got.is_cuda and got.shape == (3,)
        np.testing.assert_allclose(got.cpu().numpy(), np.mean(want, axis=0), rtol=1e-12, atol=0)
    Image.fromarray(np.zeros((H + 2, W, 3), np.uint8)).save(os.path.join(roots[2], 'val_000', 'albedo.png'))
    with pytest.raises(ValueError, match='sizes differ'):
        edit.compute_rgb_scales(*roots)
