"""CPU: the numpy statement of the material selection (tests/material_edit_model.py) against a per-pixel restatement in plain loops; that
every input the GPU tests draw (tests/material_edit_cases.py) exercises what it is meant to, so that the GPU run cannot pass
vacuously; `Selection` validation and `from_ui`; and the blend identity the model equality tests rest on."""
import math

import numpy as np
import pytest

from tests import material_edit_cases as cases
from tests import material_edit_model as model
from vqnerf_release_amd.decomp.nerfactor.util.material_edit import Selection
from vqnerf_release_amd.decomp.nerfactor.util.vis import _EMBED_COLOURS

f32 = np.float32


def pixel(props, i, codes, conds, ops, embed, mask, eps=model.EPS):
    """the rule for ONE pixel, in plain loops -> (selected, invalid, label or None)"""
    def values(name):
        if name == 'mat':
            return [f32(x) for k in ('diff', 'spec', 'rough') for x in np.reshape(props[k][i], -1)]
        if name.endswith('_scale'):
            p = [f32(x) for x in props[name[:-6]][i]]
            with np.errstate(all='ignore'):
                den = f32(p[2] + f32(eps))
                return [f32(p[0] / den), f32(p[1] / den)]
        return [f32(x) for x in np.reshape(props[name][i], -1)]

    def holds(cond):
        name, lo, hi = cond
        vs = values(name)
        lo = [lo] * len(vs) if np.ndim(lo) == 0 else list(lo) * (len(vs) if len(lo) == 1 else 1)
        hi = [hi] * len(vs) if np.ndim(hi) == 0 else list(hi) * (len(vs) if len(hi) == 1 else 1)
        for v, a, b in zip(vs, lo, hi):
            if math.isnan(v) or not (v > f32(a) and v < f32(b)):
                return False
        return True

    m = True
    if conds:
        m = holds(conds[0])
        for k in range(1, len(conds)):
            m = (m or holds(conds[k])) if ops[k - 1] == 'or' else (m and holds(conds[k]))
    label, invalid = None, False
    if embed is not None:
        e = embed[i]
        if isinstance(e, (np.floating, float)):
            if math.isnan(e):
                invalid = True
            else:
                fl = math.floor(e)                               # nearest, ties to even, spelled out
                d = float(e) - fl
                r = fl + (1 if d > 0.5 or (d == 0.5 and fl % 2 == 1) else 0)
                invalid, label = not 0 <= r <= 64, int(r)
        else:
            invalid, label = not 0 <= int(e) <= 64, int(e)
    if codes is not None:
        m = m and not invalid and label in codes
    if mask is not None:
        m = m and mask[i] != 0
    return m, invalid, None if invalid else label


def test_the_statement_equals_the_per_pixel_loops():
    """200 random rows, every property kind, both ops, int and float labels, with and without a mask"""
    rng, props, embed = cases._draw(200, 7, True)
    props['rough'][5] = np.nan
    props['spec'][9, 2] = np.nan
    embed[:6] = [2.5, 3.5, 70.2, -0.7, np.nan, 64.4]
    ints = np.where(np.isnan(embed), 99, np.floor(embed)).astype(np.int32)
    mask = (rng.random(200) < 0.8).astype(np.uint8)
    conds = [('mat', [0.02] * 7, [0.9] * 7), ('rgb', 0.1, 0.95), ('xyz', [-0.8] * 3, [0.6] * 3), ('diff', [0.1] * 3, [0.99] * 3),
             ('spec', [0.05] * 3, [0.9] * 3), ('rough', [0.2], [0.85]), ('rgb_scale', [0.2, 0.3], [3.0, 2.0]), ('diff_scale', 0.25, 3.5),
             ('spec_scale', [0.1, 0.1], [4.0, 4.0])]
    seen_ops = set()
    for trial in range(12):
        pick = rng.permutation(len(conds))[:rng.integers(1, 6)]
        cs = [conds[j] for j in pick]
        ops = [('and', 'or')[int(rng.integers(0, 2))] for _ in cs[1:]]
        seen_ops.update(ops)
        for codes, emb, msk in ((cases.MEMBERS, embed, None), (None, ints, mask), ((1, 4), ints, mask), (None, None, None)):
            want = [pixel(props, i, codes, cs, ops, emb, msk) for i in range(200)]
            got = model.select(props, codes, cs, ops, embed=emb, mask=msk)
            assert [bool(x) for x in got['mask']] == [w[0] for w in want]
            assert got['selected'] == sum(w[0] for w in want) and got['invalid'] == sum(w[1] for w in want) and got['rows'] == 200
            per = np.zeros(65, np.int64)
            for w in want:
                if w[0] and w[2] is not None:
                    per[w[2]] += 1
            assert np.array_equal(got['per_code'], per)
    assert seen_ops == {'and', 'or'}
    assert {c[0] for c in conds} == set(model.CHANNELS)
    # membership alone, and the keep rule of the edit
    got = model.select(props, (1, 2), embed=embed)
    assert [bool(x) for x in got['mask']] == [pixel(props, i, (1, 2), [], [], embed, None)[0] for i in range(200)]
    with pytest.raises(ValueError):
        model.select(props, None, [], [])
    m = got['mask']
    a, s, r = model.apply(props['diff'], props['spec'], props['rough'], m, {'diff': [0.3, 0.2, 0.1], 'spec': [-1, 0.5, 0.5], 'rough': [0.7]})
    for i in range(200):
        assert np.array_equal(a[i], f32([0.3, 0.2, 0.1]) if m[i] else props['diff'][i])
        assert np.array_equal(s[i], props['spec'][i], equal_nan=True)                      # first component negative: kept
        assert np.array_equal(r[i], f32([0.7]) if m[i] else props['rough'][i], equal_nan=True)


@pytest.mark.parametrize('name', cases.ALL_CASES)
def test_a_gpu_case_exercises_what_it_is_meant_to(name):
    c = cases.case(name)
    sel, out = cases.expected(name)
    n, conds, ops, props = c['n'], c['conds'], c['ops'], c['props']
    assert sel['rows'] == n and len(sel['mask']) == n
    if n == 1:
        assert sel['selected'] == 1
    elif n == 3:
        assert 0 < sel['selected'] < 3
    else:
        assert 0.05 <= sel['selected'] / n <= 0.95
    if c['mode'] == 'edit':                                      # no program: the mask is mask_in
        assert np.array_equal(sel['mask'], c['mask_in'] != 0)
        return
    each = [model.condition(props, cond) for cond in conds]
    if n >= 17:
        for e in each:
            assert e.any() and not e.all()
        m = each[0] if each else None
        for op, e in zip(ops, each[1:]):
            nxt = (m | e) if op == 'or' else (m & e)
            assert (nxt != m).any(), op
            m = nxt
    if conds and n >= 3:
        k = c['strict']
        v = model.prop_values(props, conds[k][0])
        lo = f32(conds[k][1][0])
        # row 1: bit-equal to the bound, excluded; with the bound one float lower it is selected: strictness alone excludes it
        assert v[1, 0].view(np.int32) == lo.view(np.int32) and not sel['mask'][1]
        relaxed = [list(x) for x in conds]
        relaxed[k][1] = [float(np.nextafter(lo, f32(-np.inf)))] + list(conds[k][1][1:])
        assert model.select(props, c['codes'], [tuple(x) for x in relaxed], ops, embed=c['embed'], mask=c['mask_in'])['mask'][1]
        # row 2: a NaN in a tested channel
        assert np.isnan(v[2]).any() and not each[k][2] and not sel['mask'][2]
    if n >= 17:
        lab, bad = model.labels(c['embed'])
        assert bad[3] and bad[4] and sel['invalid'] >= 2
        if c['codes'] is not None:
            assert not sel['mask'][3] and not sel['mask'][4]
        if c['embed'].dtype.kind == 'f':
            assert c['embed'][5] == 2.5 and lab[5] == 2 and c['embed'][6] == 3.5 and lab[6] == 4
        assert sel['per_code'].sum() == (sel['mask'] & ~bad).sum()
    if out is not None:
        assert len(out) == (5 if c['opt_scale'] is not None else 3)
        assert not np.array_equal(out[0], props['diff']) or c['dst']['diff'][0] < 0


def test_the_special_cases_are_among_the_cases():
    assert cases.case('float_embed')['embed'].dtype == np.float32 and cases.case('rows:17')['embed'].dtype == np.int32
    assert cases.case('offset')['offset'] == 1
    assert len(cases.case('max')['conds']) == 8 and len(Selection(None, cases.case('max')['conds'], cases.MAX_OPS).terms()) == 32


def test_selection_validation():
    s = Selection(codes=[3, 1, 3], conds=[('rough', 0.2, 0.8), ('mat', 0.0, [1.0] * 7)], ops=['or'])
    assert s.codes == (1, 3) and s.conds[0] == ('rough', (float(f32(0.2)),), (float(f32(0.8)),))
    assert len(s.conds[1][1]) == 7 and len(s.terms()) == 8 and s.needs() == ['rough', 'diff', 'spec']
    assert [t[:3] for t in Selection(None, [('rgb_scale', 0.1, 2.0)]).terms()] == [(0, 0, 2), (0, 1, 2)]
    with pytest.raises(ValueError, match='neither codes nor conditions'):
        Selection()
    with pytest.raises(ValueError, match='take 1 ops'):
        Selection(None, [('rough', 0, 1), ('rgb', 0, 1)], [])
    with pytest.raises(ValueError, match='take 0 ops'):
        Selection(None, [('rough', 0, 1)], ['and'])
    with pytest.raises(ValueError, match='3 channels'):
        Selection(None, [('rgb', [0, 0], [1, 1])])
    with pytest.raises(ValueError, match="'and' | 'or'"):
        Selection(None, [('rough', 0, 1), ('rgb', 0, 1)], ['xor'])
    with pytest.raises(ValueError, match='prop one of'):
        Selection(None, [('embed', 0, 1)])
    with pytest.raises(ValueError, match='code labels'):
        Selection([65])
    with pytest.raises(ValueError, match='code labels'):
        Selection([1.5])
    with pytest.raises(ValueError, match='at most 8 conditions'):
        Selection(None, [('rough', 0, 1)] * 9, ['and'] * 8)
    with pytest.raises(ValueError, match='32 channel tests'):
        Selection(None, [('mat', 0, 1)] * 5, ['and'] * 4)
    assert Selection([], []).codes == ()                         # an empty set is a selection: it selects nothing


def test_selection_from_ui():
    # the UI's empty text field: cond_flags == [''], conds_op == ['']
    col = _EMBED_COLOURS[4][::-1]                                # code 5 as embed_map.png holds it (R, G, B)
    s = Selection.from_ui([''], [], [''], embed_colours=[col / 255.0])
    assert s.codes == (5,) and s.conds == [] and s.ops == ()
    s = Selection.from_ui(['rough', 'diff_scale'], [[[0.2], [0.8]], [[0.1, 0.1], [5.0, 5.0]]], ['or'], embed_colours=np.stack([col, _EMBED_COLOURS[0][::-1]]))
    assert s.codes == (1, 5) and [c[0] for c in s.conds] == ['rough', 'diff_scale'] and s.ops == ('or',)
    s = Selection.from_ui([''], [], [''], embed_colours=[[1, 2, 3]])         # an unknown colour selects nothing
    assert s.codes == ()
    props = {'rough': np.zeros((4, 1), f32)}
    assert model.select(props, s.codes, embed=np.arange(4))['selected'] == 0
    with pytest.raises(ValueError):
        Selection.from_ui([''], [], [''])                        # neither colours nor conditions
    with pytest.raises(ValueError, match='bounds'):
        Selection.from_ui(['rough', 'rgb'], [[[0.2], [0.8]]], ['or'])


def test_the_blend_identity_of_the_torch_statements():
    """src * (1 - m) + m * v == where(m, v, src) under ==, for finite src, v and m in {0, 1}: with m = 1 the sum is src * 0 + v =
    (+-0) + v = v for v != 0 and a zero for v = 0; with m = 0 it is src + 0 * v = src + (+-0) = src, a zero staying a zero.  The signs
    of zeros can differ, the values cannot: the model tests compare with torch.equal, which is ==."""
    import torch
    vals = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.35, 1e-38, -1e-38, 1e-45, 3.4e38, -3.4e38, 0.1, 7.25], dtype=torch.float32)
    src = vals.reshape(-1, 1, 1).expand(-1, len(vals), 2)
    v = vals.reshape(1, -1, 1).expand(len(vals), -1, 2)
    m = torch.tensor([0.0, 1.0]).reshape(1, 1, 2).expand(len(vals), len(vals), -1)
    blend = src * (1 - m) + m * v
    where = torch.where(m > 0, v, src)
    assert torch.equal(blend, where)
    g = torch.Generator().manual_seed(0)
    src, v = torch.randn(4096, generator=g) * 3, torch.randn(4096, generator=g)
    m = (torch.rand(4096, generator=g) < 0.5).float()
    assert torch.equal(src * (1 - m) + m * v, torch.where(m > 0, v, src))
