"""The inputs of the material edit tests, drawn once: tests/test_material_edit_model.py checks (on the CPU) that every case exercises
what it is meant to, tests/test_gpu_material_edit.py runs them on the kernel against tests/material_edit_model.py.

The first nine rows of every case are planted (the rest is random):
  0  selected;
  1  one tested value is bit-equal to a bound and nothing else keeps the row out: strictness alone excludes it;
  2  a NaN in a tested channel;
  3  a label above 64, 4 a negative one (both invalid);
  5  a float label at 2.5 (-> 2, nearest-even), 6 one at 3.5 (-> 4);
  7, 8  rows on which the standard program's 'and' / 'or' change the running mask.
A case with fewer rows has the first n of them."""
import functools

import numpy as np

from tests import material_edit_model as model
from vqnerf_release_amd import _C

P, G = _C.MATEDIT_ROWS_PER_PASS, _C.MATEDIT_GRID_CAP
MEMBERS = (1, 2, 3, 5, 64)
DST = {'diff': [0.1, 0.07, 0.02], 'spec': [0.85, 0.7, 0.35], 'rough': [0.35]}
OPT_SCALE = [1.25, 0.8, 1.1]
# the standard program: ((rough and diff_scale) or xyz), members only
STD_CONDS = [('rough', [0.25], [0.9]), ('diff_scale', [0.1, 0.1], [5.0, 5.0]), ('xyz', [-0.5] * 3, [0.5] * 3)]
STD_OPS = ['and', 'or']
# 8 conditions, 32 terms: 7 + 7 + 7 + 3 + 3 + 2 + 2 + 1 (the planted rows 1 and 2 hinge on the last condition, ANDed last)
MAX_CONDS = [('mat', [0.03] * 7, [0.97] * 7), ('mat', [0.5] * 3 + [0.0] * 4, [1.0] * 7), ('mat', [0.0] * 7, [0.6] * 3 + [1.0] * 4),
             ('rgb', [0.2] * 3, [1.0] * 3), ('xyz', [-0.9] * 3, [0.9] * 3), ('rgb_scale', [0.2, 0.2], [4.0, 4.0]),
             ('spec_scale', [0.0, 0.3], [2.0, 9.0]), ('rough', [0.3], [0.8])]
MAX_OPS = ['or', 'or', 'and', 'or', 'and', 'or', 'and']
KINDS = {'rgb': ([0.3] * 3, [0.95] * 3), 'xyz': ([-0.6] * 3, [0.7] * 3), 'diff': ([0.2] * 3, [0.9] * 3), 'spec': ([0.1] * 3, [0.8] * 3),
         'rough': ([0.3], [0.9]), 'mat': ([0.1] * 7, [0.97] * 7), 'rgb_scale': ([0.3, 0.2], [3.0, 4.0]),
         'diff_scale': ([0.3, 0.2], [3.0, 4.0]), 'spec_scale': ([0.3, 0.2], [3.0, 4.0])}


def _draw(n, seed, float_embed):
    rng = np.random.default_rng(seed)
    props = {'rgb': rng.uniform(0.02, 1, (n, 3)), 'xyz': rng.uniform(-1, 1, (n, 3)), 'diff': rng.uniform(0.02, 1, (n, 3)),
             'spec': rng.uniform(0.02, 1, (n, 3)), 'rough': rng.uniform(0, 1, (n, 1))}
    props = {k: v.astype(np.float32) for k, v in props.items()}
    runs = np.repeat(rng.integers(0, 9, n // 5 + 1), 5)[:n]                  # flat runs of 5 rows, as label images are
    embed = np.where(rng.random(n) < 0.5, runs, rng.integers(0, 9, n))
    embed[rng.random(n) < 0.02] = 64
    embed = embed.astype(np.float32 if float_embed else np.int32)
    if float_embed:
        embed += rng.uniform(-0.3, 0.3, n).astype(np.float32)
    return rng, props, embed


def _plant(props, embed, conds, n, strict=0):
    """the planted rows of the module docstring; condition `strict` is the one rows 1 and 2 hinge on"""
    def put(row, key, value):
        if row < n:
            props[key][row] = value
    inside = {'rgb': 0.5, 'xyz': 0.0, 'diff': 0.5, 'spec': 0.5, 'rough': 0.55}
    for row in (0, 1, 2):
        for k, v in inside.items():
            put(row, k, v)
    for row, lab in ((0, 1), (1, 1), (2, 1), (3, 77), (4, -3), (5, 2.5), (6, 3.5), (7, 1), (8, 1)):
        if embed is not None and row < n:
            embed[row] = lab if embed.dtype.kind == 'f' else int(np.floor(lab))   # (int: 2 and 3; 3 is a member too)
    if embed is not None and embed.dtype.kind != 'f' and n > 6:
        embed[6] = 4
    if not conds:
        return conds
    conds = [(p, list(lo), list(hi)) for p, lo, hi in conds]
    name = conds[strict][0]
    plane = 'diff' if name == 'mat' else name[:-6] if name.endswith('_scale') else name
    if n > 1:                                                    # row 1: the bound becomes the row's own value, bit for bit
        props[plane][1, 0] = inside[plane] - 0.2                 # (below the other planted rows' value: they stay inside)
        conds[strict][1][0] = float(model.prop_values({k: v[1:2] for k, v in props.items()}, name)[0, 0])
    put(2, plane, np.float32('nan') if props[plane].shape[1] == 1 else
        np.array([inside[plane]] * (props[plane].shape[1] - 1) + [np.nan], np.float32))
    if len(conds) == len(STD_CONDS) and [c[0] for c in conds] == [c[0] for c in STD_CONDS]:
        for row in (1, 2):
            put(row, 'xyz', 0.8)                                 # outside the xyz box: the 'or' does not rescue rows 1 and 2
        put(7, 'rough', 0.5), put(7, 'diff', [0.9, 0.9, 0.01]), put(7, 'xyz', 0.8)      # rough holds, diff_scale does not
        put(8, 'rough', 0.1), put(8, 'xyz', 0.0)                                          # the pair fails, xyz holds
    return conds


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(n, props, embed, mask_in, codes, conds, ops, dst, opt_scale, offset, mode): numpy inputs, never modified after"""
    kind, _, arg = name.partition(':')
    c = dict(name=name, codes=MEMBERS, conds=STD_CONDS, ops=STD_OPS, dst=DST, opt_scale=OPT_SCALE, offset=0, mode='both', mask_in=None)
    n, float_embed, seed = 2 * P + 5, False, sum(map(ord, name))
    if kind == 'rows':
        n = {'1': 1, '3': 3, '17': 17, 'P-1': P - 1, 'P': P, 'P+1': P + 1, '2P+5': 2 * P + 5, 'GP+P+7': G * P + P + 7}[arg]
    elif kind == 'offset':
        c['offset'] = 1
    elif kind == 'select':
        c.update(mode='select', dst=None, opt_scale=None)
    elif kind == 'mask_and_program':
        c['mask_in'] = True
    elif kind == 'edit_from_mask':
        c.update(mode='edit', codes=None, conds=[], ops=[], mask_in=True)
    elif kind == 'float_embed':
        float_embed = True
    elif kind == 'keep':
        c['dst'] = dict(DST, **{arg: [-1.0] * len(DST[arg])})
    elif kind == 'no_scale':
        c['opt_scale'] = None
    elif kind == 'kind':
        n = P + 1
        c.update(conds=[(arg,) + KINDS[arg]], ops=[])
    elif kind == 'codes_only':
        c.update(conds=[], ops=[])
    elif kind == 'conds_only':
        c.update(codes=None)
    elif kind == 'max':
        c.update(conds=MAX_CONDS, ops=MAX_OPS)
    else:
        raise KeyError(name)
    rng, props, embed = _draw(n + c['offset'], seed, float_embed)
    off = c['offset']
    props = {k: v[off:] for k, v in props.items()}                # (row views of the larger arrays: the planted rows are the views')
    embed = embed[off:]
    c['conds'] = _plant(props, embed, c['conds'], n, strict=len(c['conds']) - 1 if kind == 'max' else 0)
    c['strict'] = len(c['conds']) - 1 if kind == 'max' else 0
    if c['mask_in']:
        m = (rng.random(n + off) < 0.7).astype(np.uint8)[off:]
        m[:3] = 1
        c['mask_in'] = m
    c.update(n=n, props=props, embed=embed)
    for a in list(props.values()) + [embed] + ([c['mask_in']] if c['mask_in'] is not None else []):
        a.flags.writeable = False
    return c


ROW_CASES = ['rows:' + s for s in ('1', '3', '17', 'P-1', 'P', 'P+1', '2P+5', 'GP+P+7')]
MODE_CASES = ['offset', 'select', 'mask_and_program', 'edit_from_mask', 'float_embed', 'keep:diff', 'keep:spec', 'keep:rough', 'no_scale',
              'codes_only', 'conds_only', 'max'] + ['kind:' + k for k in KINDS]
ALL_CASES = ROW_CASES + MODE_CASES


@functools.lru_cache(maxsize=None)
def expected(name):
    """the statement's answer for a case, computed once: (select dict or None, edited tuple or None)"""
    c = case(name)
    sel = model.select(c['props'], c['codes'], c['conds'], c['ops'], embed=c['embed'] if c['mode'] != 'edit' else None, mask=c['mask_in'], n=c['n'])
    out = None
    if c['mode'] != 'select':
        p = c['props']
        out = model.apply(p['diff'], p['spec'], p['rough'], sel['mask'], c['dst'], c['opt_scale'])
    return sel, out
