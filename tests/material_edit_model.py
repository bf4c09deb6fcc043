"""The numpy statement of the material selection and edit (csrc/material_edit.hip, decomp/nerfactor/util/material_edit.py): what the
kernel must give, bit for bit.  Comparisons and the scale quotient are float32, counts int64.

A selection is (codes, conds, ops):
  codes  a collection of code labels in [0, 64] (0 = background, 1..K = codes, as in the `embed` image), or None: no membership test;
  conds  a list of (prop, lo, hi); lo / hi hold one bound per channel of the property;
  ops    'and' | 'or', one fewer than conds.
Condition i holds on a pixel when EVERY channel c of its property has v_c > lo_c and v_c < hi_c (both strict; a NaN fails).
m = cond_0, then m = m | cond_i or m & cond_i for i = 1 .., strictly left to right, no precedence; the membership test is ANDed
last; `mask`, when given, after it.  With no conditions the mask is the membership test alone; with neither, `mask` alone.
Properties: rgb, xyz, diff, spec (3 channels), rough (1), mat = diff | spec | rough (7), and rgb_scale / diff_scale / spec_scale =
(p_0 / (p_2 + eps), p_1 / (p_2 + eps)) (2), eps = 5e-6, sum and quotient each rounded to float32.
A float `embed` is rounded to nearest-even (np.rint); a label outside [0, 64] (or NaN) is `invalid`: it fails the membership test,
is counted in `invalid` whenever embed is given, and enters no per-code count."""
import numpy as np

CHANNELS = {'rgb': 3, 'xyz': 3, 'diff': 3, 'spec': 3, 'rough': 1, 'mat': 7, 'rgb_scale': 2, 'diff_scale': 2, 'spec_scale': 2}
EPS = 5e-6
N_CODES = 65


def prop_values(props, name, eps=EPS):
    """the float32 [n, ch] values a condition on `name` tests"""
    f = lambda k: np.asarray(props[k], np.float32).reshape(len(props[k]), -1)
    if name == 'mat':
        return np.concatenate([f('diff'), f('spec'), f('rough')], axis=1)
    if name.endswith('_scale'):
        p = f(name[:-len('_scale')])
        with np.errstate(all='ignore'):
            return p[:, :2] / (p[:, 2:3] + np.float32(eps))             # float32 + float32, float32 / float32: each rounded once
    return f(name)


def labels(embed):
    """embed image (integers, or floats rounded to nearest-even) -> (int64 labels with -1 for an invalid one, bool invalid)"""
    e = np.asarray(embed).reshape(-1)
    if e.dtype.kind == 'f':
        r = np.rint(e.astype(np.float32))
        ok = (r >= 0) & (r <= N_CODES - 1)                           # (a NaN compares false)
        lab = np.where(ok, np.where(ok, r, 0), -1).astype(np.int64)
    else:
        e = e.astype(np.int64)
        ok = (e >= 0) & (e <= N_CODES - 1)
        lab = np.where(ok, e, -1)
    return lab, ~ok


def condition(props, cond, eps=EPS):
    name, lo, hi = cond
    v = prop_values(props, name, eps)
    lo = np.broadcast_to(np.asarray(lo, np.float32).reshape(-1), (v.shape[1],))
    hi = np.broadcast_to(np.asarray(hi, np.float32).reshape(-1), (v.shape[1],))
    with np.errstate(invalid='ignore'):
        return np.all((v > lo) & (v < hi), axis=-1)


def select(props, codes=None, conds=(), ops=(), embed=None, mask=None, eps=EPS, n=None):
    """-> {'mask' bool [n], 'selected', 'rows', 'invalid' ints, 'per_code' int64 [65]}"""
    conds, ops = list(conds), list(ops)
    assert len(ops) == max(len(conds) - 1, 0)
    if codes is None and not conds and mask is None:
        raise ValueError('a selection with neither codes nor conditions')
    if n is None:
        n = len(embed) if embed is not None else len(mask) if mask is not None else len(next(iter(props.values())))
    m = np.ones(n, bool)
    if conds:
        m = condition(props, conds[0], eps)
        for op, c in zip(ops, conds[1:]):
            m = (m | condition(props, c, eps)) if op == 'or' else (m & condition(props, c, eps))
    lab, bad = (None, np.zeros(n, bool)) if embed is None else labels(embed)
    if codes is not None:
        m = m & np.isin(lab, np.asarray(sorted(codes), np.int64)) & ~bad
    if mask is not None:
        m = m & (np.asarray(mask).reshape(-1) != 0)
    per_code = np.zeros(N_CODES, np.int64)
    if lab is not None:
        per_code += np.bincount(lab[m & ~bad], minlength=N_CODES).astype(np.int64)
    return {'mask': m, 'selected': int(m.sum()), 'rows': int(n), 'invalid': int(bad.sum()), 'per_code': per_code}


def apply(albedo, spec, rough, mask, dst, opt_scale=None):
    """dst = {'diff': [3], 'spec': [3], 'rough': [1]}: a material whose FIRST component is negative is left alone; otherwise a selected
    row takes the constant.  -> (albedo', spec', rough') and, with opt_scale [3], (albedo' * opt_scale, spec' * opt_scale) after them"""
    m = np.asarray(mask).reshape(-1, 1) != 0
    out = []
    for src, key in ((albedo, 'diff'), (spec, 'spec'), (rough, 'rough')):
        src = np.asarray(src, np.float32)
        v = np.asarray(dst[key], np.float32).reshape(1, -1)
        out.append(src.copy() if v[0, 0] < 0 else np.where(m, v, src).astype(np.float32))
    if opt_scale is not None:
        s = np.asarray(opt_scale, np.float32).reshape(1, 3)
        out += [out[0] * s, out[1] * s]
    return tuple(out)
