"""Material selection and editing on the device: pick the pixels of a material by their VQ code, optionally narrowed by bounds on other
per-pixel properties, and replace their material -- the selection rule of the reference's decomp/nerfvq_nfr3/ui4_offline.py (`map_f`
:263-345, numpy inside a PyQt window) and the six blend statements of its vq_nfr.py:325-330, in one launch of csrc/material_edit.hip
(tests/material_edit_model.py is the numpy statement).

A `Selection` is a set of code labels (0 = background, 1..K = codes, as in the `embed` image; None: no membership test), a list of box
conditions (prop, lo[], hi[]) and one 'and' | 'or' fewer than conditions:
  * a condition holds where EVERY channel of its property has lo < v < hi, both strict; a NaN fails;
  * m = cond_0, then m = m | cond_i or m & cond_i, strictly left to right, no precedence (ui4_offline.py:325-330);
  * the membership test is ANDed last (:331-332); with no conditions the mask is the membership test alone.
Properties: rgb, xyz, diff (albedo), spec: 3 channels; rough: 1; mat = diff | spec | rough: 7; rgb_scale, diff_scale, spec_scale:
(p_0 / (p_2 + eps), p_1 / (p_2 + eps)), eps = 5e-6 (:300-302); `mat` and the `*_scale` forms are terms of the kernel's program on the
tensors as the models hold them, never materialised.

One deviation from the reference: its `mat` property reads the SOURCE view's files for every view (:295-297), a slip; here every
view tests its own values.

There is no CPU path: numpy inputs are uploaded."""
import numpy as np
import torch

from vqnerf_release_amd import _C

CHANNELS = {'rgb': 3, 'xyz': 3, 'diff': 3, 'spec': 3, 'rough': 1, 'mat': 7, 'rgb_scale': 2, 'diff_scale': 2, 'spec_scale': 2}
PLANES = ('rgb', 'xyz', 'diff', 'spec', 'rough')       # the kernel's plane slots
EPS = 5e-6                                             # ui4_offline.py:263
_OPS = {'and': 0, 'or': 1}


class Selection:
    """codes: labels in [0, 64] or None; conds: (prop, lo, hi) with one bound per channel of the property (a single float is
    broadcast, as the UI's text fields allow); ops: 'and' | 'or', one fewer than conds."""

    def __init__(self, codes=None, conds=(), ops=()):
        self.codes = None
        if codes is not None:
            codes = list(codes)
            if any(int(c) != c or not 0 <= int(c) < _C.MATEDIT_CODES for c in codes):
                raise ValueError(f'code labels are integers in [0, {_C.MATEDIT_CODES - 1}], got {codes}')
            self.codes = tuple(sorted({int(c) for c in codes}))
        self.conds = []
        for cond in conds:
            if len(cond) != 3 or cond[0] not in CHANNELS:
                raise ValueError(f'a condition is (prop, lo, hi) with prop one of {sorted(CHANNELS)}, got {cond!r}')
            prop, ch = cond[0], CHANNELS[cond[0]]
            bounds = []
            for b in cond[1:]:
                b = np.asarray(b, np.float32).reshape(-1)
                if b.size not in (1, ch):
                    raise ValueError(f'{prop} has {ch} channels, got a bound of {b.size} values')
                bounds.append(tuple(float(x) for x in np.broadcast_to(b, (ch,))))
            self.conds.append((prop, bounds[0], bounds[1]))
        self.ops = tuple(ops)
        if any(o not in _OPS for o in self.ops):
            raise ValueError(f"ops are 'and' | 'or', got {list(ops)}")
        if len(self.ops) != max(len(self.conds) - 1, 0):
            raise ValueError(f'{len(self.conds)} conditions take {max(len(self.conds) - 1, 0)} ops, got {len(self.ops)}')
        if self.codes is None and not self.conds:
            raise ValueError('a selection with neither codes nor conditions selects nothing in particular: refused')
        if len(self.conds) > _C.MATEDIT_MAX_CONDS or len(self.terms()) > _C.MATEDIT_MAX_TERMS:
            raise ValueError(f'a selection has at most {_C.MATEDIT_MAX_CONDS} conditions and {_C.MATEDIT_MAX_TERMS} channel tests, got '
                             f'{len(self.conds)} and {len(self.terms())}')

    @classmethod
    def from_ui(cls, cond_flags, cond_bounds, conds_op, embed_colours=None):
        """The UI's own argument shapes (ui4_offline.py:358-372, :392): cond_flags a list of property names ([''] or []: none),
        cond_bounds [[lo[], hi[]], ...], conds_op a list of 'and' | 'or' (entries past the needed ones are ignored, as the UI's loop
        does), embed_colours the picked `embed_map.png` colours, RGB as the file holds them, bytes or floats in [0, 1].  A colour
        becomes its code through vis._EMBED_COLOURS; an unknown colour selects nothing."""
        from vqnerf_release_amd.decomp.nerfactor.util.vis import _EMBED_COLOURS
        flags = [] if cond_flags is None or (len(cond_flags) > 0 and cond_flags[0] == '') else list(cond_flags)
        bounds = list(cond_bounds or [])[:len(flags)]
        if len(bounds) != len(flags):
            raise ValueError(f'{len(flags)} conditions with {len(bounds)} bounds')
        codes = None
        if embed_colours is not None:
            codes = set()
            for col in np.asarray(embed_colours).reshape(-1, 3):
                byte = np.rint(col * 255.0) if np.asarray(col).dtype.kind == 'f' else col
                hit = np.nonzero((_EMBED_COLOURS[:, ::-1].astype(np.int64) == np.asarray(byte, np.int64)).all(-1))[0]
                codes.update(int(i) + 1 for i in hit)          # (the file is RGB, the table B, G, R; code i has row i - 1)
        return cls(codes, [(f, b[0], b[1]) for f, b in zip(flags, bounds)], list(conds_op or [])[:max(len(flags) - 1, 0)])

    def needs(self):
        """the planes (of PLANES) the conditions read"""
        out = []
        for prop, _, _ in self.conds:
            for p in (('diff', 'spec', 'rough') if prop == 'mat' else (prop[:-len('_scale')] if prop.endswith('_scale') else prop,)):
                if p not in out:
                    out.append(p)
        return out

    def terms(self):
        """the kernel's program: rows (plane, channel, denominator channel or -1, lo, hi, condition id)"""
        rows = []
        for i, (prop, lo, hi) in enumerate(self.conds):
            if prop == 'mat':
                where = [('diff', 0), ('diff', 1), ('diff', 2), ('spec', 0), ('spec', 1), ('spec', 2), ('rough', 0)]
                rows += [(PLANES.index(p), c, -1, lo[j], hi[j], i) for j, (p, c) in enumerate(where)]
            elif prop.endswith('_scale'):
                rows += [(PLANES.index(prop[:-len('_scale')]), c, 2, lo[c], hi[c], i) for c in range(2)]
            else:
                rows += [(PLANES.index(prop), c, -1, lo[c], hi[c], i) for c in range(CHANNELS[prop])]
        return rows

    def __repr__(self):
        return f'Selection(codes={self.codes}, conds={self.conds}, ops={self.ops})'


def _device_of(*ts):
    return next((t.device for t in ts if torch.is_tensor(t) and t.is_cuda), torch.device('cuda'))


def _rows(t, ch, dev, name):
    t = torch.as_tensor(t).to(dev)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    t = t.reshape(-1, ch) if t.dim() != 2 or t.shape[1] != ch else t
    if t.dim() != 2 or t.shape[1] != ch:
        raise ValueError(f'{name} has {ch} channels, got {tuple(t.shape)}')
    return t.contiguous()


def _launch(props, selection, embed, mask, edit, dst, opt_scale, want_mask=True):
    props = props or {}
    dev = _device_of(*props.values(), embed, mask, *(edit or ()))
    planes, terms, ops, n_conds, codes = [None] * len(PLANES), (), (), 0, None
    if selection is not None:
        missing = [p for p in selection.needs() if props.get(p) is None]
        if missing:
            raise ValueError(f'the selection reads {missing}, which `props` does not hold')
        for p in selection.needs():
            planes[PLANES.index(p)] = _rows(props[p], CHANNELS[p], dev, p)
        terms, ops, n_conds, codes = selection.terms(), [_OPS[o] for o in selection.ops], len(selection.conds), selection.codes
        if codes is not None and embed is None:
            raise ValueError('a selection by codes needs `embed`, the code label of every row')
    if embed is not None:
        embed = torch.as_tensor(embed).to(dev).reshape(-1)
        if embed.dtype == torch.bool:
            raise ValueError('embed holds code labels (integers, or the float embed image), got bool')
        if embed.dtype not in (torch.int32, torch.float32):
            embed = embed.to(torch.float32 if embed.is_floating_point() else torch.int32)
        embed = embed.contiguous()
    if mask is not None:
        mask = torch.as_tensor(mask).to(dev).reshape(-1)
        mask = (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()
    if edit is not None:
        edit = tuple(_rows(t, ch, dev, k) for t, ch, k in zip(edit, (3, 3, 1), ('albedo', 'spec', 'rough')))
        dst = [float(x) for k, ch in (('diff', 3), ('spec', 3), ('rough', 1)) for x in np.broadcast_to(np.asarray(dst[k], np.float32).reshape(-1), (ch,))]
    sized = [t for t in planes if t is not None] + [t for t in (embed, mask) if t is not None] + list(edit or ())
    if not sized:
        raise ValueError('nothing to select from: no property, embed or mask')
    n = sized[0].shape[0]
    if any(t.shape[0] != n for t in sized):
        raise ValueError(f'the inputs differ in their row counts: {[t.shape[0] for t in sized]}')
    return _C.material_select_edit(n, planes, embed, mask, terms, ops, n_conds, codes, EPS, edit, dst, opt_scale, want_mask=want_mask)


def _result(mask, counts):
    h = _C.MATEDIT_HEAD_WORDS
    return {'mask': mask, 'selected': counts[0], 'invalid': counts[2], 'per_code': counts[h:h + _C.MATEDIT_CODES]}


def select(props, selection, embed=None, mask=None):
    """props: {'rgb' | 'xyz' | 'diff' | 'spec': [n, 3], 'rough': [n, 1]} (only what the selection reads is needed); embed: the code
    label of every row, integers or the float `embed` image (rounded to nearest-even), needed for a selection by codes; mask: rows
    to restrict the selection to.
    -> {'mask': uint8 [n] (0 / 1), 'selected', 'invalid' (rows whose label is outside [0, 64]): int64 scalars, 'per_code': int64 [65],
        the selected rows of each label}, all on the device, one launch, no host synchronisation."""
    if not isinstance(selection, Selection):
        raise ValueError(f'expected a Selection, got {type(selection).__name__}')
    m, counts, _ = _launch(props, selection, embed, mask, None, None, None)
    return _result(m, counts)


def apply(albedo, spec, rough, mask, dst, opt_scale=None):
    """dst = {'diff': [3], 'spec': [3], 'rough': [1]}: a material whose FIRST component is negative is left alone (vq_nfr.py:325-330);
    otherwise a row with mask != 0 takes the constant and any other row keeps its value.
    -> (albedo', spec', rough'), with opt_scale [3] also (albedo' * opt_scale, spec' * opt_scale) after them.  One launch."""
    _, _, out = _launch(None, None, None, mask, (albedo, spec, rough), dst, opt_scale, want_mask=False)
    return out


def select_apply(props, selection, albedo, spec, rough, dst, embed=None, mask=None, opt_scale=None):
    """select(...) and apply(...) of its mask in the ONE launch; the selection reads the pre-edit values.
    -> (the dict of select, the tuple of apply)"""
    if not isinstance(selection, Selection):
        raise ValueError(f'expected a Selection, got {type(selection).__name__}')
    m, counts, out = _launch(props, selection, embed, mask, (albedo, spec, rough), dst, opt_scale)
    return _result(m, counts), out


# ---- the models' side: fast_render(edit_select=..., edit_rows=..., edit_props=...) of vq_nfr.Model and ref_nfr.Model ----
def check_edit_keywords(edit_mask, edit_material, edit_select, edit_rows, edit_props):
    """the argument rules of the two models' new keywords, before any launch -> whether the kernel does this call's edit"""
    if edit_select is None and edit_rows is None:
        return False
    if edit_mask is not None:
        raise ValueError('edit_mask together with edit_select / edit_rows: one call takes one form of the selection')
    if edit_material is None:
        raise ValueError('edit_select / edit_rows without edit_material: nothing to replace the selected material with')
    if edit_select is not None:
        if not isinstance(edit_select, Selection):
            raise ValueError(f'edit_select is a material_edit.Selection, got {type(edit_select).__name__}')
        if 'rgb' in edit_select.needs() and (edit_props is None or edit_props.get('rgb') is None):
            raise ValueError("a condition on rgb / rgb_scale needs edit_props={'rgb': tensor [n, 3]}: the rendered colour of this "
                             'view is not known before the edit')
    return True


def edit_rows_of_a_view(fg, albedo, spec, rough, xyz, embed, edit_material, edit_select, edit_rows, edit_props, opt_scale):
    """One launch for a view's foreground rows.  fg: the row indices of the foreground (None: every row); albedo / spec / rough /
    xyz / embed (1-based code index): foreground rows; edit_rows / edit_props: over ALL rows.
    -> (the selection uint8 [foreground rows] or None without edit_select, albedo', spec', rough', albedo' * opt_scale,
    spec' * opt_scale -- the last two are albedo', spec' themselves when opt_scale is None)"""
    rows = None
    if edit_rows is not None:
        rows = torch.as_tensor(edit_rows).to(albedo.device).reshape(-1)
        rows = rows if fg is None else rows[fg]
    if edit_select is None:
        picked, out = None, apply(albedo, spec, rough, rows, edit_material, opt_scale)
    else:
        props = {'diff': albedo, 'spec': spec, 'rough': rough, 'xyz': xyz}
        if 'rgb' in edit_select.needs():
            rgb = torch.as_tensor(edit_props['rgb']).to(albedo.device).reshape(-1, 3)
            props['rgb'] = rgb if fg is None else rgb[fg]
        res, out = select_apply(props, edit_select, albedo, spec, rough, edit_material, embed=embed.to(torch.int32), mask=rows,
                                opt_scale=opt_scale)
        picked = res['mask']
    return (picked,) + tuple(out[:3]) + (tuple(out[3:5]) if opt_scale is not None else (out[0], out[1]))
