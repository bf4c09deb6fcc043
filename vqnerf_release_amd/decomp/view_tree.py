"""The per-view directory tree of a scene, as the drivers of decomp/ read it: which directories are views, which prediction view pairs
with which ground-truth view, how an image file becomes an array, and the file forms of the reference's selection window
(ui4_offline.py).  What `util/vis.py` is to the writers of that tree, this is to its readers: metric_eval, cluster_eval, meanshift,
edit and video keep no walk, loader, pairing rule or size check of their own.

    batch<NNNNNNNNN>/   what train_nfr.render_views, edit.run and meanshift.run write per view (`batch_view`)
    val_NNN/, train_NNN/  the data set's views and the renderings named after them (`gt_view`)
    test_NNN/           the frames of a camera path (`frame_view`)
    auto_sel/           <view>.npy, bool [H, W, 3], and dst.json: an edit's selection and replacement material

Views pair by NUMBER: `batch000000007` with `val_007`.  The reference pairs by the last three characters in some scripts and by the
integer in others; the two agree up to view 999, which covers every data set of the project, and only the integer is right beyond."""
import json
import os
import re

import numpy as np

BATCH_VIEWS = r'batch\d+'                    # the rendered views the evaluators score
EDIT_VIEWS = r'(batch|test).*'               # what the selection window lists (ui4_offline.py:288)
SCENE_VIEWS = r'(train|val)_\d+'             # the data set's views, as the mean-shift baseline reads them

_LABEL_MODES = ('L', 'I', 'I;16', 'I;16L', 'I;16B')


def view_dirs(root, pattern):
    """the sorted names of root's sub-directories whose whole name matches pattern"""
    return sorted(n for n in os.listdir(root) if re.fullmatch(pattern, n) and os.path.isdir(os.path.join(root, n)))


def view_number(name):
    return int(re.search(r'\d+$', name).group())


def gt_view(name_or_number):
    """the ground-truth directory of a view, by its name (`batch000000007`) or its number: `val_007`"""
    return 'val_%03d' % (name_or_number if isinstance(name_or_number, int) else view_number(name_or_number))


def batch_view(number):
    return 'batch%09d' % number


def frame_view(number):
    return 'test_%03d' % number


def read_image(path, mode='RGB'):
    """-> uint8 [H, W, 3 | 4] or [H, W] (mode 'L'), the file converted to the PIL mode"""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert(mode))


def read_alpha(path):
    return read_image(path, 'RGBA')[..., 3]


def read_colours_or_labels(path):
    """-> (array, is_label): uint8 [H, W, 3] colours, or int32 labels [H, W] for a single-channel integer file"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in _LABEL_MODES:
            return np.asarray(im).astype(np.int32), True
        return np.array(im.convert('RGB')), False


def check_sizes(where, sizes):
    """sizes: {path or label: (H, W)} of images that must match -> that (H, W); nothing is resized"""
    sizes = {k: tuple(v) for k, v in sizes.items()}
    if len(set(sizes.values())) != 1:
        raise ValueError(f'{where}: image sizes differ: ' + ', '.join(f'{k} {v}' for k, v in sizes.items()) + ' (resizing is not implemented)')
    return next(iter(sizes.values()))


# ---- the selection window's files (ui4_offline.py:267-271, :333-338) ----------------------------------------------------------------
def write_selection(path, mask_hw, event=None):
    """mask_hw [H, W], non-zero = selected -> path as bool [H, W, 3], which is returned.  event: the copy that fills mask_hw, waited for
    first (a job of vis.AsyncWriter)."""
    if event is not None:
        event.synchronize()
    m = np.repeat((np.asarray(mask_hw) != 0)[..., None], 3, axis=-1)
    np.save(path, m)
    return m


def read_selection(path, n):
    """-> bool [n]: the rows of a view of n pixels the file selects; one channel or three (gen_video.py:219-240)"""
    m = np.load(path)
    if m.size not in (n, 3 * n):
        raise ValueError(f'{path} has {m.size} entries, the view has {n} pixels (resizing is not implemented)')
    return m.reshape(n, -1)[:, 0] != 0


def write_dst(sel_dir, dst):
    os.makedirs(sel_dir, exist_ok=True)
    with open(os.path.join(sel_dir, 'dst.json'), 'w') as f:
        json.dump({k: [float(x) for x in np.asarray(dst[k], np.float64).reshape(-1)] for k in ('diff', 'spec', 'rough')}, f)


def read_dst(sel_dir):
    with open(os.path.join(sel_dir, 'dst.json')) as f:
        return json.load(f)
