"""CPU: the two homes of the scene output tree's rules.  Writer side: the table `vis.view_files` and the image former `vis.view_image`
against the files `vis_batch(png='host')` writes -- formed from torch CPU tensors, which is the branch the device writer takes.  Reader
side: decomp/view_tree.py -- the walk, the pairing by view number, the loaders, the size check and the selection window's files."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests.test_vis_output import _Stub, _view
from vqnerf_release_amd.decomp import view_tree
from vqnerf_release_amd.decomp.nerfactor.util import vis

Image = pytest.importorskip('PIL.Image')


def _files(root, ext):
    return sorted(os.path.relpath(os.path.join(r, f), root) for r, _, fs in os.walk(root) for f in fs if f.endswith(ext))


@pytest.mark.parametrize('H,W', [(1, 1), (6, 9), (12, 20)])
@pytest.mark.parametrize('mode,simp', [(m, s) for m in ('vali', 'test', 'render') for s in (False, True)])
def test_table_against_the_files_of_the_host_path(tmp_path, H, W, mode, simp):
    m, d = _Stub(), _view(H, W, seed=H)
    out = tmp_path / 'vis' / 'batch000'
    full = tmp_path / 'full' if mode == 'vali' else None
    vis.vis_batch(m, d, str(out), mode=mode, alpha_thres=0.8, simp=simp, full_vis_path=full and str(full), png='host').flush()
    # the entries as images, torch CPU tensors: [N, 1] -> [H, W], [N, ...] -> [H, W, ...]
    t = {k: v.to(torch.float32).reshape((H, W) + (() if v.shape[1:] == (1,) else tuple(v.shape[1:])))
         for k, v in d.items() if torch.is_tensor(v) and k != 'hw'}
    images, arrays = vis.view_files({k: tuple(v.shape) for k, v in t.items()}, mode, simp, full is not None, *vis.light_names(m))
    alpha = vis.threshold_alpha(t['gt_alpha'], 0.8)
    stems = [stem for stem, _, _, _ in images]
    assert len(set(stems)) == len(stems) and sorted(s + '.png' for s in stems) == _files(out, '.png')
    assert 'pred_rgb' in stems and 'embed_map' in stems and 'pred_rgb_probes_forest' in stems
    for stem, k, light, kind in images:
        img = vis.view_image(t[k], light, kind, alpha, m.white_bg)
        assert torch.is_tensor(img) and img.dtype == torch.uint8, stem
        assert np.array_equal(img.numpy(), np.asarray(Image.open(out / (stem + '.png')))), stem
    want = sorted((os.path.join('full' if where == 'full_vis_path' else os.path.join('vis', 'batch000'), k + '.npy'), k) for k, where in arrays)
    assert [f for f, _ in want] == [f for f in _files(tmp_path, '.npy') if os.path.basename(f) not in ('np_light.npy', 'vq_embed.npy')]      # (those: once per run)
    for f, k in want:
        assert np.array_equal(np.load(tmp_path / f), t[k].numpy()), f
    assert os.path.exists(out / 'metadata.json') == (not simp)


def test_embed_map_in_both_forms_and_its_inverse():
    e = np.array([list(range(19)) + [19.0, -1.0, 2.5, 3.5]], np.float32)                     # 2.5 -> 2, 3.5 -> 4: round half to even
    want = np.zeros(e.shape + (3,), np.uint8)
    for i, c in enumerate(e[0]):
        code = {2.5: 2, 3.5: 4}.get(float(c), int(c))
        if 1 <= code <= 18:
            want[0, i] = vis._EMBED_COLOURS[code - 1][::-1]
    got_np, got_t = vis.embed_map(e), vis.embed_map(torch.as_tensor(e))
    assert got_np.dtype == np.uint8 and got_t.dtype == torch.uint8 and got_np.shape == e.shape + (3,)
    assert np.array_equal(got_np, want) and np.array_equal(got_t.numpy(), want)
    codes = np.arange(19, dtype=np.float32).reshape(1, 19)
    labels = vis.embed_labels(vis.embed_map(codes), 'cpu')
    assert labels.dtype == torch.int32 and labels.tolist() == list(range(19))
    assert vis.embed_labels(np.array([[[1, 2, 3]]], np.uint8), 'cpu').tolist() == [0]       # no code's colour


def test_walk_and_pairing(tmp_path):
    for name in ('batch000000007', 'batch7x', 'val_007', 'train_003', 'test_012', 'test_0005'):
        os.makedirs(tmp_path / name)
    (tmp_path / 'batch000000008').write_text('a file')
    root = str(tmp_path)
    isdir = lambda n: os.path.isdir(os.path.join(root, n))
    # the filters the five drivers held, restated
    old = {view_tree.BATCH_VIEWS: [n for n in sorted(os.listdir(root)) if re.fullmatch(r'batch\d+', n) and isdir(n)],
           view_tree.EDIT_VIEWS: [n for n in sorted(os.listdir(root)) if (n.startswith('batch') or n.startswith('test')) and isdir(n)],
           view_tree.SCENE_VIEWS: sorted(n for n in os.listdir(root) if re.fullmatch(r'(train|val)_\d+', n) and isdir(n))}
    assert old[view_tree.BATCH_VIEWS] == ['batch000000007'] and old[view_tree.SCENE_VIEWS] == ['train_003', 'val_007']
    assert old[view_tree.EDIT_VIEWS] == ['batch000000007', 'batch7x', 'test_0005', 'test_012']
    for pattern, want in old.items():
        assert view_tree.view_dirs(root, pattern) == want, pattern
    assert view_tree.gt_view('batch000000007') == 'val_007' == view_tree.gt_view(7) and view_tree.batch_view(7) == 'batch000000007'
    assert view_tree.view_number('val_007') == 7 and view_tree.frame_view(12) == 'test_012' and view_tree.view_number('test_0005') == 5
    assert view_tree.gt_view('batch000001234') == 'val_1234'                                  # by number, not by the last three characters
    for i in (0, 9, 10, 99, 100, 999):                                                         # up to 999 the old rules and this one agree
        name = 'batch%09d' % i
        assert view_tree.gt_view(name) == 'val_' + name[-3:] == 'val_{i:03d}'.format(i=int(name[len('batch'):]))
        assert view_tree.batch_view(view_tree.view_number(view_tree.gt_view(name))) == name


def test_loaders_and_size_check(tmp_path):
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    Image.fromarray(rgba).save(tmp_path / 'rgba.png')
    Image.fromarray(rgba[..., 0]).save(tmp_path / 'grey.png')
    Image.fromarray(rng.integers(0, 60000, (5, 7)).astype(np.uint16)).save(tmp_path / 'idx16.png')
    got = view_tree.read_image(str(tmp_path / 'rgba.png'))
    assert got.dtype == np.uint8 and np.array_equal(got, rgba[..., :3])
    assert np.array_equal(view_tree.read_image(str(tmp_path / 'rgba.png'), 'RGBA'), rgba)
    alpha = view_tree.read_alpha(str(tmp_path / 'rgba.png'))
    assert alpha.dtype == np.uint8 and np.array_equal(alpha, rgba[..., 3])
    assert (view_tree.read_alpha(str(tmp_path / 'grey.png')) == 255).all()                      # a file without alpha is opaque
    grey = view_tree.read_image(str(tmp_path / 'grey.png'), 'L')
    assert grey.dtype == np.uint8 and np.array_equal(grey, rgba[..., 0])
    assert np.array_equal(view_tree.read_image(str(tmp_path / 'grey.png')), np.repeat(rgba[..., :1], 3, axis=-1))
    labels, is_label = view_tree.read_colours_or_labels(str(tmp_path / 'idx16.png'))
    assert is_label and labels.dtype == np.int32 and np.array_equal(labels, np.asarray(Image.open(tmp_path / 'idx16.png')))
    labels, is_label = view_tree.read_colours_or_labels(str(tmp_path / 'grey.png'))
    assert is_label and labels.dtype == np.int32 and np.array_equal(labels, rgba[..., 0])
    colours, is_label = view_tree.read_colours_or_labels(str(tmp_path / 'rgba.png'))
    assert not is_label and colours.dtype == np.uint8 and np.array_equal(colours, rgba[..., :3])
    assert view_tree.check_sizes('view', {'a.png': (16, 15), 'b.png': torch.Size([16, 15]), 'alpha': (16, 15)}) == (16, 15)
    with pytest.raises(ValueError, match='sizes differ') as err:
        view_tree.check_sizes('batch000000007', {'a.png': (16, 14), 'alpha': (16, 15)})
    assert '(resizing is not implemented)' in str(err.value) and 'a.png (16, 14)' in str(err.value) and 'alpha (16, 15)' in str(err.value)


def test_selection_files(tmp_path):
    mask = (np.arange(24).reshape(4, 6) % 5 == 0).astype(np.uint8)
    path = str(tmp_path / 'test_003.npy')
    written = view_tree.write_selection(path, mask)
    on_disk = np.load(path)
    assert on_disk.dtype == bool and on_disk.shape == (4, 6, 3) and np.array_equal(on_disk, written)
    assert np.array_equal(on_disk, np.repeat((mask != 0)[..., None], 3, axis=-1))
    rows = view_tree.read_selection(path, 24)
    assert rows.dtype == bool and rows.shape == (24,) and np.array_equal(rows, mask.reshape(-1) != 0)
    np.save(tmp_path / 'one.npy', mask)                                                        # one channel reads the same
    assert np.array_equal(view_tree.read_selection(str(tmp_path / 'one.npy'), 24), rows)
    with pytest.raises(ValueError, match=r'test_003\.npy has 72 entries, the view has 23 pixels \(resizing is not implemented\)'):
        view_tree.read_selection(path, 23)
    dst = {'diff': np.float32([0.7, 0.2, 0.1]), 'spec': [-1, -1, -1], 'rough': 0.35, 'unused': 1}
    view_tree.write_dst(str(tmp_path / 'auto_sel'), dst)
    want = {'diff': [float(np.float32(x)) for x in (0.7, 0.2, 0.1)], 'spec': [-1.0, -1.0, -1.0], 'rough': [0.35]}
    assert view_tree.read_dst(str(tmp_path / 'auto_sel')) == want == json.load(open(tmp_path / 'auto_sel' / 'dst.json'))
