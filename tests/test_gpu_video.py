"""GPU: the fly-through video path end to end on a tiny scene (3 path poses, 24 x 20 pixels, 2 probes): geometry buffers along the camera
path (geo/gen_geo.py: extract_video over geo/models/videoset.py), the loader (decomp/nerfactor/datasets/video_nfr.py), and the driver
(decomp/video.py) in the modes relight, edit with a Selection and edit with the mask files the first edit wrote.  Every `00dc` chunk of
every stream must be the device JPEG of exactly the pixels `vis_batch` wrote as PNG for the same key (frames=True)."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.decomp_util import make_config
from tests.test_mjpeg_avi import walk

pytestmark = pytest.mark.gpu
H, W, N_VIEWS = 24, 20, 3
SCALE = [1.2, 0.9, 0.8]
DST = {'diff': [0.7, 0.2, 0.1], 'spec': [-1.0, -1.0, -1.0], 'rough': [0.35]}


@pytest.fixture(scope='module')
def path_scene(tmp_path_factory):
    """a Blender-format set with a camera path file, its VideoSet, and the extracted buffers"""
    from tests.test_datasets import _pose, _write_blender_set
    from tests.test_gpu_neus_render import _build
    from vqnerf_release_amd.geo import conf as hocon
    from vqnerf_release_amd.geo.gen_geo import GeoExtractor
    from vqnerf_release_amd.geo.models.nerfset import Dataset
    from vqnerf_release_amd.geo.models.videoset import VideoSet
    root = tmp_path_factory.mktemp('flythrough')
    assert 'surf' not in str(root)
    scene = str(root / 'scene')
    _write_blender_set(scene, n=3, H=H, W=W)
    poses = [_pose(0.3 + 0.25 * i) for i in range(N_VIEWS)]
    frames = [{'transform_matrix': p.tolist()} for p in poses]
    frames[1]['transform_matrix'] = ','.join(repr(float(v)) for v in poses[1].reshape(-1))        # the string form
    with open(os.path.join(scene, 'transforms_test.json'), 'w') as f:
        json.dump({'camera_angle_x': 0.6911, 'frames': frames}, f)
    ds = Dataset(hocon.parse_string('dataset { data_dir = %s\n longint = false }' % scene)['dataset'], device='cuda')
    vs = VideoSet(ds)
    cfg, sdf, col, var, ren = _build('small')
    ren.n_importance, ren.up_sample_steps, ren.perturb = 16, 4, 0.0
    ex = GeoExtractor(ren, max_radius=ds.max_radius, light_h=16, max_rays=8192)
    out = str(root / 'geo' / 'video')
    done = [ex.extract_video(vs, out, num_p=2, p_i=1), ex.extract_video(vs, out, num_p=2, p_i=0), ex.extract_video(vs, out)]
    return dict(root=root, vs=vs, ex=ex, out=out, done=done, poses=poses)


def test_extract_video_writes_the_views_and_resumes(path_scene):
    from vqnerf_release_amd.geo.gen_geo import GeoExtractor
    s = path_scene
    assert s['done'] == [[2], [0, 1], []]                              # the split of extract_views; a second call skips everything
    assert sorted(os.listdir(s['out'])) == ['test_000', 'test_001', 'test_002']
    for i in range(N_VIEWS):
        d = os.path.join(s['out'], f'test_{i:03d}')
        assert set(os.listdir(d)) == set(GeoExtractor.VIEW_FILES) | {'metadata.json'}
        meta = json.load(open(os.path.join(d, 'metadata.json')))
        assert set(meta) == {'focal', 'cx', 'cy', 'cam_transform_mat'} and meta['cx'] is None
        assert meta['focal'] == float(s['vs'].focal)
        np.testing.assert_array_equal(np.array(meta['cam_transform_mat'], np.float32), s['poses'][i].astype(np.float32))
        assert np.load(os.path.join(d, 'xyz.npy')).shape == (H, W, 3) and np.load(os.path.join(d, 'lvis.npy')).shape == (H, W, 512)
    alpha = np.asarray(Image.open(os.path.join(s['out'], 'test_000', 'alpha.png')))
    lv = np.load(os.path.join(s['out'], 'test_000', 'lvis.npy'))
    assert 10 < (alpha > 0).sum() and (lv[alpha == 0] == 0).all() and (lv[alpha > 0] != 0).any()      # visibility on the predicted mask
    os.remove(os.path.join(s['out'], 'test_001', 'metadata.json'))     # a view without its metadata is not finished
    assert s['ex'].extract_video(s['vs'], s['out']) == [1]


def _dataset(path_scene, **kw):
    from vqnerf_release_amd.decomp.nerfactor.datasets import get_dataset_class
    cfg = make_config(model='ref_nfr', dataset='video_nfr', data_nerf_root=str(path_scene['root'] / 'geo' / 'surf'), imh=H)
    return get_dataset_class('video_nfr')(cfg, 'test', **kw)


def test_video_nfr_loads_the_views_with_the_rays_of_the_videoset(path_scene):
    dset = _dataset(path_scene)
    assert dset.get_n_views() == N_VIEWS and dset.bs == H * W and _dataset(path_scene, interp=2).get_n_views() == 2
    for i in range(N_VIEWS):
        b = dset.view(i)
        assert len(b) == 11 and b[0] == [f'test_{i:03d}'] and tuple(b[1][0].tolist()) == (H, W)
        o, v = path_scene['vs'].gen_rays_at(i)
        assert torch.allclose(b[2].reshape(H, W, 3), o, atol=1e-6)
        d = b[3] / b[3].norm(dim=-1, keepdim=True)                     # the loader's directions are not normalised (video_nfr.py:316-317)
        assert torch.allclose(d.reshape(H, W, 3), v, atol=1e-5)
        assert torch.equal(b[5], b[6]) and b[10].shape == (H * W, 512) and b[9].shape == (H * W, 3)
        nn = b[8].norm(dim=-1)
        assert torch.allclose(nn, torch.ones_like(nn), atol=1e-5)


@pytest.fixture(scope='module')
def models():
    from tests.test_gpu_decomp import _ref_setup
    from tests.test_gpu_vq_entrypoints import _build
    ref = _ref_setup('nerf')[4]
    vq = _build('nerf', 8)[3]
    rng = np.random.default_rng(8)
    probes = {f'probe{i}': torch.tensor(rng.uniform(0, 2, (16, 32, 3)).astype(np.float32)).cuda() for i in range(2)}
    ref.novel_probes, vq.novel_probes = dict(probes), dict(probes)
    return ref, vq


def _png(path):
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


def _chunks(path):
    d = walk(open(path, 'rb').read())
    assert (d['w'], d['h']) == (W, H) and d['total'] == d['length'] == len(d['frames'])
    return d['frames']


STREAMS = {'toy_rgb': ('', 'pred_rgb'), 'toy_probe0': ('', 'pred_rgb_probes_probe0'), 'toy_probe1': ('', 'pred_rgb_probes_probe1'),
           'toy_vq_probe0': ('vq', 'pred_rgb_probes_probe0'), 'toy_vq_probe1': ('vq', 'pred_rgb_probes_probe1')}


def _check_against_the_pngs(root, files, quality=75):
    from vqnerf_release_amd.decomp.nerfactor.util import mjpeg
    assert sorted(files) == sorted(STREAMS)
    enc = mjpeg.JpegEncoder(quality=quality)
    out = {}
    for name, (sub, key) in STREAMS.items():
        assert files[name] == os.path.join(root, name + '.avi')
        chunks = _chunks(files[name])
        assert len(chunks) == N_VIEWS
        for i, c in enumerate(chunks):
            px = _png(os.path.join(root, sub, f'test_{i:03d}', key + '.png'))
            assert px.shape == (H, W, 3)
            assert c == enc.encode(torch.tensor(px[None]).cuda())[0], (name, i)
            im = Image.open(io.BytesIO(c))
            im.load()
            assert im.size == (W, H)
        out[name] = chunks
    return out


def test_relight_and_the_two_edits(path_scene, models, tmp_path):
    from vqnerf_release_amd.decomp import video
    from vqnerf_release_amd.decomp.nerfactor.util import material_edit as me
    ref, vq = models
    dset = _dataset(path_scene)
    root = str(tmp_path / 'video_relight')
    files = video.run(ref, dset, root, 'relight', vq_model=vq, opt_scale=SCALE, frames=True, scene='toy')
    relit = _check_against_the_pngs(root, files)
    assert len({c for cs in relit.values() for c in cs}) > N_VIEWS                   # streams and frames differ
    plain = video.run(ref, dset, str(tmp_path / 'plain'), 'recon', scene='toy')      # videos only: no frame directories
    assert list(plain) == ['toy_rgb'] and sorted(os.listdir(tmp_path / 'plain')) == ['toy_rgb.avi']
    assert _chunks(plain['toy_rgb']) == relit['toy_rgb']                             # rgb comes from the unscaled materials either way

    # a selection that picks part of the first view: its two most frequent codes, rows above their median roughness
    with torch.no_grad():
        base = vq.fast_render(dset.view(0), mode='test', gen_embed=True)[0]
    emb = base['embed'][:, 0].cpu().numpy().astype(np.int64)
    codes = [int(c) for c in np.argsort(-np.bincount(emb[emb > 0], minlength=9))[:2]]
    med = float(np.median(base['rough'].cpu().numpy()[np.isin(emb, codes), 0]))
    sel = me.Selection(codes, [('rough', med, 2.0)], [])
    root1, root2 = str(tmp_path / 'video_edit'), str(tmp_path / 'video_edit_masks')
    first = _check_against_the_pngs(root1, video.run(ref, dset, root1, 'edit', vq_model=vq, opt_scale=SCALE, selection=sel, dst=DST,
                                                     frames=True, scene='toy'))
    masks = [np.load(os.path.join(root1, 'auto_sel', f'test_{i:03d}.npy')) for i in range(N_VIEWS)]
    assert all(m.dtype == bool and m.shape == (H, W, 3) for m in masks) and masks[0].any() and not masks[0].all()
    assert json.load(open(os.path.join(root1, 'auto_sel', 'dst.json')))['rough'] == [0.35]
    second = _check_against_the_pngs(root2, video.run(ref, dset, root2, 'edit', vq_model=vq, opt_scale=SCALE,
                                                      mask_dir=os.path.join(root1, 'auto_sel'), frames=True, scene='toy'))
    assert first == second                                                           # the two edit runs agree, byte for byte
    assert first['toy_rgb'][0] != relit['toy_rgb'][0] and first['toy_vq_probe0'][0] != relit['toy_vq_probe0'][0]     # the edit took place

    with pytest.raises(ValueError, match='either a selection or a mask_dir'):
        video.run(ref, dset, root2, 'edit', vq_model=vq, dst=DST)
    with pytest.raises(ValueError, match='give vq_model'):
        video.run(ref, dset, root2, 'edit', selection=sel, dst=DST)
    with pytest.raises(ValueError, match='mode is one of'):
        video.run(ref, dset, root2, 'vq_dcomps')
