"""CPU: the host side of the fly-through video path -- camera-path parsing (geo/models/videoset.py), the view discovery of the video
loader (decomp/nerfactor/datasets/video_nfr.py) on a written directory tree, and the stream names of decomp/video.py."""
import json
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests.decomp_util import make_config
from tests.test_datasets import _pose, _write_blender_set


def _train_set(root):
    from vqnerf_release_amd.geo import conf as hocon
    from vqnerf_release_amd.geo.models.nerfset import Dataset
    _write_blender_set(root, n=2, H=6, W=8)
    return Dataset(hocon.parse_string('dataset { data_dir = %s\n longint = false }' % root)['dataset'], device='cpu')


def _write_path(path, poses, as_str):
    frames = [{'transform_matrix': ','.join(repr(float(v)) for v in p.reshape(-1)) if s else p.tolist()} for p, s in zip(poses, as_str)]
    with open(path, 'w') as f:
        json.dump({'camera_angle_x': 0.6911, 'frames': frames}, f)


def test_videoset_parses_both_pose_forms_and_takes_the_rest_from_the_training_set(tmp_path):
    from vqnerf_release_amd.geo.models.videoset import VideoSet, parse_pose
    root = str(tmp_path / 'a' / 'b' / 'scene')
    ds = _train_set(root)
    poses = [_pose(0.2 * i) for i in range(4)]
    _write_path(os.path.join(root, 'transforms_test.json'), poses, [False, True, False, True])
    vs = VideoSet(ds)
    assert vs.n_images == 4 and vs.pose_all.dtype == torch.float32
    np.testing.assert_array_equal(vs.pose_all.numpy(), np.stack(poses).astype(np.float32))
    assert (vs.H, vs.W, vs.focal, vs.near, vs.far, vs.max_radius, vs.cx, vs.cy) == (ds.H, ds.W, ds.focal, ds.near, ds.far, ds.max_radius, None, None)
    assert vs.object_bbox_min is ds.object_bbox_min and vs.object_bbox_max is ds.object_bbox_max
    # the contract of nerfset: rays of the path's poses through the training set's intrinsics
    ds.pose_all = vs.pose_all[:2]
    for got, want in zip(vs.gen_rays_at(1, resolution_level=2), ds.gen_rays_at(1, resolution_level=2)):
        assert got.shape == (3, 4, 3) and torch.equal(got, want)
    near, far = vs.near_far_from_sphere(*vs.gen_rays_at(0))
    assert near.shape == (6, 8, 1) and float(near[0, 0, 0]) == ds.near and float(far[0, 0, 0]) == ds.far
    assert vs.metadata(3) == {'focal': float(ds.focal), 'cx': None, 'cy': None, 'cam_transform_mat': poses[3].astype(np.float32).tolist()}
    with pytest.raises(ValueError, match='no masks'):
        vs.gen_rays_at(0, gen_mask=True)
    with pytest.raises(ValueError, match='16 entries'):
        parse_pose('1,2,3')


def test_videoset_falls_back_two_directories_up(tmp_path):
    from vqnerf_release_amd.geo.models.videoset import VideoSet
    root = str(tmp_path / 'a' / 'b' / 'scene')
    ds = _train_set(root)
    with pytest.raises(FileNotFoundError, match='two directories up'):
        VideoSet(ds)
    _write_path(str(tmp_path / 'a' / 'transforms_test.json'), [_pose(0.1)], [True])
    vs = VideoSet(ds)
    assert vs.n_images == 1 and vs.cameras_path == str(tmp_path / 'a' / 'transforms_test.json')
    _write_path(os.path.join(root, 'path2.json'), [_pose(0.1), _pose(0.2)], [False, False])
    assert VideoSet(ds, cameras='path2.json').n_images == 2           # the set's own directory comes first


def _write_view(d, with_lvis=True, skip=None, H=4, W=6):
    os.makedirs(d)
    rng = np.random.default_rng(len(d))
    nrm = rng.normal(size=(H, W, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm[0, 0] = 0.0                                                    # zero: becomes (0, 1, 0)
    nrm[0, 1] = (0.5, 0.0, 0.0)                                        # not of unit length: becomes (0, 1, 0)
    alpha = np.zeros((H, W), np.uint8)
    alpha[1:, 1:] = 255
    files = {'xyz.npy': lambda p: np.save(p, rng.normal(size=(H, W, 3)).astype(np.float32)), 'normal.npy': lambda p: np.save(p, nrm),
             'alpha.png': lambda p: Image.fromarray(alpha).save(p),
             'rgb.png': lambda p: Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(p),
             'metadata.json': lambda p: json.dump({'focal': 7.5, 'cx': None, 'cy': None, 'cam_transform_mat': _pose(0.3).tolist()}, open(p, 'w'))}
    if with_lvis:
        files['lvis.npy'] = lambda p: np.save(p, rng.uniform(-0.2, 1.2, (H, W, 5)).astype(np.float32))
    for name, write in files.items():
        if name != skip:
            write(os.path.join(d, name))


def test_video_nfr_globs_strides_and_skips_incomplete_views(tmp_path):
    from vqnerf_release_amd.decomp.nerfactor.datasets import get_dataset_class
    video = tmp_path / 'geo' / 'video'
    for i in range(5):
        _write_view(str(video / f'test_{i:03d}'), skip='normal.npy' if i == 3 else None)
    _write_view(str(video / 'val_000'))                                # not a path view
    _write_view(str(video / 'test_0005'))                              # not test_???
    cfg = make_config(model='ref_nfr', dataset='video_nfr', data_nerf_root=str(tmp_path / 'geo' / 'surf'), imh=4)
    Dataset = get_dataset_class('video_nfr')
    ds = Dataset(cfg, 'test', device='cpu')
    ids = lambda d: [os.path.basename(os.path.dirname(f)) for f in d.files]
    assert ids(ds) == ['test_000', 'test_001', 'test_002', 'test_004'] and ids(Dataset(cfg, 'test', device='cpu', interp=2)) == ['test_000', 'test_002', 'test_004']
    assert [os.path.basename(os.path.dirname(f)) for f in ds.incomplete_paths] == ['test_003']
    assert ids(Dataset(cfg, 'test', device='cpu', interp=3)) == ['test_000']                     # the stride runs over ALL sorted views: 0, 3 (incomplete)
    assert ds.bs == 24
    id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal, ref, lvis = ds.view(1)
    assert id_ == ['test_001'] and tuple(hw[0].tolist()) == (4, 6) and lvis.shape == (24, 5) and 0.0 <= float(lvis.min()) and float(lvis.max()) <= 1.0
    assert torch.equal(alpha, pred_alpha) and set(alpha.unique().tolist()) == {0.0, 1.0}
    np.testing.assert_allclose(rayo.numpy(), np.tile(_pose(0.3)[:3, 3].astype(np.float32), (24, 1)))
    want_d = np.stack([(np.arange(6) - 3.0) / 7.5, np.zeros(6) + 2.0 / 7.5, -np.ones(6)], -1) @ _pose(0.3)[:3, :3].T      # pixel row 0: y = 0, cy = 2
    np.testing.assert_allclose(rayd.numpy()[:6], want_d, atol=1e-6)
    assert torch.equal(normal[0], torch.tensor([0.0, 1.0, 0.0])) and torch.equal(normal[1], torch.tensor([0.0, 1.0, 0.0]))
    assert torch.allclose(normal.norm(dim=-1), torch.ones(24), atol=1e-6)
    px = np.asarray(Image.open(video / 'test_001' / 'rgb.png')).reshape(-1, 3) / 255.0
    np.testing.assert_allclose(ref.numpy(), px, atol=1e-7)                                       # the base colour
    a = alpha.numpy()
    np.testing.assert_allclose(rgb.numpy(), px * a + 1.0 * (1 - a), atol=1e-7)                   # over the white background
    # without visibility files a 'nerf' set has no view; another data type does not read them
    for i in range(5):
        os.remove(video / f'test_{i:03d}' / 'lvis.npy')
    with pytest.raises(AssertionError, match='No file'):
        Dataset(cfg, 'test', device='cpu')
    hw_cfg = make_config(model='ref_nfr', dataset='video_nfr', data_type='hw', data_nerf_root=str(tmp_path / 'geo' / 'surf'), imh=4)
    assert len(Dataset(hw_cfg, 'test', device='cpu').view(0)) == 10


def test_stream_names():
    from vqnerf_release_amd.decomp import video
    probes, olats = ['city', 'night'], ['0000-0000', '0000-0001', '0001-0000', '0001-0001']
    names = lambda *a, **k: [s[0] for s in video.stream_names(*a, **k)]
    assert names('lego', 'recon', probes, olats, 2, vq=True) == ['lego_rgb']
    assert names('lego', 'relight', probes, olats, 2) == ['lego_rgb', 'lego_city', 'lego_night']
    assert video.stream_names('lego', 'relight', probes, olats, 2)[2] == ('lego_night', 'ref', 'pred_rgb_probes', 1)
    assert names('lego', 'relight', probes, olats, 2, vq=True) == ['lego_rgb', 'lego_city', 'lego_night', 'lego_vq_city', 'lego_vq_night']
    assert names('lego', 'edit', probes, olats, 2, vq=True) == names('lego', 'relight', probes, olats, 2, vq=True)
    # OLAT maps: the top half of the light grid only, ahead of the probes, where the model renders them
    got = video.stream_names('lego', 'relight', probes, olats, 2, vq=True, vq_olat=True)
    assert [s[0] for s in got] == ['lego_rgb', 'lego_city', 'lego_night', 'lego_vq_0000-0000', 'lego_vq_0000-0001', 'lego_vq_city', 'lego_vq_night']
    assert got[3] == ('lego_vq_0000-0000', 'vq', 'pred_rgb_olat', 0) and got[5] == ('lego_vq_city', 'vq', 'pred_rgb_probes', 0)
    with pytest.raises(ValueError, match='share a name'):
        video.stream_names('lego', 'relight', ['rgb'], [], 0)
    with pytest.raises(ValueError, match='mode is one of'):
        video.stream_names('lego', 'gen_comps')


def test_run_refuses_before_it_renders():
    from vqnerf_release_amd.decomp import video
    model = types.SimpleNamespace(white_bg=True)
    ds = types.SimpleNamespace(files=[])
    with pytest.raises(ValueError, match='belong to mode edit'):
        video.run(model, ds, 'out', 'relight', dst={'diff': [0, 0, 0]})
    with pytest.raises(ValueError, match='either a selection or a mask_dir'):
        video.run(model, ds, 'out', 'edit', selection=object(), mask_dir='x')
    with pytest.raises(ValueError, match='material_edit.Selection'):
        video.run(model, ds, 'out', 'edit', selection=object(), dst={})
