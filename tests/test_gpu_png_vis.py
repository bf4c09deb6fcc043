"""GPU: `vis_batch(png='device')` against `vis_batch(png='host')` on the stub model and the view of tests/test_vis_output.py, with the
tensors on the device: the same file names, every PNG decoding to the same mode and pixels, every .npy and metadata.json the same
bytes.  (The PNG bytes differ on purpose: the device writes its own deflate stream; tests/test_gpu_png.py holds that to its model.)"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.gpu_util import launches
from tests.test_vis_output import _Stub, _view
from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.util import vis

pytestmark = pytest.mark.gpu


class _FixedStub(_Stub):
    """the stub with one codebook for both passes (the stub draws a new one per call, which vq_embed.npy would show)"""

    def __init__(self):
        super().__init__()
        self.codebook = torch.rand(256, 15)

    def get_codebook(self):
        return self.codebook


def _on_device(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def _files(root):
    return sorted(os.path.relpath(os.path.join(r, f), root) for r, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize('H,W', [(6, 9), (12, 20)])
@pytest.mark.parametrize('mode', ['vali', 'test'])
def test_device_files_decode_to_the_host_files(tmp_path, H, W, mode):
    m, d = _FixedStub(), _on_device(_view(H, W, seed=H))
    roots = {}
    for png in ('host', 'device'):
        roots[png] = tmp_path / png
        full = str(roots[png] / 'full') if mode == 'vali' else None
        with launches() as rec:
            w = vis.vis_batch(m, d, str(roots[png] / 'vis' / 'batch000'), mode=mode, alpha_thres=0.8, full_vis_path=full, png=png,
                              metrics=H == 12)                               # (the larger view also with the device's scores)
            w.flush()
        assert rec.counts.get('vqn_png_encode', 0) == (2 if png == 'device' else 0), rec.counts      # the colour batch and the grey batch
    names = _files(roots['host'])
    assert names == _files(roots['device'])
    assert 'vis/batch000/pred_rgb.png' in names and 'vis/batch000/embed_map.png' in names and 'vis/batch000/metadata.json' in names
    n_png = 0
    for name in names:
        a, b = roots['host'] / name, roots['device'] / name
        if name.endswith('.png'):
            ia, ib = Image.open(a), Image.open(b)
            assert ia.mode == ib.mode and ia.size == ib.size, name
            assert np.array_equal(np.asarray(ia), np.asarray(ib)), name
            n_png += 1
        else:
            assert a.read_bytes() == b.read_bytes(), name
    assert n_png >= 12
    if mode == 'vali':
        meta = (roots['device'] / 'vis' / 'batch000' / 'metadata.json').read_text()
        assert 'psnr' in meta and ('ssim' in meta) == (H == 12)


def test_simp_and_unknown_values(tmp_path):
    m, d = _FixedStub(), _on_device(_view(6, 9))
    for png in ('host', 'device'):
        vis.vis_batch(m, d, str(tmp_path / png / 'v' / 'b'), mode='vali', simp=True, png=png).flush()
    assert _files(tmp_path / 'host') == _files(tmp_path / 'device')
    assert 'v/b/metadata.json' not in _files(tmp_path / 'device') and 'v/b/gt_alpha.png' not in _files(tmp_path / 'device')
    with pytest.raises(ValueError, match="'host' or 'device'"):
        vis.vis_batch(m, d, str(tmp_path / 'x'), mode='test', png='gpu')
    with pytest.raises(_C.VqnError, match='no CPU fallback'):
        vis.vis_batch(m, _view(6, 9), str(tmp_path / 'y'), mode='test', png='device')
    assert not (tmp_path / 'y').exists()
