"""Mean-shift baseline of the segmentation table: the counterpart of the reference's decomp/nerfvq_nfr3/meanshift.py on the device
clustering of decomp/nerfactor/util/meanshift.py.

`run(pred_scene, data_scene, dst_scene, bandwidth)` reads, for every `train_*` and `val_*` directory under `pred_scene` (the
continuous model's renderings), `albedo.png` and `spec.png` as RGB and `rough.png` as one channel -- 7 byte features per pixel, each
read as k / 255. -- and the mask alpha > 0 from `data_scene/<view>/rgba.png` (walk, loaders, size check: decomp/view_tree.py).  A size
mismatch raises; nothing is resized.  The masked pixels of the training views, subsampled to `n_samples` by a seeded permutation on the device
(the reference's cap of 10,000 answers sklearn's speed on the host; `n_samples=None` keeps every pixel), are clustered; every masked
pixel of the validation views gets the label of its nearest centre.  Written:

    dst_scene/center.npy                          the centres, float64 [K, 7]
    dst_scene/batch<NNNNNNNNN>/labels.npy         uint8 [H, W]: label + 1 on masked pixels, 0 elsewhere
    dst_scene/batch<NNNNNNNNN>/labels.png         value i as `segmentation.PD_PALETTE[i - 1]` (R, G, B), black for 0

NNN is the number in the view's own name (`val_007` -> `batch000000007`), which is what `cluster_eval` pairs on; the reference
numbers the views in the order its directory listing returns them.  The files are then scored by
`cluster_eval.evaluate(dst_scene, label_root, data_root, pred_file='labels.png')`."""
import os

import numpy as np
import torch

from vqnerf_release_amd.decomp import view_tree
from vqnerf_release_amd.decomp.nerfactor.util import segmentation
from vqnerf_release_amd.decomp.nerfactor.util.meanshift import MeanShift

FILES = ('albedo.png', 'spec.png', 'rough.png')


def _view(pred_scene, data_scene, view, files):
    """-> (uint8 features [H, W, 7], mask [H, W])"""
    paths = [os.path.join(pred_scene, view, name) for name in files]
    planes = [view_tree.read_image(path, mode) for path, mode in zip(paths, ('RGB', 'RGB', 'L'))]
    alpha = view_tree.read_alpha(os.path.join(data_scene, view, 'rgba.png'))
    view_tree.check_sizes(view, dict([(path, p.shape[:2]) for path, p in zip(paths, planes)] + [('alpha', alpha.shape)]))
    return np.concatenate([p if p.ndim == 3 else p[..., None] for p in planes], axis=-1), alpha > 0


def run(pred_scene, data_scene, dst_scene, bandwidth, n_samples=10000, seed=0, files=FILES, device='cuda'):
    """-> {'centers': float64 [K, 7] (host), 'views': the batch directories written, 'n_fit': the pixels clustered, 'n_iter',
    'sample': those pixels, uint8 [n_fit, 7] on the device}.  See the module docstring."""
    device = torch.device(device)
    train, val = [], []
    for view in view_tree.view_dirs(pred_scene, view_tree.SCENE_VIEWS):
        z, mask = _view(pred_scene, data_scene, view, files)
        if view.startswith('train_'):
            train.append(z[mask])
        else:
            val.append((view, z, mask))
    if not train or not val:
        raise ValueError(f'{pred_scene}: needs train_* and val_* views, found {len(train)} and {len(val)}')
    x = torch.as_tensor(np.concatenate(train), device=device)                # uint8 [n, 7]
    if x.shape[0] == 0:
        raise ValueError(f'{pred_scene}: no training pixel has alpha > 0')
    if n_samples is not None and x.shape[0] > n_samples:
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        x = x[torch.randperm(x.shape[0], generator=g, device=device)[:int(n_samples)]]
    model = MeanShift(bandwidth, cluster_all=True).fit(x)
    centers = model.cluster_centers_.cpu().numpy()
    K = centers.shape[0]
    if K > len(segmentation.PD_PALETTE):
        raise ValueError(f'{K} clusters at bandwidth {bandwidth}: labels.png has {len(segmentation.PD_PALETTE)} colours')
    os.makedirs(dst_scene, exist_ok=True)
    np.save(os.path.join(dst_scene, 'center.npy'), centers)
    colours = np.concatenate([np.zeros((1, 3), np.uint8), segmentation.PD_PALETTE])
    from PIL import Image
    written = []
    for view, z, mask in val:
        im = np.zeros(mask.shape, np.uint8)
        if mask.any():
            im[mask] = model.predict(torch.as_tensor(z[mask], device=device)).cpu().numpy().astype(np.uint8) + 1
        out = view_tree.batch_view(view_tree.view_number(view))
        os.makedirs(os.path.join(dst_scene, out), exist_ok=True)
        np.save(os.path.join(dst_scene, out, 'labels.npy'), im)
        Image.fromarray(colours[im]).save(os.path.join(dst_scene, out, 'labels.png'))
        written.append(out)
    return {'centers': centers, 'views': written, 'n_fit': int(x.shape[0]), 'n_iter': model.n_iter_, 'sample': x}
