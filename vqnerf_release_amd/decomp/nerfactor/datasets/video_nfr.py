"""Loader of the fly-through video: mirror of decomp/nerfvq_nfr3/nerfactor/datasets/video_nfr.py -- the buffers geo/gen_geo.py's
`extract_video` wrote along a camera path, in the batch layout of the stage-3 loader (datasets/ref_nfr.py:
`id, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal, ref[, lvis]`), which both reflectance models read.

What differs from datasets/shape_unit.py, as in the reference: the views are `test_???` under `data_nerf_root` with `surf` replaced by
`video` (:40-55) and there is no `data_root` side at all -- `metadata.json` lies next to the buffers; every `interp`-th of the sorted
views is taken (:61); rays come from that file's `focal`, `cx`, `cy` and `cam_transform_mat` (:228-239; the dtu branch from `intrinsic`
and `cam_transform_mat`, :218-226) at the size of xyz.npy; there is no ground truth, so alpha = pred_alpha = alpha.png and rgb is the
NeuS render rgb.png composited over the configured background (:242-248, :277-280), which is also the extra map `ref`; normals that
are zero or not of unit length become (0, 1, 0) before the normalisation (:269-273); `lvis` is read only for `data_type == 'nerf'`."""
import json
import os
from glob import glob
from os.path import join

import numpy as np

from vqnerf_release_amd.decomp.nerfactor.datasets import shape_unit


class Dataset(shape_unit.Dataset):
    def __init__(self, config, mode, debug=False, device='cuda', interp=1):
        self.interp = max(int(interp), 1)
        super().__init__(config, mode, debug=debug, device=device)

    def _glob(self):
        cfg = self.config
        nerf_root = self.nerf_root = cfg.get('DEFAULT', 'data_nerf_root').replace('surf', 'video')
        self.data_type = cfg.get('DEFAULT', 'data_type')
        self.model_name = cfg.get('DEFAULT', 'model', fallback='')
        pattern = join(nerf_root, 'test_002' if self.debug else 'test_???')
        metadata_paths, self.incomplete_paths = [], []
        for metadata_path in sorted(glob(join(pattern, 'metadata.json')))[::self.interp]:
            id_ = self._parse_id(metadata_path)
            paths = {'xyz': join(nerf_root, id_, 'xyz.npy'), 'normal': join(nerf_root, id_, 'normal.npy'),
                     'alpha': join(nerf_root, id_, 'alpha.png'), 'basecolor': join(nerf_root, id_, 'rgb.png')}
            if self.data_type == 'nerf':
                paths['lvis'] = join(nerf_root, id_, 'lvis.npy')
            if all(os.path.exists(p) for p in paths.values()):
                metadata_paths.append(metadata_path)
                self.meta2buf[metadata_path] = paths
            else:
                self.incomplete_paths.append(metadata_path)
        return metadata_paths

    def _load_data(self, metadata_path):
        """-> (id, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal, ref[, lvis]) as [H,W,...] float32 arrays."""
        white_bg = self.config.getboolean('DEFAULT', 'white_bg')
        id_ = self._parse_id(metadata_path)
        with open(metadata_path) as f:
            metadata = json.load(f)
        paths = self.meta2buf[metadata_path]
        xyz, normal = np.load(paths['xyz']), np.load(paths['normal']).copy()
        imh, imw = xyz.shape[:2]
        m = metadata['cam_transform_mat']
        cam_to_world = np.array([float(x) for x in m.split(',')] if isinstance(m, str) else m, np.float64).reshape(4, 4)
        if self.data_type == 'dtu':
            intrinsic = np.array(metadata['intrinsic'], np.float64).reshape(4, 4)
            rayo, rayd = self._gen_rays(cam_to_world, np.linalg.inv(intrinsic), imh, imw)
        else:
            rayo, rayd = self._gen_rays(cam_to_world, metadata['focal'], imh, imw, metadata.get('cx'), metadata.get('cy'))
        rayo, rayd = rayo.astype(np.float32), rayd.astype(np.float32)

        alpha = pred_alpha = shape_unit.read_image_normalized(paths['alpha'])
        basecolor = shape_unit.read_image_normalized(paths['basecolor'])
        if basecolor.ndim == 2:
            basecolor = np.repeat(basecolor[:, :, None], 3, 2)
        basecolor = basecolor[:, :, :3]
        fit = lambda a: shape_unit.resize_hw(a, imh) if a.shape[0] != imh else a
        alpha, pred_alpha, basecolor = fit(alpha), fit(pred_alpha), fit(basecolor)

        normal[np.mean(normal, axis=-1) == 0.0] = np.array([0.0, 1.0, 0.0])
        normal[~np.isclose(np.linalg.norm(normal, axis=2), 1)] = np.array([0.0, 1.0, 0.0])
        normal = normal / np.linalg.norm(normal, axis=2, keepdims=True)
        bg = np.ones_like(basecolor) if white_bg else np.zeros_like(basecolor)
        rgb = (basecolor * alpha[..., None] + bg * (1.0 - alpha[..., None])).astype(np.float32)
        out = (id_, rayo, rayd, rgb, alpha.astype(np.float32), pred_alpha.astype(np.float32), xyz.astype(np.float32),
               normal.astype(np.float32), basecolor.astype(np.float32))
        if self.data_type == 'nerf':
            out = out + (np.clip(fit(np.load(paths['lvis'])), 0, 1).astype(np.float32),)
        return out

    def _gen_rays(self, to_world, intrinsic, imh, imw, cx=None, cy=None):
        """as shape_unit's, but the pin-hole branch is handed the focal length itself (video_nfr.py:312-317)"""
        if self.data_type == 'dtu':
            return super()._gen_rays(to_world, intrinsic, imh, imw)
        rayo = np.tile(to_world[:3, 3][None, None, :], (imh, imw, 1))
        xs, ys = np.meshgrid(np.linspace(0, imw, imw, endpoint=False), np.linspace(0, imh, imh, endpoint=False))
        cx = 0.5 * imw if cx is None else cx
        cy = 0.5 * imh if cy is None else cy
        rayd = np.stack(((xs - cx) / intrinsic, -(ys - cy) / intrinsic, -np.ones_like(xs)), axis=-1)
        return rayo, np.sum(rayd[:, :, np.newaxis, :] * to_world[:3, :3], axis=-1)
