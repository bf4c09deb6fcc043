"""Cameras along a path for the fly-through video: mirror of geo/NeuS-ours2/models/hwvideo.py.

`VideoSet(train_set, cameras='transforms_test.json')` has no images: its poses come from the `frames[*].transform_matrix` of the camera
file (a nested list, or the comma-separated string some exporters write), everything else -- H, W, focal, cx, cy, near, far, max_radius,
the bounding box -- from the training set it is built on.  When the file is not in the set's `data_dir` it is looked for two
directories up, as the reference does (hwvideo.py:27-31).  `gen_rays_at` and `near_far_from_sphere` are those of models/nerfset.py:
geo/gen_geo.py's `extract_video` walks it like any other set."""
import json
import os

import numpy as np
import torch

from vqnerf_release_amd.geo.models import nerfset


def parse_pose(m):
    """transform_matrix, nested list or 'a,b,c,...' -> float32 [4, 4]"""
    if isinstance(m, str):
        m = [float(x) for x in m.split(',')]
    a = np.asarray(m, np.float32)
    if a.size != 16:
        raise ValueError(f'a transform_matrix has 16 entries, got {a.size}')
    return a.reshape(4, 4)


def find_cameras(data_dir, cameras):
    path = os.path.join(data_dir, cameras)
    if not os.path.exists(path):
        path = os.path.join(os.path.dirname(os.path.dirname(data_dir)), cameras)
    if not os.path.exists(path):
        raise FileNotFoundError(f'{cameras} is neither in {data_dir} nor two directories up')
    return path


class VideoSet(nerfset.Dataset):
    def __init__(self, train_set, cameras='transforms_test.json'):      # (no images to load: the parent's constructor is not run)
        self.device, self.conf = train_set.device, train_set.conf
        self.data_dir = train_set.data_dir
        self.render_cameras_name = self.object_cameras_name = cameras
        self.near, self.far, self.longint = train_set.near, train_set.far, getattr(train_set, 'longint', True)
        self.cameras_path = find_cameras(self.data_dir, cameras)
        with open(self.cameras_path) as f:
            self.camera_dict = json.load(f)
        self.n_images = len(self.camera_dict['frames'])
        if self.n_images == 0:
            raise ValueError(f'{self.cameras_path}: no frames')
        self.cx, self.cy = train_set.cx, train_set.cy
        self.pose_all = torch.from_numpy(np.stack([parse_pose(fr['transform_matrix']) for fr in self.camera_dict['frames']])).to(self.device)
        self.H, self.W, self.focal = train_set.H, train_set.W, train_set.focal
        self.image_pixels = self.H * self.W
        self.max_radius = train_set.max_radius
        self.object_bbox_min, self.object_bbox_max = train_set.object_bbox_min, train_set.object_bbox_max
        self.images = self.masks = None

    def gen_rays_at(self, img_idx, resolution_level=1, gen_mask=False):
        if gen_mask:
            raise ValueError('a camera path has no masks')
        return super().gen_rays_at(img_idx, resolution_level=resolution_level)

    def gen_random_rays_at(self, img_idx, batch_size):
        raise ValueError('a camera path has no images to draw pixels from')

    def image_at(self, idx, resolution_level):
        raise ValueError('a camera path has no images')

    def metadata(self, idx):
        """what the video loader of the decomp half reads per view (gen_video.py:165-169)"""
        none = lambda v: None if v is None else float(v)
        return {'focal': float(self.focal), 'cx': none(self.cx), 'cy': none(self.cy), 'cam_transform_mat': self.pose_all[idx].cpu().numpy().tolist()}
