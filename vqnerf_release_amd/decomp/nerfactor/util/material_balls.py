"""Material balls: every material of a list as a lit sphere under every light probe of a list -- the reference's
decomp/nerfvq_nfr3/brdf/renderer.py SphereRenderer (numpy, one BRDF per call, used there only to build the MERL dataset) as one
launch of csrc/material_balls.hip (include/vqn_material_balls.h states the geometry and the shading).

  render      materials [M, 7] x lights [P, L, 3] -> the linear float images and / or their 8-bit sRGB form, on the device
  sheet       the same balls tiled into one contact sheet per probe, in a given order
  load_light  the reference's two synthetic probes, 'white' and 'point', as arrays (probe FILES go through the models' _load_light)
  material_row  a dst material of the editing driver ({'diff', 'spec', 'rough'}) as a row of `materials`

One deviation from the reference, stated in the header: a sample's surface point is the exact sphere point above it (an orthographic
lift); the reference back-projects a depth map through a perspective camera and gets points close to the sphere."""
import math

import numpy as np
import torch

from vqnerf_release_amd import _C

MATERIAL_FLOATS = 7              # albedo[3], f0[3], rough[1]


def load_light(name, h=16):
    """'white': ones [h, 2 h, 3]; 'point': zeros with a 4 x 4 patch of ones (renderer.py:222-233) -> float64 array"""
    h = int(h)
    if name == 'white':
        return np.ones((h, 2 * h, 3), dtype=float)
    if name == 'point':
        env = np.zeros((h, 2 * h, 3), dtype=float)
        i, j, d = -h // 4, -int(2 * h * 7 / 8), 2
        env[(i - d):(i + d), (j - d):(j + d), :] = 1
        return env
    raise ValueError(f"load_light: 'white' or 'point', got {name!r} (probe files are read by the models' _load_light)")


def material_row(dst):
    """{'diff': [3], 'spec': [3], 'rough': [1]} (decomp/edit.py's dst) -> float32 [7]"""
    row = np.concatenate([np.asarray(dst[k], np.float32).reshape(-1) for k in ('diff', 'spec', 'rough')])
    if row.size != MATERIAL_FLOATS:
        raise ValueError(f'a material is diff[3], spec[3], rough[1], got {row.size} values')
    return row


def _device_inputs(materials, lights, lxyz, areas):
    dev = materials.device if torch.is_tensor(materials) else (lights.device if torch.is_tensor(lights) else torch.device('cuda'))
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=dev).detach().contiguous()
    areas = t(areas).reshape(-1)
    L = areas.numel()
    materials, lights, lxyz = t(materials).reshape(-1, MATERIAL_FLOATS), t(lights).reshape(-1, L, 3), t(lxyz).reshape(L, 3)
    _C.require_device(materials, 'material_balls')
    return materials, lights, lxyz, areas


def render(materials, lights, lxyz, areas, ims=128, spp=4, sphere_radius=0.4, cam_rot=None, white_bg=True, gamma=None,
           want_f32=True, want_u8=True):
    """materials [M, 7] = albedo, f0, rough; lights [P, L, 3] or [P, h, w, 3]; lxyz, areas as gen_light_xyz gives them (arrays or
    tensors; copied to the device of `materials` when they are not there).  gamma: None or the pair (g0, g1) of (rgb g0) ^ g1.
    -> (f32 [M, P, ims, ims, 3] linear | None, u8 [M, P, ims, ims, 3] sRGB bytes | None), device tensors."""
    out = _C.material_balls(*_device_inputs(materials, lights, lxyz, areas), ims, spp, sphere_radius=sphere_radius, cam_rot=cam_rot,
                            white_bg=white_bg, gamma=gamma, want_f32=want_f32, want_u8=want_u8)
    return out['f32'], out['u8']


def sheet_shape(n, cols=None):
    """(rows, cols) of a sheet of n balls: `cols` across (default: the next integer from sqrt(n))"""
    cols = int(cols) if cols else max(1, math.ceil(math.sqrt(n)))
    return (n + cols - 1) // cols, cols


def sheet(materials, lights, lxyz, areas, order=None, cols=None, ims=128, spp=4, sphere_radius=0.4, cam_rot=None, white_bg=True,
          gamma=None, want_u8=False):
    """The contact sheet uint8 [P, rows ims, cols ims, 3]: ball order[i] (default 0 .. M - 1) at cell (i // cols, i % cols), the cells
    past the last ball in the background colour.  want_u8: also the single images -> (sheet, u8 | None)."""
    materials, lights, lxyz, areas = _device_inputs(materials, lights, lxyz, areas)
    n = materials.shape[0] if order is None else len(order)
    rows, cols = sheet_shape(n, cols)
    out = _C.material_balls(materials, lights, lxyz, areas, ims, spp, sphere_radius=sphere_radius, cam_rot=cam_rot, white_bg=white_bg,
                            gamma=gamma, want_f32=False, want_u8=want_u8, sheet=(order, rows, cols))
    return out['sheet'], out['u8']
