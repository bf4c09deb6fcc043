"""CPU: the float64 model of the material-ball renderer (tests/material_balls_model.py) against closed forms, and the numpy side of
decomp/nerfactor/util/material_balls.py (load_light) against the model's restatement."""
import numpy as np
import pytest

from tests import material_balls_model as mb


def _lights(h=16):
    xyz, areas = mb.gen_light_xyz(h, 2 * h)
    return xyz.reshape(-1, 3), areas.reshape(-1)


def test_areas_sum_to_four_pi():
    for h in (8, 16):
        assert abs(_lights(h)[1].sum() - 4 * np.pi) < 1e-12


def test_white_probe_diffuse_ball_centre_is_the_albedo_within_the_grid_error():
    # the centre sample of an odd grid lies at (0.5, 0.5): normal = toward the camera.  With f0 = 0 the glossy part still has the
    # Schlick tail, so the diffuse part is checked on its own: albedo / pi * sum cos area over the front-lit lights, which would be the
    # albedo if the sum were the integral pi; the light grid's discretisation error is that sum's distance from pi, computed here
    lxyz, areas = _lights()
    white = mb.load_light('white').reshape(1, -1, 3)
    albedo = np.array([0.7, 0.4, 0.2])
    mats = np.concatenate([albedo, np.zeros(3), [0.5]])[None]
    fg, xyz, normal, cam = mb.geometry(1, 1)
    assert fg.shape == (1, 1) and fg[0, 0] and np.allclose(xyz[0], [0.0, -0.4, 0.0]) and np.allclose(normal[0], [0.0, -1.0, 0.0])
    _, diff, _, _ = mb.shade(xyz, normal, cam, mats, white, lxyz, areas, parts=True)
    l = lxyz - xyz[0]
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    cos = l @ normal[0]
    integral = (np.where(cos > 0, cos, 0.0) * areas).sum() / np.pi               # 1 for an exact quadrature
    grid_error = abs(integral - 1.0)
    assert grid_error < 0.05                                                     # (a 16 x 32 grid is a few percent off)
    assert np.all(np.abs(diff[0, 0, 0] - albedo) <= albedo * grid_error * (1 + 1e-9) + 1e-15)
    assert np.allclose(diff[0, 0, 0], albedo * integral, rtol=1e-12)


def test_glossy_part_is_zero_where_the_view_grazes():
    # v . n = 0: G1(v.n) = divide_no_nan(0, ...) = 0 and the denominator 4 |l.n| |v.n| = 0 -> divide_no_nan gives 0, never NaN
    lxyz, areas = _lights()
    cam = np.array([0.0, -10.0, 0.0])
    xyz = np.array([[0.4, -10.0, 0.0]])                                          # the camera sees this point edge-on
    normal = np.array([[0.0, 0.0, 1.0]])
    mats = np.array([[0.5, 0.5, 0.5, 0.04, 0.5, 1.0, 0.3], [0.1, 0.2, 0.3, 1.0, 1.0, 1.0, 1e-3]])
    out, diff, gloss, _ = mb.shade(xyz, normal, cam, mats, mb.load_light('white').reshape(1, -1, 3), lxyz, areas, parts=True)
    assert np.all(gloss == 0.0) and np.all(np.isfinite(out)) and np.all(diff > 0)


def test_averaging_a_constant_image_gives_the_constant():
    for spp in (1, 4, 9, 16):
        sps = mb.sps_of(spp)
        img = np.full((5 * sps, 5 * sps, 2, 3), 0.3)
        assert np.allclose(mb.average(img, spp), 0.3, rtol=0, atol=1e-16) and mb.average(img, spp).shape == (5, 5, 2, 3)
    img = np.arange(16.0).reshape(4, 4)
    assert np.array_equal(mb.average(img, 4), [[2.5, 4.5], [10.5, 12.5]])


def test_sheet_puts_ball_i_at_cell_i_div_cols_i_mod_cols():
    M, P, ims, rows, cols = 5, 2, 3, 2, 3
    u8 = np.zeros((M, P, ims, ims, 3), np.uint8)
    for m in range(M):
        u8[m] = 10 * (m + 1) + np.arange(P)[:, None, None, None]
    sh = mb.sheet(u8, None, rows, cols, white_bg=True)
    assert sh.shape == (P, rows * ims, cols * ims, 3)
    for i in range(rows * cols):
        cell = sh[:, (i // cols) * ims:(i // cols + 1) * ims, (i % cols) * ims:(i % cols + 1) * ims]
        assert np.array_equal(cell, u8[i]) if i < M else np.all(cell == 255)
    order = [4, 2, 0]
    sh = mb.sheet(u8, order, 1, 4, white_bg=False)
    for i in range(4):
        cell = sh[:, :, i * ims:(i + 1) * ims]
        assert np.array_equal(cell, u8[order[i]]) if i < 3 else np.all(cell == 0)


def test_grid_and_mask_follow_the_reference_scene():
    # the f32 grid against np.linspace in float64 (the reference's statement), and the mask's area against the disc's
    for ims, spp in ((1, 1), (8, 4), (33, 9), (128, 4)):
        sps = mb.sps_of(spp)
        w = 1 / (sps + 1)
        want = np.linspace(w, ims - w, ims * sps) / ims
        assert np.allclose(mb.grid(ims, spp), want, rtol=0, atol=2e-7)
    _, _, fg, hz2 = mb.samples(128, 4)
    assert abs(fg.mean() - np.pi * 0.16) < 2e-3 and np.all(hz2 >= 0)
    assert not mb.samples(8, 1)[2][0, 0] and mb.samples(1, 1)[2][0, 0]


def test_the_default_camera_lights_the_top_of_the_ball_from_the_top_rows_of_the_probe():
    lxyz, areas = _lights()
    top = np.zeros((16, 32, 3))
    top[:4] = 1.0                                                                # the probe's top rows: the zenith, +Z
    mats = np.array([[0.8, 0.8, 0.8, 0.0, 0.0, 0.0, 1.0]])
    img = mb.render(mats, top.reshape(1, -1, 3), lxyz, areas, 9, 1, white_bg=False)[0, 0]
    assert img[1, 4].sum() > 5 * img[7, 4].sum() and img[4, 4].sum() > 0         # row 1 is the top of the image


def test_load_light_is_the_models_restatement():
    from vqnerf_release_amd.decomp.nerfactor.util import material_balls
    for name in ('white', 'point'):
        for h in (8, 16):
            got = material_balls.load_light(name, h)
            assert got.shape == (h, 2 * h, 3) and np.array_equal(got, mb.load_light(name, h))
    assert mb.load_light('point', 16).sum() == 16 * 3                            # a 4 x 4 patch
    with pytest.raises(ValueError):
        material_balls.load_light('sunset')


def test_python_constants_equal_the_defines_of_the_header():
    from tests import abi_headers
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.decomp.nerfactor.util import material_balls
    d = abi_headers.defines('vqn_material_balls.h')
    assert d['VQN_MATBALLS_MAX_MATERIALS'] == _C.MATBALLS_MAX_MATERIALS and d['VQN_MATBALLS_MAX_PROBES'] == _C.MATBALLS_MAX_PROBES
    assert d['VQN_MATBALLS_SCRATCH_PER_LIGHT'] == _C.MATBALLS_SCRATCH_PER_LIGHT and d['VQN_MATBALLS_MAX_OUT_BYTES'] == _C.MATBALLS_MAX_OUT_BYTES
    assert d['VQN_MATBALLS_MATERIAL_FLOATS'] == material_balls.MATERIAL_FLOATS
    assert set(d) == {'VQN_MATBALLS_MAX_MATERIALS', 'VQN_MATBALLS_MAX_PROBES', 'VQN_MATBALLS_LIGHT_STEP', 'VQN_MATBALLS_MAX_LIGHTS',
                      'VQN_MATBALLS_MAX_IMS', 'VQN_MATBALLS_MAX_SPS', 'VQN_MATBALLS_MATERIAL_FLOATS', 'VQN_MATBALLS_SCRATCH_PER_LIGHT',
                      'VQN_MATBALLS_SUM_BLOCK', 'VQN_MATBALLS_MAX_OUT_BYTES'}
