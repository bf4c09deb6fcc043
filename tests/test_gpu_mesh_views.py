"""GPU: meshes drawn from dataset cameras (geo/mesh_render.py) -- a marching-cubes sphere against its analytic silhouette and depth,
Runner.validate_mesh_image / evaluate_mesh_views on a runner whose dataset has masks, and decomp/material_mesh.run(views=...)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.test_mesh_raster_model import look_at

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RADIUS, RES = 0.75, 48
STEP = 2.0 / (RES - 1)


@pytest.fixture(scope='module')
def sphere():
    """the project's device marching cubes on the grid of an analytic sphere SDF -> (vertices, triangles)"""
    from vqnerf_release_amd.geo import mesh
    g = torch.linspace(-1.0, 1.0, RES, device='cuda')
    x, y, z = torch.meshgrid(g, g, g, indexing='ij')
    u = (RADIUS - torch.sqrt(x * x + y * y + z * z)).contiguous()
    return mesh.marching_cubes(u, 0.0, origin=(-1.0, -1.0, -1.0), step=(STEP, STEP, STEP))


def pinhole_rays(eye, focal, H, W):
    """unit f32 rays through the pixels (i, j) of a pin-hole camera at `eye` looking at the origin, as a dataset's gen_rays_at gives them"""
    _, R, K = look_at(eye, focal, ((W - 1) / 2.0, (H - 1) / 2.0))
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    d = np.stack([j, i, np.ones_like(i)], -1).astype(np.float64) @ np.linalg.inv(K).T @ R
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.asarray(eye, np.float64), d.shape)
    return torch.tensor(o, dtype=torch.float32, device='cuda'), torch.tensor(d, dtype=torch.float32, device='cuda')


@pytest.mark.parametrize('eye', [(0.3, 0.4, 2.6), (-1.9, 1.1, -1.5)])
def test_sphere_silhouette_and_depth(sphere, eye):
    from vqnerf_release_amd.geo import mesh_render
    v, t = sphere
    H = W = 96
    rays_o, rays_d = pinhole_rays(eye, 100.0, H, W)
    P = mesh_render.camera_from_rays(rays_o, rays_d)
    out = mesh_render.render(v, t, P, H, W)
    assert out['stats']['bad_index'] == out['stats']['unusable_vertex'] == out['stats']['culled'] == 0 and out['stats']['pairs'] >= t.shape[0] // 2
    o, d = rays_o.double(), rays_d.double()
    along = -(o * d).sum(-1)                                                      # the ray's closest approach to the centre
    dist = (o + along[..., None] * d).norm(dim=-1)
    # the mesh lies within one cell of the sphere: outside that band the silhouette is the analytic one
    sure = (dist < RADIUS - STEP) | (dist > RADIUS + STEP)
    assert sure.float().mean() > 0.8 and (dist < RADIUS - STEP).sum() > 1000
    assert torch.equal(out['mask'][sure], (dist < RADIUS)[sure])
    # on rays within 0.8 r the surface is met at cos >= 0.6, so a radial error of one cell is at most step / 0.6 < 2 step along the ray
    near = dist < 0.8 * RADIUS
    hit = along - torch.sqrt((RADIUS ** 2 - dist ** 2).clamp(min=0))
    axis = torch.as_tensor(P[2, :3], device='cuda').double()
    want = hit * (d @ axis)
    err = (out['depth'].double() - want).abs()[near]
    assert near.sum() > 500 and float(err.max()) <= 2 * STEP, float(err.max())
    assert float(err.max()) > 0 and torch.isinf(out['depth'][~out['mask']]).all()
    # normals: unit, towards the camera on the mesh, the diagonal off it
    n = out['normal']
    assert torch.allclose(n.norm(dim=-1), torch.ones_like(n[..., 0]), atol=1e-5)
    assert ((n * rays_d).sum(-1)[out['mask']] <= 0.05).all()                      # (turned by the face's centre: a cell subtends 0.02 rad)
    assert torch.allclose(n[~out['mask']], torch.full((3,), 1 / math.sqrt(3.0), device='cuda'))
    radial = torch.nn.functional.normalize(rays_o + out['depth'][..., None] / (rays_d @ axis.float())[..., None] * rays_d, dim=-1)
    assert float((n * radial).sum(-1)[near].min()) > 0.9                          # ... and along the sphere's own normal
    # culling one winding leaves the front of a closed surface as it is, culling the other shows its back
    faces = [mesh_render.rasterize(v, t, P, H, W, cull=c) for c in (1, -1)]
    same = [torch.equal(f['face'], out['face']) for f in faces]
    assert sorted(same) == [False, True]
    back = faces[same.index(False)]
    # (the chord of a ray within 0.8 r is at least 1.2 r, seen within 0.3 rad of the axis, each end within 2 step)
    assert (back['depth'][near] > out['depth'][near] + 0.9 * RADIUS).all() and back['stats']['culled'] > 1000
    u8 = mesh_render.to_uint8(out)
    assert u8['mask'].dtype == torch.uint8 and set(u8['mask'].unique().tolist()) == {0, 255}
    assert int(u8['depth'][out['mask']].max()) == 255 and int(u8['depth'][out['mask']].min()) == 0
    assert torch.equal(u8['normal'], (n * 128 + 128).clip(0, 255).to(torch.uint8))


def test_render_colours_and_labels(sphere):
    from vqnerf_release_amd.decomp.nerfactor.util.segmentation import PD_PALETTE
    from vqnerf_release_amd.geo import mesh_render
    v, t = sphere
    H = W = 64
    P = mesh_render.camera_from_rays(*pinhole_rays((0.3, 0.4, 2.6), 64.0, H, W))
    labels = (v[:, 0] > 0).int() * 3 + (v[:, 1] > 0).int()                        # codes 0, 1, 3, 4
    colors = (v * 0.5 + 0.5).clamp(0, 1)
    out = mesh_render.render(v, t, P, H, W, normals=torch.nn.functional.normalize(v, dim=-1), colors=colors, labels=labels)
    m = out['mask']
    assert set(out['label_index'][m].unique().tolist()) == {0, 1, 3, 4} and (out['label_index'][~m] == -1).all()
    assert torch.equal(out['label'][m], torch.as_tensor(PD_PALETTE, device='cuda')[out['label_index'][m]]) and not out['label'][~m].any()
    assert (out['color'][~m] == 1.0).all()
    # the interpolated colour of a point of the sphere is its position, to the chord error of a cell
    depth = torch.where(m, out['depth'], torch.zeros_like(out['depth']))
    axis = torch.as_tensor(P[2, :3], device='cuda')
    rays_o, rays_d = pinhole_rays((0.3, 0.4, 2.6), 64.0, H, W)
    x = rays_o + (depth / (rays_d @ axis))[..., None] * rays_d
    assert float((out['color'] - (x * 0.5 + 0.5))[m].abs().max()) < STEP
    assert float((out['normal'] * torch.nn.functional.normalize(x, dim=-1)).sum(-1)[m].min()) > 0.99
    u8 = mesh_render.to_uint8(out)
    assert torch.equal(u8['color'], (out['color'].clamp(0, 1) * 255.0).to(torch.uint8)) and u8['label'] is out['label']


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runner(tmp_path_factory):
    import re
    from tests.test_datasets import _write_blender_set
    from vqnerf_release_amd.geo.nerf_runner import Runner
    tmp = tmp_path_factory.mktemp('mesh_views')
    data = tmp / 'scene'
    data.mkdir()
    _write_blender_set(str(data), n=3, H=24, W=32)
    text = open(os.path.join(HERE, 'golden', 'neus_like.conf')).read().replace('./exp/', str(tmp) + '/exp/')
    text = re.sub(r'data_dir = [^\n]*', 'data_dir = %s/\n    longint = false' % data, text, count=1)
    torch.manual_seed(0)
    r = Runner(conf_text=text, case='views')
    r.renderer.perturb = 0.0
    return r


def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_validate_mesh_image_writes_what_it_returns(runner):
    r = runner
    path = r.validate_mesh(resolution=32, normals=True, colors=True)
    imgs = r.validate_mesh_image(idx=1, resolution_level=1)
    out_dir = os.path.join(r.base_exp_dir, 'mesh_views')
    assert sorted(os.listdir(out_dir)) == ['00000000_0_1_%s.png' % k for k in ('color', 'depth', 'mask', 'normal')]
    assert sorted(imgs) == ['color', 'depth', 'mask', 'normal']
    for name, arr in imgs.items():
        assert arr.dtype == np.uint8 and arr.shape[:2] == (24, 32)
        np.testing.assert_array_equal(_decode(os.path.join(out_dir, '00000000_0_1_%s.png' % name)), arr)
    assert imgs['mask'].max() == 255 and 0 < (imgs['mask'] > 0).mean() < 1 and imgs['depth'][imgs['mask'] > 0].max() == 255
    assert (imgs['depth'][imgs['mask'] == 0] == 0).all() and (imgs['color'][imgs['mask'] == 0] == 255).all()
    bg = imgs['normal'][imgs['mask'] == 0]
    assert (bg == int(128 / math.sqrt(3) + 128)).all()
    # a PLY without colours and normals: no colour image, face normals; at half the size
    from vqnerf_release_amd.geo import mesh
    v, t, _ = mesh.read_ply(path)
    plain = os.path.join(r.base_exp_dir, 'plain.ply')
    mesh.write_ply(plain, v, t)
    half = r.validate_mesh_image(idx=2, resolution_level=2, mesh_path=plain)
    assert sorted(half) == ['depth', 'mask', 'normal'] and half['mask'].shape == (12, 16)
    assert not os.path.exists(os.path.join(out_dir, '00000000_0_2_color.png')) and os.path.exists(os.path.join(out_dir, '00000000_0_2_mask.png'))


@pytest.mark.parametrize('level', [1, 2])
def test_evaluate_mesh_views_scores_against_the_masks(runner, level):
    from vqnerf_release_amd.geo import mesh, mesh_render
    r = runner
    path = r.validate_mesh(resolution=32)
    got = r.evaluate_mesh_views(resolution_level=level, volume=(level == 2))
    assert got == json.load(open(os.path.join(r.base_exp_dir, 'meshes', '00000000_views.json')))
    v, t, _ = mesh.read_ply(path)
    assert got['mesh'] == '00000000.ply' and got['n_faces'] == t.shape[0] and [row['view'] for row in got['views']] == [0, 1, 2]
    ds = r.dataset
    H, W = ds.H // level, ds.W // level
    ious = []
    for idx, row in enumerate(got['views']):
        P = mesh_render.camera_from_rays(*ds.gen_rays_at(idx, resolution_level=level))
        mask = mesh_render.rasterize(v, t, P, H, W)['face'] >= 0
        ty = torch.round(torch.linspace(0, ds.H - 1, H)).long()
        tx = torch.round(torch.linspace(0, ds.W - 1, W)).long()
        gt = (ds.masks[idx, :, :, 0] > 0.5)[ty.cuda()][:, tx.cuda()]
        want = float((mask & gt).sum() / (mask | gt).sum())
        assert row['iou'] == want and 0 < want < 1 and row['mesh_pixels'] == int(mask.sum()) and (row['H'], row['W']) == (H, W)
        ious.append(want)
    assert got['mean']['iou'] == float(np.mean(ious)) and got['stats']['bad_index'] == 0 and got['stats']['pairs'] > 0
    if level == 2:
        for row in got['views']:
            assert 0 <= row['iou_volume'] <= 1 and row['depth_pixels'] >= 0
            assert (row['depth_abs_mean'] is None) == (row['depth_pixels'] == 0)
            assert row['depth_pixels'] == 0 or 0 <= row['depth_abs_median'] < 4.0
        assert set(got['mean']) == {'iou', 'iou_volume', 'depth_abs_mean', 'depth_abs_median'}
    else:
        assert set(got['mean']) == {'iou'} and 'iou_volume' not in got['views'][0]
    assert r.evaluate_mesh_views(views=[2], resolution_level=level)['views'][0]['iou'] == ious[2]


def test_evaluate_mesh_views_needs_masks(runner):
    from vqnerf_release_amd.geo.nerf_runner import Runner, SyntheticDataset
    text = open(os.path.join(HERE, 'golden', 'neus_like.conf')).read().replace('./exp/', runner.base_exp_dir + '/nomask/')
    r = Runner(conf_text=text, case='views', dataset=SyntheticDataset(n_images=2, H=16, W=16))
    with pytest.raises(ValueError, match='masks'):
        r.evaluate_mesh_views(mesh_path='unused.ply')


# ---- material meshes -----------------------------------------------------------------------------------------------------------------
def test_material_mesh_views(sphere, tmp_path):
    from tests.test_gpu_vq_entrypoints import _build
    from vqnerf_release_amd.decomp import material_mesh
    from vqnerf_release_amd.decomp.nerfactor.util.segmentation import PD_PALETTE
    from vqnerf_release_amd.geo import mesh, mesh_render
    model = _build('nerf', 8)[3]
    v, t = sphere
    today = ['material_mesh.json', 'material_mesh.mtl', 'material_mesh.obj', 'material_mesh.ply']
    rec0 = material_mesh.run(model, (v, t), str(tmp_path / 'none'))
    assert sorted(os.listdir(str(tmp_path / 'none'))) == today and 'views' not in rec0
    views = [(mesh_render.camera_from_rays(*pinhole_rays(eye, 60.0, H, W)), H, W) for eye, H, W in (((0.3, 0.4, 2.6), 64, 64), ((-1.9, 1.1, -1.5), 40, 56))]
    out = str(tmp_path / 'views')
    rec = material_mesh.run(model, (v, t), out, views=views)
    names = ['material_mesh_view_%03d_%s.png' % (i, k) for i in range(2) for k in ('albedo', 'material', 'rough')]
    assert sorted(os.listdir(out)) == sorted(today + names)
    assert {k: rec[k] for k in rec0} == rec0 and [(w['H'], w['W']) for w in rec['views']] == [(64, 64), (40, 56)]
    for name in today[1:]:
        assert open(os.path.join(out, name), 'rb').read() == open(str(tmp_path / 'none' / name), 'rb').read(), name
    label = mesh.read_ply(os.path.join(out, 'material_mesh.ply'), extra=['material'])[3]['material']
    allowed = {tuple(int(c) for c in PD_PALETTE[k]) for k in label.unique().tolist()} | {(0, 0, 0)}
    for i, (P, H, W) in enumerate(views):
        mat = _decode(os.path.join(out, 'material_mesh_view_%03d_material.png' % i))
        assert mat.shape == (H, W, 3) and {tuple(c) for c in mat.reshape(-1, 3).tolist()} <= allowed
        mask = (mesh_render.rasterize(v, t, P, H, W)['face'] >= 0).cpu().numpy()
        assert np.array_equal(mat.any(-1), mask) and rec['views'][i]['pixels'] == int(mask.sum()) > 200
        albedo, rough = (_decode(os.path.join(out, 'material_mesh_view_%03d_%s.png' % (i, k))) for k in ('albedo', 'rough'))
        assert albedo.shape == (H, W, 3) and (albedo[~mask] == 255).all() and rough.shape == (H, W) and (rough[~mask] == 0).all()
