"""Times of the mesh rasteriser (geo/mesh_render.py: rasterize, render; csrc/mesh_raster.hip) at 800 x 800 on a marching-cubes mesh of an
analytic sphere SDF, meshed by the sparse route at resolution 512 (the tiles hold far more triangles than pixels) and at resolution 64
(far fewer), and -- with --validate-image -- of Runner.validate_image of one 800 x 800 view with the bench's full-size networks: the
volumetric way to see the same kind of surface.  1 warm-up + 5 repetitions by a host clock around a device synchronise (rasterize
reads the host once, so its host time belongs to the figure); the entry points' own device times by _C.KernelClock in a separate
repetition.  Reported, not gated.

    python scripts/probe_mesh_raster.py [out.json]                       -> profiles/mesh_raster.json unless told otherwise
    python scripts/probe_mesh_raster.py --validate-image [out.json]      (uses nothing this rasteriser added: runs on any commit)"""
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
REPS = 5
SIDE = 800
ANGLE_X = 0.6911                  # the field of view of the NeRF-synthetic cameras


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 3)


def repeat(fn):
    ms = [wall(fn)[1] for _ in range(1 + REPS)][1:]
    return {'wall_ms': ms, 'median_ms': sorted(ms)[len(ms) // 2]}


def camera_rays(dev, dist=2.6):
    """the rays of a NeRF-synthetic style camera at (0, 0, dist) looking at the origin, as nerfset.gen_rays_at shoots them"""
    import torch
    focal = 0.5 * SIDE / math.tan(0.5 * ANGLE_X)
    t = torch.linspace(0, SIDE - 1, SIDE, device=dev)
    py, px = torch.meshgrid(t, t, indexing='ij')
    d = torch.stack([(px - SIDE // 2) / focal, -(py - SIDE // 2) / focal, -torch.ones_like(py)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor([0.0, 0.0, dist], device=dev).expand(d.shape)
    return o, d


def raster_cases():
    import torch
    from probe_mesh_materials import RADIUS, sparse_sphere
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo import mesh_render
    dev = torch.device('cuda:0')
    rays_o, rays_d = camera_rays(dev)
    P = mesh_render.camera_from_rays(rays_o, rays_d)
    cases = {}
    for R in (512, 64):
        v, t, info = sparse_sphere(R, dev)
        r = mesh_render.rasterize(v, t, P, SIDE, SIDE)
        tile_count = _C.raster_count(v, t, P, SIDE, SIDE, 1e-3, 0)[1]
        _C.KernelClock.reset(True)
        mesh_render.rasterize(v, t, P, SIDE, SIDE)
        torch.cuda.synchronize()
        entries = {k: round(ms, 3) for k, (n, ms) in _C.KernelClock.summary().items()}
        _C.KernelClock.reset(False)
        cases[f'resolution_{R}'] = {
            'resolution': R, 'vertices': int(v.shape[0]), 'triangles': int(t.shape[0]), **info, 'stats': r['stats'],
            'covered_pixels': int((r['face'] >= 0).sum()), 'tiles': int(tile_count.numel()), 'tiles_in_use': int((tile_count > 0).sum()),
            'largest_tile_list': int(tile_count.max()), 'mean_list_of_tiles_in_use': round(float(tile_count[tile_count > 0].float().mean()), 1),
            'entry_device_ms': entries,
            'rasterize': repeat(lambda: mesh_render.rasterize(v, t, P, SIDE, SIDE)),
            'render': repeat(lambda: mesh_render.render(v, t, P, SIDE, SIDE)),
        }
    return {
        'what': f'geo/mesh_render.rasterize and render (face normals, no attributes) at {SIDE} x {SIDE} on one MI355X: a sphere of radius '
                f'{RADIUS} meshed by the sparse route, seen from distance 2.6 with the NeRF-synthetic field of view',
        'method': f'1 warm-up + {REPS} repetitions; a host clock around a device synchronise, the one host read of rasterize included; '
                  'entry_device_ms: HIP events around each entry point in one more repetition (_C.KernelClock); not gated',
        'cases': cases,
    }


def validate_image_case():
    import numpy as np
    import torch
    from PIL import Image
    import bench
    from vqnerf_release_amd.geo import conf as hocon
    from vqnerf_release_amd.geo.models.nerfset import Dataset
    from vqnerf_release_amd.geo.nerf_runner import Runner
    tmp = tempfile.mkdtemp(prefix='probe_mesh_raster_')
    view = os.path.join(tmp, 'scene', 'train_000')
    os.makedirs(view)
    rgba = np.full((SIDE, SIDE, 4), 255, np.uint8)
    Image.fromarray(rgba, 'RGBA').save(os.path.join(view, 'rgba.png'))
    pose = np.eye(4)
    pose[2, 3] = 4.0                                               # a camera on the +z axis looking down its own -z at the origin
    with open(os.path.join(tmp, 'scene', 'transforms_train.json'), 'w') as f:
        json.dump({'camera_angle_x': ANGLE_X, 'frames': [{'transform_matrix': pose.tolist()}]}, f)
    dataset = Dataset(hocon.parse_string('dataset { data_dir = %s/scene\n longint = false }' % tmp)['dataset'], device='cuda:0')
    torch.manual_seed(0)
    runner = Runner(conf_text=bench.full_conf_text().replace('/tmp/vqn_bench_exp', os.path.join(tmp, 'exp')), case='probe', dataset=dataset)
    run = lambda: runner.validate_image(idx=0, resolution_level=1)
    imgs = run()
    return {
        'what': f'Runner.validate_image of one {SIDE} x {SIDE} view with the full-size networks of bench.py (untrained: the geometric-init '
                'sphere), files written: the volumetric way to see the surface',
        'method': f'1 warm-up + {REPS} repetitions; a host clock around the call and a device synchronise; includes composing and writing '
                  'the four PNG files, as a user of the call pays them',
        'alpha_pixels': int((imgs['alpha'] > 0).sum()), 'rays': SIDE * SIDE,
        'n_samples_per_ray': runner.renderer.n_samples + runner.renderer.n_importance,
        **repeat(run),
    }


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    volumetric = '--validate-image' in sys.argv
    out = validate_image_case() if volumetric else raster_cases()
    path = args[0] if args else os.path.join(ROOT, 'profiles', 'mesh_raster.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out if volumetric else {k: {x: c[x] for x in ('triangles', 'largest_tile_list', 'entry_device_ms')} | {
        'rasterize_ms': c['rasterize']['median_ms'], 'render_ms': c['render']['median_ms']} for k, c in out['cases'].items()}))


if __name__ == '__main__':
    main()
