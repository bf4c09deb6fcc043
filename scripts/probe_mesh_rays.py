"""Times of the mesh ray caster (geo/mesh_rays.py; csrc/mesh_rays.hip) on the sparse-route sphere of scripts/probe_mesh_raster.py at
resolutions 64 and 512: the grid build and its (triangle, cell) pairs, `cast` of the 800 x 800 camera rays beside `rasterize` of the
same view, and `light_visibility` of the view's foreground points x the 512 lights of the 16 x 32 light map for both lane mappings,
in rays per second over the front-lit pairs (the rays the volumetric route marches).  Beside them the yardstick: GeoExtractor.
compute_vis in bench.py's 4,096-point configuration with the bench's full-size networks -- code this caster does not touch, so the
figure is the parent commit's -- and, on the mesh of that same untrained network, how many (point, light) pairs the two routes agree
on.  1 warm-up + 5 repetitions, median and range; device times by HIP events on the stream apart from whole calls by a host clock
around a device synchronise.  Reported, not gated.

    python scripts/probe_mesh_rays.py [out.json]                         -> profiles/mesh_rays.json unless told otherwise
    python scripts/probe_mesh_rays.py --no-volumetric [out.json]         (the mesh side only)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
REPS = 5
SIDE = 800


def timed(fn):
    """1 warm-up + REPS repetitions -> (last result, {device_ms by HIP events, wall_ms by a host clock around a synchronise})"""
    import torch
    dev_ms, wall_ms, out = [], [], None
    for rep in range(1 + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            dev_ms.append(round(e0.elapsed_time(e1), 3))
            wall_ms.append(round(wall, 3))
    stat = lambda ms: {'median_ms': sorted(ms)[len(ms) // 2], 'min_ms': min(ms), 'max_ms': max(ms), 'all_ms': ms}
    return out, {'device': stat(dev_ms), 'wall': stat(wall_ms)}


def lights_512(dev):
    import torch
    from vqnerf_release_amd.decomp.brdf.renderer import gen_light_xyz
    return torch.tensor(gen_light_xyz(16, 32)[0].reshape(-1, 3), dtype=torch.float32, device=dev)


def front_lit(points, normals, lights):
    import torch
    n = 0
    for s in range(0, points.shape[0], 8192):
        d = torch.nn.functional.normalize(lights[None] - points[s:s + 8192, None, :], dim=-1)
        n += int((torch.einsum('ijk,ik->ij', d, normals[s:s + 8192]) > 0).sum())
    return n


def mesh_cases(dev):
    import torch
    from probe_mesh_materials import RADIUS, sparse_sphere
    from probe_mesh_raster import camera_rays
    from vqnerf_release_amd.geo import mesh_render
    from vqnerf_release_amd.geo.mesh_rays import MeshRays
    rays_o, rays_d = camera_rays(dev)
    P = mesh_render.camera_from_rays(rays_o, rays_d)
    o, d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    lights = lights_512(dev)
    cases = {}
    for R in (64, 512):
        v, t, _ = sparse_sphere(R, dev)
        m, build = timed(lambda: MeshRays(v, t))
        counts = torch.cat([m.cell_offset[1:].long(), torch.tensor([m.n_pairs], device=dev)]) - m.cell_offset
        hit, cast = timed(lambda: m.cast(o, d))
        raster, rast = timed(lambda: mesh_render.rasterize(v, t, P, SIDE, SIDE))
        fg = hit['face'] >= 0
        same = int((fg.reshape(SIDE, SIDE) == (raster['face'] >= 0)).sum())
        points = (o + hit['t'][:, None] * d)[fg].contiguous()
        normals = torch.nn.functional.normalize(points, dim=-1)                # the sphere's own normals
        n_front = front_lit(points, normals, lights)
        case = {'resolution': R, 'vertices': int(v.shape[0]), 'triangles': int(t.shape[0]), 'grid_dims': list(m.grid.dims),
                'cell': m.cell, 'cells': int(m.grid.cells), 'cells_in_use': int((counts > 0).sum()),
                'n_pairs': m.n_pairs, 'largest_cell_list': int(counts.max()), 'stats': m.stats, 'build': build,
                'cast_800x800': dict(cast, rays=SIDE * SIDE, hits=int(fg.sum()), pixels_equal_to_rasterize=same,
                                     rays_per_s=round(SIDE * SIDE / (cast['device']['median_ms'] * 1e-3))),
                'rasterize_800x800': rast, 'light_visibility': {'points': int(points.shape[0]), 'lights': 512, 'front_lit_pairs': n_front,
                                                                'bias': m.default_bias()}}
        outs = {}
        for lanes in ('points', 'lights'):
            outs[lanes], tm = timed(lambda: m.light_visibility(points, normals, lights, lanes=lanes))
            ms = tm['device']['median_ms']
            case['light_visibility'][lanes] = dict(tm, front_lit_rays_per_s=round(n_front / (ms * 1e-3)),
                                                   pairs_per_s=round(points.shape[0] * 512 / (ms * 1e-3)))
        case['light_visibility']['mappings_equal'] = bool(torch.equal(outs['points'], outs['lights']))
        case['light_visibility']['visible_pairs'] = int(outs['points'].sum())
        cases[f'resolution_{R}'] = case
    return {'sphere_radius': RADIUS, 'cases': cases}


def volumetric_case(dev):
    """bench.py's compute_vis leg, and the agreement of the two routes on the mesh of the same network"""
    import torch
    import bench
    from vqnerf_release_amd.geo.gen_geo import GeoExtractor
    from vqnerf_release_amd.geo.mesh_rays import MeshRays
    from vqnerf_release_amd.geo.models.fields import RenderingNetwork, SDFNetwork, SingleVarianceNetwork
    from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
    torch.manual_seed(0)
    sdf, col, var = SDFNetwork(**bench.FULL['sdf']).to(dev), RenderingNetwork(**bench.FULL['color']).to(dev), SingleVarianceNetwork(0.3).to(dev)
    ren = NeuSRenderer(None, sdf, var, col, **bench.FULL['renderer'])
    ex = GeoExtractor(ren, max_radius=2.0, light_h=16, max_rays=1 << 20)
    npts = 4096
    u = torch.randn(npts, 3, device=dev)
    nrm = u / u.norm(dim=-1, keepdim=True)
    msk = torch.ones(npts, 1, device=dev)
    surf = 0.5 * nrm                                            # bench.py's points
    n_sec = front_lit(surf, nrm, ex.lxyz[0].to(dev))
    _, tm = timed(lambda: ex.compute_vis(surf, nrm, msk, perturb_overwrite=0))
    out = {'compute_vis_bench_configuration': dict(tm, surface_points=npts, secondary_rays=n_sec,
                                                   secondary_rays_per_s=round(n_sec / (tm['wall']['median_ms'] * 1e-3)),
                                                   note='whole call by the host clock, as bench.py reports it; f32 kernels')}
    # the two routes on the same points: the network's own surface, by its mesh
    lo, hi = torch.full((3,), -1.0, device=dev), torch.full((3,), 1.0, device=dev)
    v, t = ren.extract_geometry_device(lo, hi, 256, 0.0, sparse=True)
    m = MeshRays(v, t)
    pick = torch.randperm(v.shape[0], device=dev)[:npts]
    pts = v[pick].contiguous()
    g = sdf.gradient(pts).reshape(-1, 3).detach()
    nr = torch.nn.functional.normalize(g, dim=-1)
    vol = ex.compute_vis(pts, nr, msk, perturb_overwrite=0)
    msh = ex.compute_vis_mesh(pts, nr, msk, m)
    front = torch.einsum('ijk,ik->ij', torch.nn.functional.normalize(ex.lxyz.to(dev) - pts[:, None, :], dim=-1), nr) > 0
    agree = ((vol > 0.5) == (msh > 0.5))
    out['agreement_on_the_untrained_network'] = {
        'mesh_resolution': 256, 'triangles': int(t.shape[0]), 'points': npts, 'pairs': int(agree.numel()), 'pairs_agreeing': int(agree.sum()),
        'front_lit_pairs': int(front.sum()), 'front_lit_pairs_agreeing': int((agree & front).sum()), 'bias': m.default_bias(),
        'volumetric_visible': int((vol > 0.5).sum()), 'mesh_visible': int((msh > 0.5).sum()),
        'note': 'an untrained geometric-init sphere casts no shadow on itself: this agreement says little beyond front / back lighting'}
    return out


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    dev = torch.device('cuda:0')
    out = {'what': 'geo/mesh_rays.MeshRays on one MI355X: grid build, cast of 800 x 800 camera rays, light visibility of the view\'s '
                   'foreground points x 512 lights, on a sphere meshed by the sparse route; beside GeoExtractor.compute_vis (volumetric)',
           'method': f'1 warm-up + {REPS} repetitions, median and range; device: HIP events around the call on its stream; wall: a host '
                     'clock around the call and a device synchronise (the build reads the host once); not gated'}
    out.update(mesh_cases(dev))
    if '--no-volumetric' not in sys.argv:
        out['volumetric'] = volumetric_case(dev)
    path = args[0] if args else os.path.join(ROOT, 'profiles', 'mesh_rays.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    brief = {k: {'n_pairs': c['n_pairs'], 'build_ms': c['build']['wall']['median_ms'], 'cast_ms': c['cast_800x800']['device']['median_ms'],
                 'rasterize_ms': c['rasterize_800x800']['wall']['median_ms'],
                 'lvis_rays_per_s': {l: c['light_visibility'][l]['front_lit_rays_per_s'] for l in ('points', 'lights')}}
             for k, c in out['cases'].items()}
    if 'volumetric' in out:
        brief['compute_vis_rays_per_s'] = out['volumetric']['compute_vis_bench_configuration']['secondary_rays_per_s']
        a = out['volumetric']['agreement_on_the_untrained_network']
        brief['agreement'] = [a['pairs_agreeing'], a['pairs']]
    print(json.dumps(brief))


if __name__ == '__main__':
    main()
