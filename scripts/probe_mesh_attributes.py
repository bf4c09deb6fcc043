"""Stage times of the mesh clean-up and attributes (geo/mesh.py: components, filter_components, vertex_normals, vertex_colors) on the
resolution-512 mesh of the full-size network, beside the stages profiles/mesh_export.json lists and the whole default
Runner.validate_mesh(resolution=512) call of the same run.  1 warm-up + 3 repetitions each, stages by HIP events on the launch stream,
whole calls by a host clock around a device synchronise.  Reported, not gated.

    python scripts/probe_mesh_attributes.py [resolution [out.json]]      -> profiles/mesh_attributes.json unless told otherwise"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 3


def main():
    import torch
    import bench
    from vqnerf_release_amd.geo import mesh
    from vqnerf_release_amd.geo.nerf_runner import Runner, SyntheticDataset
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp()
    text = bench.full_conf_text(2560).replace('/tmp/vqn_bench_exp', tmp)
    r = Runner(conf_text=text, case='mesh_attr', dataset=SyntheticDataset(device=dev, n_images=8), device=dev)
    sdf, col = r.renderer.sdf_network, r.renderer.color_network
    bmin = torch.tensor(r.dataset.object_bbox_min, dtype=torch.float32)
    bmax = torch.tensor(r.dataset.object_bbox_max, dtype=torch.float32)

    def stage(fn):
        out, ms = None, []
        for i in range(1 + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms.append(round(e0.elapsed_time(e1), 3))
        return out, ms

    def wall(fn):
        ms = []
        for i in range(1 + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i:
                ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        return ms

    stages = {}
    u, stages['field_ms'] = stage(lambda: mesh.extract_fields_device(bmin, bmax, R, sdf))
    b_min, b_max = bmin.numpy().astype('float64'), bmax.numpy().astype('float64')
    (v, t), stages['marching_cubes_ms'] = stage(lambda: mesh.marching_cubes(u, 0.0, origin=b_min, step=(b_max - b_min) / (R - 1.0)))
    del u
    labels, stages['components_ms'] = stage(lambda: mesh.components(t, v.shape[0]))
    (fv, ft, info), stages['filter_components_keep_largest_1_ms'] = stage(lambda: mesh.filter_components(v, t, keep_largest=1))
    _, stages['vertex_normals_ms'] = stage(lambda: mesh.vertex_normals(fv, sdf))
    _, stages['vertex_colors_ms'] = stage(lambda: mesh.vertex_colors(fv, sdf, col))
    whole = {'validate_mesh_default_wall_ms': wall(lambda: r.validate_mesh(resolution=R)),
             'validate_mesh_keep_largest_1_normals_colors_wall_ms':
                 wall(lambda: r.validate_mesh(resolution=R, keep_largest=1, normals=True, colors=True))}
    med = lambda a: sorted(a)[len(a) // 2]
    out = {
        'what': 'mesh clean-up and attributes on one MI355X: stage times of geo/mesh.py on the mesh of the full-size network (bench.py '
                'full_conf_text: 8 x 256 SDF network), object box of the synthetic dataset, next to the default validate_mesh call (the '
                "parent commit's code path, byte-identical output) in the same run",
        'method': f'1 warm-up + {REPS} repetitions; stages by HIP events on the launch stream (filter_components includes its one host '
                  'read), whole calls by a host clock around a device synchronise; not gated',
        'resolution': R, 'vertices': int(v.shape[0]), 'triangles': int(t.shape[0]),
        'components': int(torch.unique(labels).numel()), 'filter_info': info,
        'vertices_kept': int(fv.shape[0]), 'triangles_kept': int(ft.shape[0]),
        'stages_ms': stages, 'whole_ms': whole,
        'median': {k: med(a) for k, a in list(stages.items()) + list(whole.items())},
    }
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'mesh_attributes.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out['median']))
    print(json.dumps({k: out[k] for k in ('resolution', 'vertices', 'triangles', 'components', 'filter_info', 'vertices_kept', 'triangles_kept')}))


if __name__ == '__main__':
    main()
