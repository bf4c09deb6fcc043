"""Stage times of the sparse mesh export (geo/mesh.py extract_geometry_sparse) on the full-size network, object box of the synthetic
dataset, as profiles/mesh_export.json: at resolution 512 beside the dense route of the same run, with the two meshes compared; at
1024 and 2048, which the dense route cannot do or cannot afford, alone.  1 warm-up + 3 repetitions, stages by HIP events on the launch
stream (the stage marks of extract_geometry_sparse; a stage that ends in a host read includes it), the kernels' own times from
_C.KernelClock.  Reported, not gated.

    python scripts/probe_mesh_sparse.py [out.json [resolution ...]]      -> profiles/mesh_sparse.json unless told otherwise"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 3


def main():
    import torch
    import bench
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo import mesh
    from vqnerf_release_amd.geo.nerf_runner import Runner, SyntheticDataset
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'mesh_sparse.json')
    resolutions = [int(a) for a in sys.argv[2:]] or [512, 1024, 2048]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    text = bench.full_conf_text(2560).replace('/tmp/vqn_bench_exp', tempfile.mkdtemp())
    r = Runner(conf_text=text, case='mesh_sparse', dataset=SyntheticDataset(device=dev, n_images=8), device=dev)
    sdf = r.renderer.sdf_network
    bmin = torch.tensor(r.dataset.object_bbox_min, dtype=torch.float32)
    bmax = torch.tensor(r.dataset.object_bbox_max, dtype=torch.float32)
    med = lambda a: sorted(a)[len(a) // 2]
    out = {
        'what': 'sparse mesh export on one MI355X: stage times of geo/mesh.py extract_geometry_sparse on the full-size network (bench.py '
                'full_conf_text: 8 x 256 SDF network), object box of the synthetic dataset, lipschitz = 2.0; at 512 beside the dense '
                'route (extract_geometry_device) in the same run',
        'method': f'1 warm-up + {REPS} repetitions; stages by HIP events on the launch stream: centres = the network at the brick centres, '
                  'the selection and its host read; brick_list = the list and the allocation; brick_field = point generation + the '
                  'network on the active bricks; classify; sort_and_sums = the key sort, both prefix sums and the host read; emit.  '
                  'kernel_ms: per C-ABI entry, all its launches of one call, from the last repetition.  Not gated',
        'box': [bmin.tolist(), bmax.tolist()], 'runs': {},
    }

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)

    for R in resolutions:
        run = {}
        stages, whole, kernels, res = {}, [], {}, None
        for i in range(1 + REPS):
            marks = []
            _C.KernelClock.reset(True)
            res = mesh.extract_geometry_sparse(bmin, bmax, R, 0.0, sdf, marks=marks)
            torch.cuda.synchronize()
            kernels = {k: round(v[1], 3) for k, v in _C.KernelClock.summary().items()}
            _C.KernelClock.reset(False)
            if i:
                for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                    stages.setdefault(name + '_ms', []).append(round(e0.elapsed_time(e1), 3))
                whole.append(round(marks[0][1].elapsed_time(marks[-1][1]), 3))
        v, t, info = res
        run['sparse'] = {'info': info, 'vertices': int(v.shape[0]), 'triangles': int(t.shape[0]), 'stages_ms': stages, 'whole_ms': whole,
                         'kernel_ms': kernels, 'median': dict({k: med(a) for k, a in stages.items()}, whole_ms=med(whole))}
        print(R, json.dumps(run['sparse']['median']), json.dumps(info), flush=True)
        if R <= 512:
            ms, dres = [], None
            for i in range(1 + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dres = mesh.extract_geometry_device(bmin, bmax, R, 0.0, sdf)
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(round(e0.elapsed_time(e1), 3))
            equal = bool(torch.equal(dres[1], t) and torch.equal(dres[0].view(torch.int32), v.view(torch.int32)))
            run['dense'] = {'whole_ms': ms, 'median_whole_ms': med(ms), 'points_evaluated': R ** 3}
            run['meshes_equal'] = equal
            print(R, 'dense', med(ms), 'equal', equal, flush=True)
            del dres
        del res, v, t
        out['runs'][str(R)] = run
        flush()                                  # after every resolution: a run that is cut short keeps what it has


if __name__ == '__main__':
    main()
