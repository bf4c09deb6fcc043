"""Times of the mesh-material kernels (geo/mesh.py: smooth_labels, split_by_label; csrc/mesh_materials.hip) on an export-sized mesh --
a sphere meshed by the sparse route at a resolution that gives about 3 * 10^6 triangles -- at K = 16 and K = 128, beside the torch
statement of the same split on the same device: a stable argsort of the face codes plus torch.unique over the (code, vertex) keys.
Both results are compared before anything is timed.  1 warm-up + 5 repetitions, the two versions alternating, by a host clock around a
device synchronise (both versions read the host, so their host time belongs to the figure).  Host reads are counted by torch's
synchronisation warnings (torch.cuda.set_sync_debug_mode), entry-point calls by _C.KernelClock.  Reported, not gated.

    python scripts/probe_mesh_materials.py [resolution [out.json]]      -> profiles/mesh_materials.json unless told otherwise"""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 5
RADIUS = 0.8
# kernel launches inside each entry point (csrc/mesh_materials.hip), beside the hipMemsetAsync nodes named in the second place
KERNELS = {'vqn_mesh_label_mode': ('5 + iters', 2), 'vqn_mesh_split_count': (2, 1), 'vqn_mesh_split_emit': (2, 0)}


def sparse_sphere(R, dev):
    """the sphere |x| = RADIUS on the R^3 grid over [-1, 1]^3 through the bricks its surface passes through -> (vertices, triangles, info)"""
    import torch
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo import mesh
    axes_host = [torch.linspace(-1.0, 1.0, R) for _ in range(3)]
    plan = mesh.plan_bricks(R, mesh.BRICK, axes=[a.numpy() for a in axes_host])
    axes = [a.to(dev) for a in axes_host]
    c = [axes[a][torch.from_numpy(plan.centre[a]).to(dev)] for a in range(3)]
    dist = torch.sqrt(c[0][:, None, None] ** 2 + c[1][None, :, None] ** 2 + c[2][None, None, :] ** 2)
    active = (dist - RADIUS).abs() <= torch.from_numpy(plan.h).to(dev)           # |x| is 1-Lipschitz
    brick_ijk = torch.nonzero(active).to(torch.int32).contiguous()               # (sorted by linear index)
    n = brick_ijk.shape[0]
    ub = torch.empty((n * _C.BRICK_POINTS,), dtype=torch.float32, device=dev)
    for s in range(0, n * _C.BRICK_POINTS, mesh.FIELD_SLAB):
        pts = _C.mc_brick_points(axes, plan.dims, brick_ijk, s, min(mesh.FIELD_SLAB, n * _C.BRICK_POINTS - s))
        ub[s: s + pts.shape[0]] = RADIUS - pts.norm(dim=-1)
    step = 2.0 / (R - 1.0)
    v, t, leaks = mesh.marching_cubes_bricks(ub.reshape(n, 9, 9, 9), brick_ijk, plan.dims, 0.0, origin=(-1.0, -1.0, -1.0), step=(step,) * 3)
    assert leaks == 0
    return v, t, dict(bricks_total=int(active.numel()), bricks_active=n)


def material_like_codes(v, K, seed):
    """codes with borders and speckle: the nearest of K random directions, 5 % of the vertices re-drawn at random"""
    import torch
    g = torch.Generator(device=v.device).manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn((K, 3), device=v.device, generator=g), dim=-1)
    codes = (v @ dirs.t()).argmax(-1)
    noise = torch.rand((v.shape[0],), device=v.device, generator=g) < 0.05
    return torch.where(noise, torch.randint(0, K, (v.shape[0],), device=v.device, generator=g), codes).to(torch.int32)


def torch_split(tris, codes, K):
    """the torch statement of split_by_label: face codes, a stable argsort, torch.unique over the (code, vertex) keys"""
    import torch
    V = codes.shape[0]
    c = codes[tris.long()]
    a, b, d = c[:, 0], c[:, 1], c[:, 2]
    fc = torch.where((a == b) | (a == d), a, torch.where(b == d, b, torch.minimum(a, torch.minimum(b, d))))
    face_src = torch.argsort(fc, stable=True)
    fcs = fc[face_src].long()
    keys = fcs[:, None] * V + tris[face_src].long()
    uniq, inv = torch.unique(keys.reshape(-1), return_inverse=True)              # sorted: by (code, vertex); reads the host for its size
    first = torch.searchsorted(uniq, torch.arange(K + 1, device=tris.device) * V)
    tris_local = inv.reshape(-1, 3) - first[fcs][:, None]
    face_count = torch.bincount(fc.long(), minlength=K)
    offsets = torch.cat([torch.cumsum(face_count, 0), first]).tolist()           # the read a caller needs to slice the groups
    return dict(face_src=face_src.to(torch.int32), vert_src=(uniq % V).to(torch.int32), tris_local=tris_local.to(torch.int32),
                face_offset=[0] + offsets[:K], vert_offset=offsets[K:])


def main():
    import torch
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo import mesh
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 832
    dev = torch.device('cuda:0')
    v, t, info = sparse_sphere(R, dev)
    V, T = v.shape[0], t.shape[0]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, round((time.perf_counter() - t0) * 1e3, 3)

    def host_reads(fn):
        torch.cuda.set_sync_debug_mode(1)
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter('always')
                fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        return len(w)

    med = lambda a: sorted(a)[len(a) // 2]
    cases = {}
    for K in (16, 128):
        codes = material_like_codes(v, K, seed=K)
        ours_smooth = lambda: mesh.smooth_labels(t, codes, K, iters=2)
        lab, changed = ours_smooth()
        ours_split = lambda: mesh.split_by_label(t, lab, K)
        theirs_split = lambda: torch_split(t, lab, K)
        a, b = ours_split(), theirs_split()
        same = all(torch.equal(a[k], b[k]) for k in ('face_src', 'vert_src', 'tris_local')) and a['face_offset'] == b['face_offset'] \
            and a['vert_offset'] == b['vert_offset']
        _C.KernelClock.reset(True)
        ours_smooth(), ours_split()
        torch.cuda.synchronize()
        entries = {k: n[0] for k, n in _C.KernelClock.summary().items()}
        _C.KernelClock.reset(False)
        reads = {'smooth_labels': host_reads(ours_smooth), 'split_by_label': host_reads(ours_split), 'torch_split': host_reads(theirs_split)}
        ms = {'smooth_labels_iters2': [], 'split_by_label': [], 'torch_split': []}
        for i in range(1 + REPS):
            for name, fn in (('smooth_labels_iters2', ours_smooth), ('split_by_label', ours_split), ('torch_split', theirs_split)):
                _, dt = wall(fn)
                if i:
                    ms[name].append(dt)
        m = {k: med(x) for k, x in ms.items()}
        cases[f'K{K}'] = {
            'codes': K, 'changed': changed.tolist(), 'faces_kept': a['n_faces'], 'vertex_slots': a['n_slots'],
            'groups_used': sum(1 for c in a['face_count'] if c), 'equal_to_the_torch_statement': bool(same),
            'entry_calls': entries, 'host_reads_counted': reads, 'wall_ms': ms, 'median_ms': m,
            'median_ms_smooth_plus_split': round(m['smooth_labels_iters2'] + m['split_by_label'], 3),
            'torch_split_over_split_by_label': round(m['torch_split'] / m['split_by_label'], 2),
        }
    out = {
        'what': 'mesh-material kernels on one MI355X: smooth_labels(iters=2) and split_by_label of geo/mesh.py on a sphere meshed by the '
                'sparse route, beside the torch statement of the split (stable argsort of the face codes + torch.unique over the '
                '(code, vertex) keys + searchsorted) on the same device and the same smoothed codes; the torch statement has no '
                'counterpart of the label clean-up',
        'method': f'1 warm-up + {REPS} repetitions, the versions alternating; a host clock around a device synchronise (each version '
                  'includes its host reads); host reads counted by torch.cuda.set_sync_debug_mode warnings; entry calls by '
                  '_C.KernelClock; not gated',
        'resolution': R, 'vertices': V, 'triangles': T, **info,
        'kernel_launches_per_entry_and_memset_nodes': KERNELS,
        'torch_glue_of_split_by_label': 'two cumsum, two strided gathers, one cat, one host copy, two subtractions',
        'cases': cases,
    }
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'mesh_materials.json')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ('resolution', 'vertices', 'triangles', 'bricks_active')}))
    for k, c in cases.items():
        print(k, json.dumps({x: c[x] for x in ('median_ms', 'host_reads_counted', 'entry_calls', 'equal_to_the_torch_statement', 'changed')}))


if __name__ == '__main__':
    main()
