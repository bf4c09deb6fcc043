"""GPU: the mesh-material kernels (csrc/mesh_materials.hip: vqn_mesh_label_mode, vqn_mesh_split_count / _emit) against the plain
statement of tests/mesh_materials_model.py -- every integer output exactly equal -- at the sizes where they can go wrong (bitmap
word and wave boundaries, a prefix sum over more than one workgroup, more than one face block, a fan hub of high valence), their
caller-error and refusal paths with guard bands around every output, and the layers above them: Model.materials_at of vq_nfr and
ref_nfr against vis_mat / fast_embed bit for bit, and decomp/material_mesh.run end to end on a marching-cubes sphere."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_materials_model as mm
from tests.gpu_util import launches
from vqnerf_release_amd import _C
from vqnerf_release_amd.geo import mesh

pytestmark = pytest.mark.gpu
GUARD = 64
ENTRIES = ('vqn_mesh_label_mode', 'vqn_mesh_split_count', 'vqn_mesh_split_emit')


def _dev(a, dtype=torch.int32):
    return torch.tensor(np.asarray(a), dtype=dtype, device='cuda')


def _random_mesh(V, seed):
    """an indexed triangle list over V vertices, about 2 V triangles: random triples (degenerate ones among them at small V)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, V, (max(2 * V + 3, 4), 3)).astype(np.int32)


_sphere_cache = {}


def _sphere():
    """a device marching-cubes sphere of radius 0.75 on a 12^3 grid over [-1, 1]^3 -> (vertices, triangles) on the device"""
    if not _sphere_cache:
        g = torch.linspace(-1.0, 1.0, 12, device='cuda')
        x, y, z = torch.meshgrid(g, g, g, indexing='ij')
        u = (0.75 - torch.sqrt(x * x + y * y + z * z)).contiguous()
        step = 2.0 / 11.0
        _sphere_cache['m'] = mesh.marching_cubes(u, 0.0, origin=(-1.0, -1.0, -1.0), step=(step, step, step))
    return _sphere_cache['m']


def _check_split(tris, codes, K, got):
    """mesh.split_by_label's dict against the model, and its invariants on their own"""
    want = mm.split(tris, codes, K)
    for k in ('face_code', 'face_src', 'vert_src', 'tris_local'):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    for k in ('face_offset', 'vert_offset', 'face_count', 'vert_count', 'n_faces', 'n_slots', 'dropped'):
        assert got[k] == want[k], k
    # the invariants, without the model
    fc, fs = got['face_code'].cpu().numpy(), got['face_src'].cpu().numpy()
    vs, tl = got['vert_src'].cpu().numpy(), got['tris_local'].cpu().numpy()
    assert sorted(fs.tolist()) == np.flatnonzero(fc >= 0).tolist()                         # a permutation of the kept faces
    for k in range(K):
        f0, f1, v0, v1 = got['face_offset'][k], got['face_offset'][k + 1], got['vert_offset'][k], got['vert_offset'][k + 1]
        assert (np.diff(vs[v0:v1]) > 0).all()                                              # strictly ascending
        assert (fc[fs[f0:f1]] == k).all() and (np.diff(fs[f0:f1]) > 0).all()                # by (code, original index)
        assert np.array_equal(vs[v0 + tl[f0:f1]], np.asarray(tris)[fs[f0:f1]])
    return want


@pytest.mark.parametrize('K', [1, 2, 64, 65, 128])
@pytest.mark.parametrize('V', [1, 31, 32, 33, 63, 64, 65, 5000])
def test_labels_and_split_equal_the_model(V, K):
    tris = _random_mesh(V, seed=V)
    codes = np.random.default_rng(1000 * K + V).integers(0, K, V).astype(np.int32)
    with launches() as rec:
        lab, changed = mesh.smooth_labels(_dev(tris), _dev(codes), K, iters=2, self_weight=1)
        got = mesh.split_by_label(_dev(tris), lab, K)
    assert all(rec.counts[e] == 1 for e in ENTRIES), rec.counts
    want_lab, want_changed = mm.label_mode(tris, codes, K, self_weight=1, iters=2)
    assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), want_lab)
    assert changed.dtype == torch.int32 and np.array_equal(changed.cpu().numpy(), want_changed)
    _check_split(tris, want_lab, K, got)
    assert np.array_equal(mesh.face_labels(_dev(tris), lab, K).cpu().numpy(), mm.face_codes(tris, want_lab, K))
    if V == 5000:                                                                          # again: the same bits from run to run
        lab2, changed2 = mesh.smooth_labels(_dev(tris), _dev(codes), K, iters=2, self_weight=1)
        again = mesh.split_by_label(_dev(tris), lab2, K)
        assert torch.equal(lab, lab2) and torch.equal(changed, changed2)
        assert all(torch.equal(got[k], again[k]) for k in ('face_src', 'vert_src', 'tris_local'))


@pytest.mark.parametrize('iters,self_weight', [(1, 0), (1, 1), (3, 2), (4, 1)])
def test_sphere_with_random_codes(iters, self_weight):
    v, t = _sphere()
    V, K = v.shape[0], 7
    assert V > 100 and t.shape[0] > V
    codes = np.random.default_rng(iters).integers(0, K, V).astype(np.int32)
    lab, changed = mesh.smooth_labels(t, _dev(codes), K, iters=iters, self_weight=self_weight)
    want, want_changed = mm.label_mode(t.cpu().numpy(), codes, K, self_weight=self_weight, iters=iters)
    assert np.array_equal(lab.cpu().numpy(), want) and np.array_equal(changed.cpu().numpy(), want_changed) and want_changed[0] > 0
    _check_split(t.cpu().numpy(), want, K, mesh.split_by_label(t, lab, K))


def test_speckle_on_two_hemispheres_falls():
    v, t = _sphere()
    V, K = v.shape[0], 4
    rng = np.random.default_rng(9)
    clean = (v[:, 2] > 0).cpu().numpy().astype(np.int32)
    codes = clean.copy()
    speck = rng.choice(V, V // 20, replace=False)                                          # 5 % of the vertices
    codes[speck] = rng.integers(2, 4, len(speck))
    lab, changed = mesh.smooth_labels(t, _dev(codes), K, iters=3)
    want, want_changed = mm.label_mode(t.cpu().numpy(), codes, K, self_weight=1, iters=3)
    assert np.array_equal(lab.cpu().numpy(), want) and np.array_equal(changed.cpu().numpy(), want_changed)
    before, after = int((codes != clean).sum()), int((want != clean).sum())
    assert before == V // 20 and after < before, (before, after)
    s = mesh.split_by_label(t, lab, K)
    _check_split(t.cpu().numpy(), want, K, s)
    assert s['dropped'] == 0 and s['n_faces'] == t.shape[0] and s['n_slots'] > V              # the vertices on the border are in two groups


def test_fan_hub_of_300_triangles():
    n = 300
    tris = np.array([(0, i, i + 1) for i in range(1, n + 1)], np.int32)
    V, K = n + 2, 5
    rng = np.random.default_rng(4)
    for hub, weight, hub_stays in ((4, 1, False), (4, 700, True), (0, 0, None)):
        codes = rng.integers(0, 4, V).astype(np.int32)
        codes[0] = hub
        lab, changed = mesh.smooth_labels(_dev(tris), _dev(codes), K, iters=2, self_weight=weight)
        want, want_changed = mm.label_mode(tris, codes, K, self_weight=weight, iters=2)
        assert np.array_equal(lab.cpu().numpy(), want) and np.array_equal(changed.cpu().numpy(), want_changed)
        # one round: 600 votes move the hub unless its own weight outweighs them (in the second the rim, which heard the hub twice per
        # vertex, votes it back)
        first = mm.label_mode(tris, codes, K, self_weight=weight, iters=1)[0]
        assert hub_stays is None or (first[0] == hub) == hub_stays
        _check_split(tris, want, K, mesh.split_by_label(_dev(tris), lab, K))


def test_no_triangles_and_all_codes_equal():
    empty = torch.empty((0, 3), dtype=torch.int32, device='cuda')
    codes = _dev([2, 0, 1, 2, 2])
    lab, changed = mesh.smooth_labels(empty, codes, 3, iters=2, self_weight=0)
    assert torch.equal(lab, codes) and lab is not codes and changed.tolist() == [0, 0]
    s = mesh.split_by_label(empty, codes, 3)
    assert s['n_faces'] == s['n_slots'] == s['dropped'] == 0 and s['face_offset'] == [0] * 4 and s['vert_offset'] == [0] * 4
    assert s['face_src'].shape == (0,) and s['tris_local'].shape == (0, 3) and s['vert_src'].shape == (0,) and s['face_code'].shape == (0,)
    # all codes equal: a fixed point, every entry of `changed` is 0
    v, t = _sphere()
    codes = torch.full((v.shape[0],), 5, dtype=torch.int32, device='cuda')
    for w in (0, 1):
        lab, changed = mesh.smooth_labels(t, codes, 6, iters=3, self_weight=w)
        assert torch.equal(lab, codes) and changed.tolist() == [0, 0, 0]
    s = mesh.split_by_label(t, codes, 6)
    assert s['face_count'] == [0] * 5 + [t.shape[0]] and s['vert_count'] == [0] * 5 + [v.shape[0]]
    assert torch.equal(s['face_src'], torch.arange(t.shape[0], dtype=torch.int32, device='cuda')) and torch.equal(s['tris_local'], t)


def test_zero_iterations_return_the_same_object_and_launch_nothing():
    v, t = _sphere()
    codes = torch.zeros((v.shape[0],), dtype=torch.int32, device='cuda')
    with launches() as rec:
        lab, changed = mesh.smooth_labels(t, codes, 4, iters=0)
    assert lab is codes and changed.shape == (0,) and not rec.names


def _guarded(n, fill):
    """-> (whole buffer, the view of n int32 entries between two guard bands)"""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=torch.int32, device='cuda')
    return whole, whole[GUARD: GUARD + n]


def test_indices_out_of_range_are_dropped_and_nothing_outside_is_written():
    v, t = _sphere()
    tris = t.cpu().numpy().copy()
    V, T, K = v.shape[0], tris.shape[0], 6
    tris[7, 1] = V                                                                         # one past the end
    tris[T - 3, 2] = -1
    codes = np.random.default_rng(2).integers(0, K, V).astype(np.int32)
    codes[11] = K                                                                          # and a code out of range: it casts no vote
    iters = 2
    B, W = _C.mesh_split_shape(T, V)
    sentinel = -77
    d_tris, d_codes = _dev(tris), _dev(codes)
    bufs = {name: _guarded(n, sentinel) for name, n in (('lab', V), ('changed', iters), ('face_code', T), ('block_count', K * B),
                                                        ('bitmap', K * W), ('word_count', K * W))}
    need = _C.lib().vqn_mesh_label_scratch_bytes(T, V)
    scratch = torch.empty((need,), dtype=torch.uint8, device='cuda')
    p = lambda name: bufs[name][1].data_ptr()
    _C._call('vqn_mesh_label_mode', d_tris.data_ptr(), T, d_codes.data_ptr(), V, K, 1, iters, p('lab'), p('changed'), scratch.data_ptr(), need)
    want_lab, want_changed = mm.label_mode(tris, codes, K, self_weight=1, iters=iters)
    assert np.array_equal(bufs['lab'][1].cpu().numpy(), want_lab) and np.array_equal(bufs['changed'][1].cpu().numpy(), want_changed)
    _C._call('vqn_mesh_split_count', d_tris.data_ptr(), T, p('lab'), V, K, p('face_code'), p('block_count'), p('bitmap'), p('word_count'))
    want = mm.split(tris, want_lab, K)
    assert want['dropped'] >= 2 and want['face_code'][7] == -1 and want['face_code'][T - 3] == -1
    assert np.array_equal(bufs['face_code'][1].cpu().numpy(), want['face_code'])
    binc, winc = torch.cumsum(bufs['block_count'][1], 0, dtype=torch.int32), torch.cumsum(bufs['word_count'][1], 0, dtype=torch.int32)
    F, S = int(binc[-1]), int(winc[-1])
    assert (F, S) == (want['n_faces'], want['n_slots'])
    for name, n in (('face_src', F), ('tris_local', 3 * F), ('vert_src', S)):
        bufs[name] = _guarded(n, sentinel)
    out = (bufs['face_src'][1], bufs['tris_local'][1].view(F, 3), bufs['vert_src'][1])
    _C.mesh_split_emit(d_tris, V, K, bufs['face_code'][1].contiguous(), binc - bufs['block_count'][1], bufs['bitmap'][1].contiguous(),
                       winc - bufs['word_count'][1], F, S, out=out)
    for k in ('face_src', 'vert_src'):
        assert np.array_equal(bufs[k][1].cpu().numpy(), want[k]), k
    assert np.array_equal(out[1].cpu().numpy(), want['tris_local'])
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        assert (whole[:GUARD] == sentinel).all() and (whole[GUARD + view.numel():] == sentinel).all(), name
    # through the Python layer: the same, and the dropped faces are counted
    got = mesh.split_by_label(d_tris, bufs['lab'][1].clone(), K)
    _check_split(tris, want_lab, K, got)
    assert got['dropped'] == want['dropped']


def test_refusals_raise():
    v, t = _sphere()
    codes = torch.zeros((v.shape[0],), dtype=torch.int32, device='cuda')
    T, V = t.shape[0], v.shape[0]
    for K in (0, 129):
        with pytest.raises(_C.VqnError, match='rc=-2'):
            mesh.smooth_labels(t, codes, K)
        with pytest.raises(_C.VqnError, match='rc=-2'):
            mesh.split_by_label(t, codes, K)
    with pytest.raises(_C.VqnError, match='rc=-1'):
        mesh.smooth_labels(t, codes, 4, self_weight=-1)
    with pytest.raises(_C.VqnError, match='rc=-1'):
        mesh.smooth_labels(t, codes, 4, iters=-1)
    with pytest.raises(_C.VqnError):
        mesh.smooth_labels(t.cpu(), codes, 4)                                              # host tensors: no CPU path
    # sizes no tensor can have, stated to the library directly (it refuses before it reads or launches anything)
    out = torch.full((4 * T + 64,), -5, dtype=torch.int32, device='cuda')
    before = out.clone()
    a = (out.data_ptr(),) * 4
    for n_tris, n_verts, K, rc in ((T, 1 << 31, 4, -2), ((1 << 31) // 3 + 1, V, 4, -2), (T, 1 << 29, 128, -2), (-1, V, 4, -1), (T, -1, 4, -1)):
        with pytest.raises(_C.VqnError, match=f'rc={rc}'):
            _C._call('vqn_mesh_split_count', t.data_ptr(), n_tris, codes.data_ptr(), n_verts, K, *a)
        with pytest.raises(_C.VqnError, match=f'rc={rc}'):
            _C._call('vqn_mesh_label_mode', t.data_ptr(), n_tris, codes.data_ptr(), n_verts, K, 1, 1, out.data_ptr(), out.data_ptr(),
                     out.data_ptr(), 1 << 40)
        if K == 4:                                                                         # (the scratch does not depend on the codes)
            assert _C.lib().vqn_mesh_label_scratch_bytes(n_tris, n_verts) == rc
    for null in range(4):
        args = [t.data_ptr(), T, codes.data_ptr(), V, 4, *a]
        args[(0, 2, 5, 6)[null]] = None
        with pytest.raises(_C.VqnError, match='rc=-1'):
            _C._call('vqn_mesh_split_count', *args)
    with pytest.raises(_C.VqnError, match='rc=-1'):                                        # a scratch that is too small
        _C._call('vqn_mesh_label_mode', t.data_ptr(), T, codes.data_ptr(), V, 4, 1, 1, out.data_ptr(), out.data_ptr(), out.data_ptr(), 16)
    with pytest.raises(_C.VqnError, match='rc=-1'):                                        # totals that contradict the sizes
        _C._call('vqn_mesh_split_emit', t.data_ptr(), T, V, 4, *a, T + 1, 3, *a[:3])
    torch.cuda.synchronize()
    assert torch.equal(out, before)


# ---- the layers: materials_at, material_mesh.run --------------------------------------------------------------------------------------
K_MODEL = 8


@pytest.fixture(scope='module')
def vq():
    from tests.test_gpu_material_edit import _with_hw, H, W
    from tests.test_gpu_vq_entrypoints import _build, _points
    od, pt, specs, model, gamma, lxyz, lareas = _build('nerf', K_MODEL)
    views = [_with_hw(_points(od, 'nerf', H * W, seed)[1]) for seed in (6, 7)]
    big = _points(od, 'nerf', 700, 8)[1]
    return model, views + [big]


@pytest.fixture(scope='module')
def ref(vq):
    from tests.test_gpu_decomp import _ref_setup
    model = _ref_setup('hw')[4]
    model.__dict__['_stage2'] = vq[0]                                                      # what load_stage2 attaches
    return model


@pytest.mark.parametrize('fused', [True, False])
def test_materials_at_equals_vis_mat_and_fast_embed(vq, ref, fused):
    model, views = vq
    front = model.fuse_front
    model.fuse_front = fused
    try:
        for batch in views:
            fg = batch[5][:, 0] > 0
            xyz = batch[7][fg].contiguous()
            with launches() as rec:
                got = model.materials_at(xyz)
            assert rec.ran('vqn_mlp_chain_vq_fwd') == fused, rec.counts
            with torch.no_grad():
                pred = model.vis_mat(batch, mode='test')[0]
                emb = model.fast_embed(batch, mode='test')[3]['embed']
            assert got['code'].dtype == torch.int32 and got['code'].shape == (xyz.shape[0],)
            assert torch.equal(pred['embed'][fg][:, 0].to(torch.int32), got['code'] + 1) and torch.equal(emb[fg], pred['embed'][fg])
            assert torch.equal(pred['albedo'][fg], (1 - got['ks']) * got['basecolor'])
            assert torch.equal(pred['spec'][fg], got['ks'] * got['basecolor']) and torch.equal(pred['rough'][fg], got['rough'])
            # the VQ branch: what `call` shows for the same points (the VQ heads on the straight-through row x + (q - x), which equals
            # the code q to an ulp: the rows of material_rows themselves are what the driver's branch='vq' writes)
            with torch.no_grad():
                shown = model.call(batch, mode='test')[0]
            for k in ('vq_albedo', 'vq_spec', 'vq_rough'):
                assert torch.equal(shown[k][fg], got[k]), k
            assert xyz.shape[0] < 100 or len(torch.unique(got['code'])) > 1
            # in slabs: the same bits
            model.materials_slab = 100
            try:
                slabbed = model.materials_at(xyz)
            finally:
                del model.materials_slab
            assert all(torch.equal(got[k], slabbed[k]) for k in got)
            # the stage-3 model stands for the stage-2 model it was loaded from
            other = ref.materials_at(xyz)
            assert all(torch.equal(got[k], other[k]) for k in got)
    finally:
        model.fuse_front = front
    with pytest.raises(_C.VqnError):
        model.materials_at(views[0][7].cpu())


def _ply_faces_as_points(path):
    v, t, _ = mesh.read_ply(path, device='cpu')
    return [tuple(map(tuple, tri)) for tri in v.numpy()[t.numpy().astype(np.int64)].tolist()]


@pytest.mark.parametrize('branch', ['vq', 'main'])
def test_material_mesh_run_on_the_sphere(vq, tmp_path, branch):
    from vqnerf_release_amd.decomp import material_mesh
    model, _ = vq
    K = K_MODEL
    v, t = _sphere()
    out = str(tmp_path / branch)
    logged = []
    rec = material_mesh.run(model, (v, t), out, smooth=2, self_weight=1, branch=branch, parts=True, log=logged.append)
    assert rec == json.load(open(os.path.join(out, 'material_mesh.json'))) and len(logged) == 1
    tris = t.cpu().numpy()
    at = model.materials_at(v)
    raw = at['code'].cpu().numpy()
    lab, changed = mesh.smooth_labels(t, at['code'], K, iters=2, self_weight=1)
    want_lab, want_changed = mm.label_mode(tris, raw, K, self_weight=1, iters=2)
    assert np.array_equal(lab.cpu().numpy(), want_lab) and len(np.unique(want_lab)) > 1
    want = mm.split(tris, want_lab, K)
    used = [k for k in range(K) if want['face_count'][k]]
    assert sorted(os.listdir(out)) == sorted(['material_mesh.ply', 'material_mesh.obj', 'material_mesh.mtl', 'material_mesh.json'] +
                                             ['code_%03d.ply' % k for k in used])
    # the PLY: the smoothed codes, and under 'vq' the rows of those codes bit for bit
    pv, pt, _, extra = mesh.read_ply(os.path.join(out, 'material_mesh.ply'), extra=['material', 'spec', 'rough', 'red', 'green', 'blue'])
    assert torch.equal(pv, v) and torch.equal(pt, t) and torch.equal(extra['material'], lab) and extra['material'].dtype == torch.int32
    rows = model.material_rows()
    rgb = torch.stack([extra[c] for c in ('red', 'green', 'blue')], -1)
    if branch == 'vq':
        picked = rows[lab.long()]
        assert torch.equal(extra['rough'], picked[:, 6]) and torch.equal(extra['spec'], picked[:, 3:6].max(-1)[0])
        assert torch.equal(rgb, material_mesh._u8(picked[:, 0:3]))
    else:
        assert torch.equal(extra['rough'], at['rough'][:, 0]) and torch.equal(extra['spec'], (at['ks'] * at['basecolor']).max(-1)[0])
        assert torch.equal(rgb, material_mesh._u8((1 - at['ks']) * at['basecolor']))
    # the OBJ: one usemtl block per used code, with that code's faces in face_src order; the MTL: the rows
    from tests.test_mesh_materials_model import _parse_mtl, _parse_obj
    obj = _parse_obj(os.path.join(out, 'material_mesh.obj'))
    assert obj['mtllib'] == 'material_mesh.mtl' and [g[0] for g in obj['groups']] == ['code_%03d' % k for k in used]
    assert np.array_equal(np.array(obj['v'], np.float32), v.cpu().numpy())
    for k, (_, faces) in zip(used, obj['groups']):
        assert len(faces) == want['face_count'][k]
        assert np.array_equal(np.array(faces)[:, :, 0] - 1, tris[want['face_src'][want['face_offset'][k]: want['face_offset'][k + 1]]])
    mtl = _parse_mtl(os.path.join(out, 'material_mesh.mtl'))
    rows_h = rows.cpu().numpy()
    assert list(mtl) == ['code_%03d' % k for k in range(K)]
    for k in range(K):
        m = mtl['code_%03d' % k]
        assert np.array_equal(np.array(m['Kd'] + m['Ks'] + m['Pr'], np.float32), rows_h[k]) and m['illum'] == [2.0]
        alpha = float(rows_h[k, 6]) ** 2
        assert abs(m['Ns'][0] - min(max(2.0 / alpha ** 2 - 2.0, 0.0), 1000.0)) <= 1e-6 * max(m['Ns'][0], 1.0)
    # the parts: together the kept faces of the input, as position triples
    kept = np.flatnonzero(want['face_code'] >= 0)
    whole = sorted(tuple(map(tuple, tri)) for tri in v.cpu().numpy()[tris[kept].astype(np.int64)].tolist())
    parts = []
    for k in used:
        faces = _ply_faces_as_points(os.path.join(out, 'code_%03d.ply' % k))
        assert len(faces) == want['face_count'][k]
        parts += faces
    assert sorted(parts) == whole
    # the record: counts as the model's, regions as a union-find over the same-code edges, areas as a float64 sum
    assert rec['n_codes'] == K and rec['changed'] == want_changed.tolist() and rec['dropped_faces'] == want['dropped'] == 0
    assert [c['vertices'] for c in rec['codes']] == want['vert_count'] and [c['faces'] for c in rec['codes']] == want['face_count']
    assert [c['regions'] for c in rec['codes']] == mm.region_counts(tris[kept], want_lab, K)
    p = v.cpu().numpy().astype(np.float64)[tris.astype(np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    n = max(want['face_count'])
    for k in range(K):
        ref_area = float(area[want['face_code'] == k].sum())
        assert abs(rec['codes'][k]['area'] - ref_area) <= (n + 8) * 2.0 ** -52 * ref_area, (k, rec['codes'][k]['area'], ref_area)
    assert abs(sum(c['area'] for c in rec['codes']) - 4 * np.pi * 0.75 ** 2) < 0.5          # (a coarse sphere of radius 0.75: 7.07)


def test_material_mesh_run_reads_a_ply_and_writes_the_codes_asked_for(vq, tmp_path):
    from vqnerf_release_amd.decomp import material_mesh
    model, _ = vq
    v, t = _sphere()
    nrm = torch.nn.functional.normalize(v, dim=-1)
    src = str(tmp_path / 'in.ply')
    mesh.write_ply(src, v, t, normals=nrm)
    rec = material_mesh.run(model, src, str(tmp_path / 'out'), smooth=0, parts=True, codes=[1])
    assert rec['changed'] == [] and rec['smooth'] == 0
    assert 'code_001.ply' in os.listdir(tmp_path / 'out') and not any(f.startswith('code_00') and f != 'code_001.ply' for f in os.listdir(tmp_path / 'out'))
    pv, pt, pn, extra = mesh.read_ply(str(tmp_path / 'out' / 'material_mesh.ply'), extra=['material'])
    assert torch.equal(pn, nrm) and torch.equal(extra['material'], model.materials_at(v)['code'])     # smooth = 0: the codes as they are
    from tests.test_mesh_materials_model import _parse_obj
    obj = _parse_obj(str(tmp_path / 'out' / 'material_mesh.obj'))
    assert len(obj['vn']) == v.shape[0] and sum(len(g[1]) for g in obj['groups']) == t.shape[0]
    with pytest.raises(ValueError):
        material_mesh.run(model, (v, t), str(tmp_path / 'bad'), branch='other')
