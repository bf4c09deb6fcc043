"""CPU: the plain statement of the mesh-material kernels (tests/mesh_materials_model.py) on cases worked by hand, the PLY / OBJ / MTL
writers of geo/mesh.py read back by a small parser of this file's own, and the Python constants against the header's #defines."""
import struct

import numpy as np
import pytest
import torch

from tests import abi_headers
from tests import mesh_materials_model as mm
from vqnerf_release_amd import _C
from vqnerf_release_amd.geo import mesh

TETRA = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]


def test_tetrahedron_with_four_codes():
    # every vertex hears each of the three other codes twice (each neighbour shares two triangles with it) and itself self_weight times
    codes = [3, 1, 2, 0]
    got, changed = mm.label_mode(TETRA, codes, 4, self_weight=1)
    assert got.tolist() == [0, 0, 0, 1] and changed.tolist() == [4]         # 2 > 1: the smallest other code
    for w in (2, 3):                                                      # the own code holds the maximum: kept
        got, changed = mm.label_mode(TETRA, codes, 4, self_weight=w)
        assert got.tolist() == codes and changed.tolist() == [0]
    # two rounds read the round before, not the input: [0, 0, 0, 1] -> vertex 3 hears code 0 six times
    got, changed = mm.label_mode(TETRA, codes, 4, self_weight=1, iters=2)
    assert got.tolist() == [0, 0, 0, 0] and changed.tolist() == [4, 1]
    assert mm.face_codes(TETRA, codes, 4).tolist() == [1, 0, 0, 0]            # three distinct codes: the minimum
    s = mm.split(TETRA, codes, 4)
    assert s['face_src'].tolist() == [1, 2, 3, 0] and s['face_offset'] == [0, 3, 4, 4, 4] and s['face_count'] == [3, 1, 0, 0]
    assert s['vert_src'].tolist() == [0, 1, 2, 3, 0, 1, 2] and s['vert_offset'] == [0, 4, 7, 7, 7]
    assert s['tris_local'].tolist() == [[0, 3, 1], [0, 2, 3], [1, 3, 2], [0, 1, 2]]
    assert s['n_faces'] == 4 and s['n_slots'] == 7 and s['dropped'] == 0


def test_both_tie_rules():
    tri, codes = [(0, 1, 2)], [2, 0, 1]
    # own code among the holders of the maximum (1 : 1 : 1): kept, although a smaller code ties
    assert mm.label_mode(tri, codes, 3, self_weight=1)[0].tolist() == [2, 0, 1]
    # own code below the maximum (0 against 1 : 1): the SMALLEST code that holds it
    got, changed = mm.label_mode(tri, codes, 3, self_weight=0)
    assert got.tolist() == [0, 1, 0] and changed.tolist() == [3]


def test_degenerate_a_a_b():
    # vertex 0 is corners 0 and 1: it hears (code[0], code[1]) and (code[1], code[0]); vertex 1 is corner 2 and hears code[0] twice
    got, changed = mm.label_mode([(0, 0, 1)], [0, 1], 2, self_weight=0)
    assert got.tolist() == [0, 0] and changed.tolist() == [1]
    got, changed = mm.label_mode([(0, 0, 1)], [1, 0], 2, self_weight=0)
    assert got.tolist() == [1, 1] and changed.tolist() == [1]              # 2 : 2 at vertex 0, its own code among them
    got, _ = mm.label_mode([(0, 0, 1)], [1, 0], 2, self_weight=3)
    assert got.tolist() == [1, 0]                                         # 3 own votes against 2
    assert mm.face_codes([(0, 0, 1), (0, 1, 0), (1, 0, 0)], [0, 1], 2).tolist() == [0, 0, 0]
    assert mm.face_codes([(0, 0, 1), (0, 1, 0), (1, 0, 0)], [1, 0], 2).tolist() == [1, 1, 1]


def test_unused_vertex_and_no_votes():
    tris, codes = TETRA, [3, 1, 2, 0, 2]                                  # vertex 4: no triangle uses it
    for w in (0, 1, 5):
        assert mm.label_mode(tris, codes, 4, self_weight=w)[0][4] == 2
    # self_weight = 0 and no vote at all: every vertex keeps its code
    got, changed = mm.label_mode(np.zeros((0, 3), np.int32), [1, 0, 3], 4, self_weight=0, iters=2)
    assert got.tolist() == [1, 0, 3] and changed.tolist() == [0, 0]


def test_caller_errors_in_the_model():
    # an index outside [0, V): the triangle votes for nothing, has face code -1 and is left out; a code outside [0, K) casts no vote
    tris = [(0, 1, 2), (0, 1, 3), (0, -1, 1)]
    got, _ = mm.label_mode(tris, [0, 1, 1], 2, self_weight=0)
    assert got.tolist() == [1, 1, 1]                                      # only (0, 1, 2) voted: 0 hears 1, 1; 1 and 2 hear 0 : 1 and keep
    assert mm.face_codes(tris, [0, 1, 1], 2).tolist() == [1, -1, -1]
    got, _ = mm.label_mode([(0, 1, 2)], [0, 7, 1], 2, self_weight=0)
    assert got.tolist() == [1, 0, 0]                                      # vertex 1 (code 7) votes for nothing and takes the smallest holder
    assert mm.face_codes([(0, 1, 2)], [0, 7, 1], 2).tolist() == [-1]
    s = mm.split(tris, [0, 1, 1], 2)
    assert s['face_src'].tolist() == [0] and s['dropped'] == 2 and s['vert_src'].tolist() == [0, 1, 2]


def test_region_counts_and_icosphere():
    v, t = mm.icosphere(1)
    assert v.shape == (42, 3) and t.shape == (80, 3) and np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-6)
    edges = {tuple(sorted((int(a), int(b)))) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))}
    assert len(edges) == 120 and 42 - 120 + 80 == 2                      # closed, genus 0
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert (np.einsum('ij,ij->i', n, v[t].mean(1)) > 0).all()              # counter-clockwise from outside
    codes = (v[:, 2] > 0).astype(np.int32)                               # two caps
    assert mm.region_counts(t, codes, 3) == [1, 1, 0]
    codes[np.argmax(v[:, 2])] = 2                                        # an island on the upper cap
    assert mm.region_counts(t, codes, 3) == [1, 1, 1]


# ---- the writers, read back by a parser of this file's own ----------------------------------------------------------------------------
def _parse_ply(path):
    """-> ({vertex property: array}, faces [T, 3]) of a binary little-endian PLY with scalar vertex properties and triangle faces"""
    types = {'float': ('f', 4), 'int': ('i', 4), 'uchar': ('B', 1)}
    raw = open(path, 'rb').read()
    head, body = raw.split(b'end_header\n', 1)
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    n_v = next(int(l.split()[2]) for l in lines if l.startswith('element vertex'))
    n_f = next(int(l.split()[2]) for l in lines if l.startswith('element face'))
    props = [l.split()[1:] for l in lines if l.startswith('property') and 'list' not in l]
    fmt = '<' + ''.join(types[t][0] for t, _ in props)
    size = struct.calcsize(fmt)
    rows = [struct.unpack_from(fmt, body, i * size) for i in range(n_v)]
    vert = {name: np.array([r[j] for r in rows]) for j, (_, name) in enumerate(props)}
    faces = [struct.unpack_from('<Biii', body, n_v * size + i * 13) for i in range(n_f)]
    assert all(f[0] == 3 for f in faces) and len(body) == n_v * size + n_f * 13
    return vert, np.array([f[1:] for f in faces], np.int64).reshape(-1, 3), [name for _, name in props]


def _mesh():
    v, t = mm.icosphere(0)
    rng = np.random.default_rng(3)
    return v, t, rng.normal(size=v.shape).astype(np.float32), rng.integers(0, 256, v.shape).astype(np.uint8), rng


def test_write_ply_extra_and_read_back(tmp_path):
    v, t, nrm, col, rng = _mesh()
    extra = {'spec': rng.uniform(size=len(v)).astype(np.float32), 'rough': torch.tensor(rng.uniform(size=len(v)).astype(np.float32)),
             'material': rng.integers(0, 128, len(v)).astype(np.int32), 'flag': rng.integers(0, 2, len(v)).astype(np.uint8)}
    path = str(tmp_path / 'm.ply')
    mesh.write_ply(path, v, t, normals=nrm, colors=col, extra=extra)
    vert, faces, order = _parse_ply(path)
    assert order == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'spec', 'rough', 'material', 'flag']
    assert np.array_equal(faces, t) and np.array_equal(np.stack([vert[k] for k in 'xyz'], 1).astype(np.float32), v)
    assert np.array_equal(np.stack([vert[k] for k in ('red', 'green', 'blue')], 1), col)
    for k, a in extra.items():
        a = a.numpy() if torch.is_tensor(a) else a
        assert np.array_equal(vert[k].astype(a.dtype), a), k
    head = open(path, 'rb').read().split(b'end_header')[0].decode()
    assert 'property float spec\nproperty float rough\nproperty int material\nproperty uchar flag\n' in head
    # the project's reader: the same three values as before, and the extras on request, in the file's types
    got = mesh.read_ply(path, device='cpu')
    assert len(got) == 3 and np.array_equal(got[0].numpy(), v) and np.array_equal(got[1].numpy(), t) and np.array_equal(got[2].numpy(), nrm)
    got = mesh.read_ply(path, device='cpu', extra=['material', 'rough', 'red'])
    assert len(got) == 4 and list(got[3]) == ['material', 'rough', 'red']
    assert got[3]['material'].dtype == torch.int32 and np.array_equal(got[3]['material'].numpy(), extra['material'])
    assert got[3]['rough'].dtype == torch.float32 and torch.equal(got[3]['rough'], extra['rough'])
    assert got[3]['red'].dtype == torch.uint8 and np.array_equal(got[3]['red'].numpy(), col[:, 0])
    with pytest.raises(_C.VqnError, match='no property'):
        mesh.read_ply(path, device='cpu', extra=['nothing'])
    # without the new arguments: the bytes of before
    a, b = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')
    mesh.write_ply(a, v, t, normals=nrm, colors=col)
    mesh.write_ply(b, v, t, normals=nrm, colors=col, extra={})
    plain = open(a, 'rb').read()
    assert plain == open(b, 'rb').read() and len(plain.split(b'end_header\n', 1)[1]) == len(v) * 27 + len(t) * 13
    for bad in ({'x': np.zeros(len(v), np.float64)}, {'x': np.zeros(len(v) + 1, np.float32)}, {'a b': np.zeros(len(v), np.float32)}):
        with pytest.raises(ValueError):
            mesh.write_ply(a, v, t, extra=bad)


def _parse_obj(path):
    out = dict(v=[], vn=[], groups=[], mtllib=None)
    for line in open(path):
        w = line.split()
        if not w:
            continue
        if w[0] == 'mtllib':
            out['mtllib'] = w[1]
        elif w[0] in ('v', 'vn'):
            out[w[0]].append([float(x) for x in w[1:]])
        elif w[0] == 'usemtl':
            out['groups'].append((w[1], []))
        elif w[0] == 'f':
            out['groups'][-1][1].append([[int(i) for i in c.split('//')] for c in w[1:]])
    return out


def _parse_mtl(path):
    out, cur = {}, None
    for line in open(path):
        w = line.split()
        if w and w[0] == 'newmtl':
            cur = out[w[1]] = {}
        elif w and not w[0].startswith('#'):
            cur[w[0]] = [float(x) for x in w[1:]]
    return out


def test_write_obj_and_mtl(tmp_path):
    v, t, nrm, _, rng = _mesh()
    codes = rng.integers(0, 4, len(v)).astype(np.int32)
    codes[codes == 2] = 3                                                # group 2 stays empty
    s = mm.split(t, codes, 5)
    names = ['code_%03d' % k for k in range(5)]
    path = str(tmp_path / 'mesh.obj')
    mesh.write_obj(path, v, t[s['face_src']], s['face_offset'], names, normals=nrm)
    obj = _parse_obj(path)
    assert obj['mtllib'] == 'mesh.mtl'
    assert np.array_equal(np.array(obj['v'], np.float32), v) and np.array_equal(np.array(obj['vn'], np.float32), nrm)   # nine digits: exact
    used = [k for k in range(5) if s['face_count'][k]]
    assert [g[0] for g in obj['groups']] == [names[k] for k in used] and 2 not in used and 4 not in used
    for k, (_, faces) in zip(used, obj['groups']):
        faces = np.array(faces)
        assert len(faces) == s['face_count'][k] and np.array_equal(faces[:, :, 0], faces[:, :, 1])
        assert np.array_equal(faces[:, :, 0] - 1, t[s['face_src'][s['face_offset'][k]: s['face_offset'][k + 1]]])
    plain = str(tmp_path / 'plain.obj')
    mesh.write_obj(plain, torch.tensor(v), torch.tensor(t[s['face_src']]), s['face_offset'], names, mtllib='other.mtl')
    obj = _parse_obj(plain)
    assert obj['mtllib'] == 'other.mtl' and not obj['vn'] and np.array(obj['groups'][0][1]).shape[1:] == (3, 1)
    with pytest.raises(ValueError):
        mesh.write_obj(plain, v, t, [0, 1], names)
    rows = [dict(Kd=rng.uniform(size=3).astype(np.float32), Ks=rng.uniform(size=3).astype(np.float32), Pr=np.float32(0.37), Ns=12.5,
                 illum=2) for _ in names]
    mesh.write_mtl(str(tmp_path / 'mesh.mtl'), names, rows)
    mtl = _parse_mtl(str(tmp_path / 'mesh.mtl'))
    assert list(mtl) == names
    for name, row in zip(names, rows):
        assert np.array_equal(np.array(mtl[name]['Kd'], np.float32), row['Kd']) and np.array_equal(np.array(mtl[name]['Ks'], np.float32), row['Ks'])
        assert np.float32(mtl[name]['Pr'][0]) == row['Pr'] and mtl[name]['Ns'] == [12.5] and mtl[name]['illum'] == [2.0]


def test_mtl_rows_follow_the_material_rows():
    from vqnerf_release_amd.decomp import material_mesh
    rows = torch.tensor([[0.5, 0.25, 0.125, 0.04, 0.05, 0.06, 1.0], [0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 0.5], [1, 1, 1, 1, 1, 1, 0.01]])
    got = material_mesh.mtl_rows(rows)
    assert got[0]['Kd'] == [0.5, 0.25, 0.125] and np.allclose(got[0]['Ks'], [0.04, 0.05, 0.06], rtol=1e-7) and got[0]['illum'] == 2
    # alpha = rough^2 (util/microfacet.py's alpha): rough 1 -> Ns = 2 / 1 - 2 = 0; rough 0.5 -> alpha^2 = 1 / 16 -> 30; a mirror clips
    assert [g['Ns'] for g in got] == [0.0, 30.0, 1000.0] and [g['Pr'] for g in got] == [1.0, 0.5, float(np.float32(0.01))]


def test_python_constants_equal_the_defines():
    defined = abi_headers.defines('vqn_mesh_materials.h')
    assert defined == {'VQN_MESHMAT_MAX_CODES': _C.MESHMAT_MAX_CODES, 'VQN_MESHMAT_FACES_PER_BLOCK': _C.MESHMAT_FACES_PER_BLOCK,
                       'VQN_MESHMAT_WORD_BITS': _C.MESHMAT_WORD_BITS}
    assert _C.MESHMAT_MAX_CODES == 128
    assert _C.mesh_split_shape(0, 0) == (1, 0) and _C.mesh_split_shape(513, 33) == (2, 2) and _C.mesh_split_shape(512, 32) == (1, 1)
