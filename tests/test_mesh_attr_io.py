"""CPU: geo/mesh.py write_ply with per-vertex attributes -- float nx ny nz after z, uchar red green blue after those -- read back by
a reader kept here: counts, property order and values exact; without attributes the bytes are those of the bare layout, built here
independently."""
import struct

import numpy as np
import pytest
import torch

from vqnerf_release_amd.geo.mesh import write_ply

_TYPES = {'float': ('<f4', 4), 'uchar': ('u1', 1), 'int': ('<i4', 4)}


def read_ply_attr(path):
    """-> (vertex properties in file order [(name, type)], {name: column}, triangles int32 [T,3]) of a binary little-endian PLY with
    scalar vertex properties and `list uchar int` triangles"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0' and lines[-2:] == ['end_header', '']
    assert lines[2].startswith('element vertex ')
    nv = int(lines[2].split()[-1])
    props, i = [], 3
    while lines[i].startswith('property '):
        _, typ, name = lines[i].split()
        props.append((name, typ))
        i += 1
    assert lines[i].startswith('element face ') and lines[i + 1] == 'property list uchar int vertex_indices' and i + 4 == len(lines)
    nf = int(lines[i].split()[-1])
    dt = np.dtype([(name, _TYPES[typ][0]) for name, typ in props])
    assert dt.itemsize == sum(_TYPES[typ][1] for _, typ in props)                    # packed rows
    rows = np.frombuffer(raw, dt, nv, end)
    faces = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), nf, end + dt.itemsize * nv)
    assert len(raw) == end + dt.itemsize * nv + 13 * nf and (faces['n'] == 3).all()
    return props, {name: rows[name] for name, _ in props}, faces['v'].astype(np.int32)


XYZ = [('x', 'float'), ('y', 'float'), ('z', 'float')]
NRM = [('nx', 'float'), ('ny', 'float'), ('nz', 'float')]
RGB = [('red', 'uchar'), ('green', 'uchar'), ('blue', 'uchar')]


def _mesh():
    rng = np.random.default_rng(9)
    v = rng.normal(size=(29, 3)).astype(np.float32)
    v[0] = [np.float32(1e-38), -0.0, np.float32(3.4e38)]
    t = rng.integers(0, 29, size=(41, 3)).astype(np.int32)
    n = rng.normal(size=(29, 3)).astype(np.float32)
    c = rng.integers(0, 256, size=(29, 3)).astype(np.uint8)
    c[1] = [0, 128, 255]
    return v, t, n, c


@pytest.mark.parametrize('as_tensor', [False, True])
@pytest.mark.parametrize('with_normals, with_colors', [(True, False), (False, True), (True, True)])
def test_attributes_round_trip(tmp_path, with_normals, with_colors, as_tensor):
    v, t, n, c = _mesh()
    wrap = torch.tensor if as_tensor else (lambda a: a)
    path = str(tmp_path / 'm.ply')
    write_ply(path, wrap(v), wrap(t), normals=wrap(n) if with_normals else None, colors=wrap(c) if with_colors else None)
    props, cols, gt = read_ply_attr(path)
    assert props == XYZ + (NRM if with_normals else []) + (RGB if with_colors else [])
    assert all(len(col) == 29 for col in cols.values()) and gt.shape == (41, 3) and np.array_equal(gt, t)
    for k, name in enumerate('xyz'):
        assert np.array_equal(cols[name].view(np.int32), v[:, k].view(np.int32))
    if with_normals:
        for k, name in enumerate(('nx', 'ny', 'nz')):
            assert cols[name].dtype == np.float32 and np.array_equal(cols[name].view(np.int32), n[:, k].view(np.int32))
    if with_colors:
        for k, name in enumerate(('red', 'green', 'blue')):
            assert cols[name].dtype == np.uint8 and np.array_equal(cols[name], c[:, k])


def test_without_attributes_the_bytes_are_the_bare_layout(tmp_path):
    v, t, _, _ = _mesh()
    path = str(tmp_path / 'm.ply')
    write_ply(path, v, t)
    want = ('ply\nformat binary_little_endian 1.0\nelement vertex 29\nproperty float x\nproperty float y\nproperty float z\n'
            'element face 41\nproperty list uchar int vertex_indices\nend_header\n').encode('ascii')
    want += b''.join(struct.pack('<3f', *row) for row in v.tolist())
    want += b''.join(struct.pack('<B3i', 3, *row) for row in t.tolist())
    assert open(path, 'rb').read() == want
    write_ply(path, v, t, normals=None, colors=None)
    assert open(path, 'rb').read() == want


def test_empty_mesh_with_attributes(tmp_path):
    path = str(tmp_path / 'e.ply')
    write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), normals=np.zeros((0, 3), np.float32),
              colors=np.zeros((0, 3), np.uint8))
    props, cols, gt = read_ply_attr(path)
    assert props == XYZ + NRM + RGB and all(len(col) == 0 for col in cols.values()) and gt.shape == (0, 3)


def test_attribute_rows_must_match_the_vertices(tmp_path):
    v, t, n, c = _mesh()
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / 'm.ply'), v, t, normals=n[:-1])
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / 'm.ply'), v, t, colors=c[:-1])
