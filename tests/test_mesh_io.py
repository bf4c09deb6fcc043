"""CPU: geo/mesh.py write_ply -- binary little-endian PLY, float x y z vertices, `list uchar int` faces -- read back by a reader kept
here: counts, dtypes and values round-trip exactly, the empty mesh included."""
import numpy as np
import pytest
import torch

from vqnerf_release_amd.geo.mesh import write_ply


def read_ply(path):
    """-> (vertices float32 [V,3], triangles int32 [T,3]) of a file in exactly the layout write_ply promises"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    assert lines[2].startswith('element vertex ') and lines[3:6] == ['property float x', 'property float y', 'property float z']
    assert lines[6].startswith('element face ') and lines[7] == 'property list uchar int vertex_indices'
    assert lines[8:] == ['end_header', '']
    nv, nf = int(lines[2].split()[-1]), int(lines[6].split()[-1])
    verts = np.frombuffer(raw, '<f4', 3 * nv, end).reshape(nv, 3)
    faces = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), nf, end + 12 * nv)
    assert len(raw) == end + 12 * nv + 13 * nf and (faces['n'] == 3).all()
    return verts, faces['v'].astype(np.int32)


@pytest.mark.parametrize('as_tensor', [False, True])
def test_round_trip(tmp_path, as_tensor):
    rng = np.random.default_rng(5)
    v = rng.normal(size=(37, 3)).astype(np.float32)
    v[0] = [np.float32(1e-38), -0.0, np.float32(3.4e38)]
    t = rng.integers(0, 37, size=(61, 3)).astype(np.int32)
    path = str(tmp_path / 'm.ply')
    write_ply(path, torch.tensor(v) if as_tensor else v, torch.tensor(t) if as_tensor else t)
    gv, gt = read_ply(path)
    assert gv.dtype == np.float32 and gt.dtype == np.int32 and gv.shape == (37, 3) and gt.shape == (61, 3)
    assert np.array_equal(gv.view(np.int32), v.view(np.int32)) and np.array_equal(gt, t)


def test_float64_vertices_and_int64_triangles_are_written_as_float_and_int(tmp_path):
    v = np.array([[0.1, 0.2, 0.3], [1, 2, 3], [4, 5, 6]], np.float64)
    t = np.array([[0, 1, 2]], np.int64)
    path = str(tmp_path / 'm.ply')
    write_ply(path, v, t)
    gv, gt = read_ply(path)
    assert np.array_equal(gv, v.astype(np.float32)) and np.array_equal(gt, t.astype(np.int32))


def test_empty_mesh(tmp_path):
    path = str(tmp_path / 'e.ply')
    write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    gv, gt = read_ply(path)
    assert gv.shape == (0, 3) and gt.shape == (0, 3)
