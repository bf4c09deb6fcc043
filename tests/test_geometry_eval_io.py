"""CPU: the host side of the geometry scores -- `mesh.read_ply` (round trips of `write_ply`, ASCII point clouds, files without faces,
refusals), the grid planner through the library (no GPU) and as a stand-alone program under ASan / UBSan
(tests/native/geometry_plan_host.cpp), the refusals of the device calls that launch nothing, and the new header's #defines against
their mirrors in `_C`."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from tests import abi_headers
from tests.test_sanitizers import SAN, _run
from vqnerf_release_amd import _C
from vqnerf_release_amd.geo import mesh

HEADER = 'vqn_geometry_eval.h'


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    return _C.lib()


def _mesh(rng, V=9, T=7):
    return rng.standard_normal((V, 3)).astype(np.float32), rng.integers(0, V, (T, 3)).astype(np.int32)


@pytest.mark.parametrize('normals,colors', [(False, False), (True, False), (False, True), (True, True)])
def test_read_ply_reads_what_write_ply_writes(tmp_path, normals, colors):
    rng = np.random.default_rng(0)
    v, t = _mesh(rng)
    n = rng.standard_normal((len(v), 3)).astype(np.float32) if normals else None
    c = rng.integers(0, 256, (len(v), 3)).astype(np.uint8) if colors else None
    path = str(tmp_path / 'm.ply')
    mesh.write_ply(path, v, t, normals=n, colors=c)
    rv, rt, rn = mesh.read_ply(path, device='cpu')
    assert rv.dtype == torch.float32 and rt.dtype == torch.int32
    assert np.array_equal(rv.numpy().view(np.int32), v.view(np.int32)) and np.array_equal(rt.numpy(), t)
    assert (rn is None) if n is None else np.array_equal(rn.numpy().view(np.int32), n.view(np.int32))


def test_read_ply_ascii_point_cloud_with_normals(tmp_path):
    path = str(tmp_path / 'cloud.ply')
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\ncomment a scan\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n'
                'property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n'
                'end_header\n0 0.5 1 0 0 1 255 0 0\n-1.25 2 3e-3 0 1 0 0 255 0\n7 8 9 1 0 0 0 0 255\n')
    v, t, n = mesh.read_ply(path, device='cpu')
    assert t is None
    assert np.array_equal(v.numpy(), np.float32([[0, 0.5, 1], [-1.25, 2, 3e-3], [7, 8, 9]]))
    assert np.array_equal(n.numpy(), np.float32([[0, 0, 1], [0, 1, 0], [1, 0, 0]]))


def test_read_ply_ascii_mesh_and_binary_cloud_without_faces(tmp_path):
    path = str(tmp_path / 'tri.ply')
    with open(path, 'w') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex 4\nproperty double x\nproperty double y\nproperty double z\n'
                'element face 2\nproperty list uchar int vertex_index\nend_header\n0 0 0\n1 0 0\n0 1 0\n0 0 1\n3 0 1 2\n3 0 2 3\n')
    v, t, n = mesh.read_ply(path, device='cpu')
    assert n is None and v.dtype == torch.float32 and v.shape == (4, 3) and t.tolist() == [[0, 1, 2], [0, 2, 3]]
    pts = np.random.default_rng(1).random((5, 3)).astype('<f4')
    path = str(tmp_path / 'scan.ply')
    with open(path, 'wb') as f:
        f.write(b'ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\nend_header\n')
        f.write(pts.tobytes())
    v, t, n = mesh.read_ply(path, device='cpu')
    assert t is None and n is None and np.array_equal(v.numpy(), pts)


def test_read_ply_refuses_what_it_does_not_read(tmp_path):
    head = 'element vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n'
    verts = np.zeros((4, 3), '<f4').tobytes()
    cases = {
        'big_endian': b'ply\nformat binary_big_endian 1.0\n' + head.encode() + verts + b'\x03' + np.array([0, 1, 2], '>i4').tobytes(),
        'quad_binary': b'ply\nformat binary_little_endian 1.0\n' + head.encode() + verts + b'\x04' + np.array([0, 1, 2, 3], '<i4').tobytes(),
        'quad_ascii': ('ply\nformat ascii 1.0\n' + head + '0 0 0\n' * 4 + '4 0 1 2 3\n').encode(),
        'cut_short': b'ply\nformat binary_little_endian 1.0\n' + head.encode() + verts[:-4],
        'bad_index': b'ply\nformat binary_little_endian 1.0\n' + head.encode() + verts + b'\x03' + np.array([0, 1, 4], '<i4').tobytes(),
        'no_xyz': b'ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n',
        'not_ply': b'solid\n',
    }
    for name, data in cases.items():
        path = str(tmp_path / (name + '.ply'))
        with open(path, 'wb') as f:
            f.write(data)
        with pytest.raises(_C.VqnError):
            mesh.read_ply(path, device='cpu')


# ---- the grid planner ----
def _dims_hold(g):
    return all(1 <= d <= _C.GEOM_MAX_AXIS for d in g.dims) and g.cells == g.dims[0] * g.dims[1] * g.dims[2] <= _C.GEOM_MAX_CELLS and g.h > 0


@pytest.mark.parametrize('ext', [(1, 1, 1), (2, 0.5, 3), (0, 1, 1), (1, 0, 0), (0, 0, 0), (1e-3, 1e3, 1)])
def test_plan_respects_the_caps(lib, ext):
    lo = np.float32([-1.5, 0.25, 3])
    hi = lo + np.float32(ext)
    for e in range(0, 31):
        for n in {1 << e, max(1, (1 << e) - 1)}:
            g = _C.geom_grid_plan(lo, hi, n)
            assert _dims_hold(g) and list(g.origin) == lo.tolist(), (n, list(g.dims), g.h)
            assert [int(np.floor((float(hi[a]) - float(lo[a])) / g.h)) + 1 for a in range(3)] == list(g.dims)


def test_plan_default_and_overrides(lib):
    lo, hi = [0, 0, 0], [1, 1, 1]
    g = _C.geom_grid_plan(lo, hi, 1000000)
    assert g.h == np.float32(np.sqrt(48.0 / 1e6)) and list(g.dims) == [145, 145, 145]
    g = _C.geom_grid_plan(lo, hi, 10, cell=0.25)
    assert g.h == 0.25 and list(g.dims) == [5, 5, 5] and g.cells == 125
    assert _C.geom_grid_plan(lo, hi, 10, cell=100.0).cells == 1
    grid = _C.GeomGrid()
    P = lambda a: np.float32(a).ctypes.data_as(ctypes.c_void_p)
    for cell in (1.0 / 2000, 1.0 / 300, float('inf')):                            # 2001 per axis; 301^3 cells; not finite
        assert lib.vqn_geom_grid_plan(P(lo), P(hi), 10, cell, ctypes.addressof(grid)) == -2
        assert 'vqn_geom_grid_plan' in lib.vqn_last_error().decode()
        with pytest.raises(ValueError):
            _C.geom_grid_plan(lo, hi, 10, cell=cell)
    assert lib.vqn_geom_grid_plan(P(lo), P(hi), 0, 0.0, ctypes.addressof(grid)) == -2
    assert lib.vqn_geom_grid_plan(P(lo), P(hi), 1 << 31, 0.0, ctypes.addressof(grid)) == -2
    assert lib.vqn_geom_grid_plan(None, P(hi), 10, 0.0, ctypes.addressof(grid)) == -1
    assert lib.vqn_geom_grid_plan(P(hi), P(lo), 10, 0.0, ctypes.addressof(grid)) == -1


@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')
def test_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'geometry_plan_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'include', '-I', 'vqnerf_release_amd/csrc', 'tests/native/geometry_plan_host.cpp', '-o', exe],
               exe, tmp_path)
    assert 'geometry plan ok' in out


def test_refusals_launch_nothing(lib):
    """the negative return codes of calls that never reach a launch: no pointer is read, so none needs to be real"""
    grid = _C.geom_grid_plan([0, 0, 0], [1, 1, 1], 10)
    G, X = ctypes.addressof(grid), 4096                                           # X: a non-null, 16-byte aligned stand-in
    big = 1 << 31
    assert lib.vqn_geom_tri_areas(X, 0, X, 1, X, None) == -2 and lib.vqn_geom_tri_areas(X, 3, X, big, X, None) == -2
    assert lib.vqn_geom_tri_areas(None, 3, X, 1, X, None) == -1
    assert lib.vqn_geom_sample_surface(X, 3, X, 1, X, X, 0, X, X, X, None) == 0                      # no samples: a no-op
    assert lib.vqn_geom_sample_surface(X, 3, X, 1, X, X, big, X, X, X, None) == -2
    assert lib.vqn_geom_sample_surface(X, 3, X, 1, None, X, 5, X, X, X, None) == -1
    assert lib.vqn_geom_cell_ids(X, 0, G, X, None) == 0 and lib.vqn_geom_cell_ids(X, big, G, X, None) == -2
    assert lib.vqn_geom_cell_ids(X, 5, None, X, None) == -1
    assert lib.vqn_geom_pack_sorted(X, 0, X, X, None) == -2 and lib.vqn_geom_pack_sorted(X, 5, X, X + 4, None) == -1
    assert lib.vqn_geom_nearest(X, 0, None, X, X, 5, G, float('inf'), X, X, None) == 0              # no queries: a no-op
    assert lib.vqn_geom_nearest(X, 5, None, X, X, 0, G, float('inf'), X, X, None) == -2             # no reference points
    assert lib.vqn_geom_nearest(X, big, None, X, X, 5, G, float('inf'), X, X, None) == -2
    assert lib.vqn_geom_nearest(X, 5, None, None, X, 5, G, float('inf'), X, X, None) == -1
    assert lib.vqn_geom_nearest(X, 5, None, X, X, 5, G, -1.0, X, X, None) == -1
    bad = _C.GeomGrid.from_buffer_copy(grid)
    bad.dims[0] = _C.GEOM_MAX_AXIS + 1
    assert lib.vqn_geom_nearest(X, 5, None, X, X, 5, ctypes.addressof(bad), float('inf'), X, X, None) == -2
    assert lib.vqn_geom_cell_ids(X, 5, ctypes.addressof(bad), X, None) == -2
    tau = (ctypes.c_double * 9)(*range(9))
    T = ctypes.addressof(tau)
    assert lib.vqn_geom_reduce_scratch_bytes(0) == 0 and lib.vqn_geom_reduce_scratch_bytes(big) == 0
    assert lib.vqn_geom_reduce_scratch_bytes(1) == _C.GEOM_OUT_WORDS * 8
    assert lib.vqn_geom_reduce_scratch_bytes(10 ** 9) == _C.GEOM_REDUCE_GRID_CAP * _C.GEOM_OUT_WORDS * 8
    assert lib.vqn_geom_reduce(X, X, 0, None, None, 5, T, 2, X, 1 << 20, X, None) == -2
    assert lib.vqn_geom_reduce(X, X, 5, None, None, 5, T, 9, X, 1 << 20, X, None) == -2            # more than 8 thresholds
    assert lib.vqn_geom_reduce(X, X, 5, None, None, 5, T, 2, X, 64, X, None) == -1                 # the scratch is too small
    assert lib.vqn_geom_reduce(X, X, 5, None, None, 5, T, 2, None, 1 << 20, X, None) == -1
    assert 'vqn_geom_reduce' in lib.vqn_last_error().decode()


# ---- the header ----
def test_python_constants_equal_the_defines():
    mirrors = {'VQN_GEOM_MAX_CELLS': _C.GEOM_MAX_CELLS, 'VQN_GEOM_MAX_AXIS': _C.GEOM_MAX_AXIS, 'VQN_GEOM_MAX_THRESHOLDS': _C.GEOM_MAX_THRESHOLDS,
               'VQN_GEOM_OUT_WORDS': _C.GEOM_OUT_WORDS, 'VQN_GEOM_THREADS': _C.GEOM_THREADS, 'VQN_GEOM_REDUCE_GRID_CAP': _C.GEOM_REDUCE_GRID_CAP}
    assert abi_headers.defines(HEADER) == mirrors
    assert mirrors['VQN_GEOM_MAX_CELLS'] == 1 << 24 and mirrors['VQN_GEOM_MAX_THRESHOLDS'] == 8


def test_the_grid_struct_is_the_headers():
    assert [f[0] for f in _C.GeomGrid._fields_] == abi_headers.struct_fields(HEADER, 'VqnGeomGrid') == ['origin', 'h', 'dims', 'cells']
    assert ctypes.sizeof(_C.GeomGrid) == 32
    assert HEADER in _C.ABI_BY_HEADER and len(_C.ABI_BY_HEADER[HEADER]) == 8
