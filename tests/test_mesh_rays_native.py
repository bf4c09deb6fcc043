"""CPU: the host-only C++ of the mesh ray caster -- the grid rule, the limits, the sizes of the launches and every refusal of its entry
points (csrc/mesh_rays_plan.h) -- as a stand-alone program under ASan / UBSan (tests/native/mesh_rays_host.cpp), and the Python
restatement of the header's limits."""
import shutil

import pytest

from tests.test_sanitizers import SAN, _run


@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')
def test_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'mesh_rays_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'vqnerf_release_amd/csrc', 'tests/native/mesh_rays_host.cpp', '-o', exe], exe, tmp_path)
    assert 'mesh rays plan ok: 27280 shapes, 70 refusals' in out


def test_python_restates_the_limits():
    from tests import abi_headers
    from vqnerf_release_amd import _C
    defined = abi_headers.defines('vqn_mesh_rays.h')
    mirrors = {'VQN_RAYS_MAX_AXIS': _C.RAYS_MAX_AXIS, 'VQN_RAYS_MAX_CELLS': _C.RAYS_MAX_CELLS, 'VQN_RAYS_STATS': _C.RAYS_STATS,
               'VQN_RAYS_MARGIN_INV': _C.RAYS_MARGIN_INV, 'VQN_RAYS_PACKED_FLOATS': _C.RAYS_PACKED_FLOATS,
               'VQN_RAYS_MAX_LIGHTS': _C.RAYS_MAX_LIGHTS, 'VQN_RAYS_TILE': _C.RAYS_TILE, 'VQN_RAYS_MIN_DIR_LOG2': _C.RAYS_MIN_DIR_LOG2,
               'VQN_RAYS_LANES_POINTS': _C.RAYS_LANES_POINTS, 'VQN_RAYS_LANES_LIGHTS': _C.RAYS_LANES_LIGHTS}
    assert defined == mirrors
    assert len(_C.RAYS_STAT_NAMES) == _C.RAYS_STATS
    assert (_C.RAYS_MAX_AXIS, _C.RAYS_MAX_CELLS) == (_C.GEOM_MAX_AXIS, _C.GEOM_MAX_CELLS)      # one struct VqnGeomGrid serves both
    from tests import mesh_rays_model as model
    assert (model.STATS, float(model.MARGIN), float(model.MIN_DIR)) == (_C.RAYS_STATS, 1.0 / _C.RAYS_MARGIN_INV, 2.0 ** _C.RAYS_MIN_DIR_LOG2)


def test_the_grid_plan_through_the_binding():
    """(host only: no device is touched)"""
    import os
    from vqnerf_release_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    g = _C.rays_grid_plan([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], 320)
    assert abs(g.h - (2 * 6 / 320) ** 0.5) < 1e-6 and list(g.dims) == [7, 7, 7] and g.cells == 343
    assert all(abs(o - (-0.5 - g.h / 2)) < 1e-6 for o in g.origin)
    assert list(_C.rays_grid_plan([0, 0, 0], [1, 2, 3], 10, cell=8.0).dims) == [2, 2, 2]
    with pytest.raises(ValueError, match='cell size'):
        _C.rays_grid_plan([0, 0, 0], [1, 1, 1], 10, cell=1e-4)
    with pytest.raises(ValueError, match='bounding box'):
        _C.rays_grid_plan([0, 0, 0], [1, -1, 1], 10)
