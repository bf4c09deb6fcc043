"""CPU: the host-only C++ of the mesh rasteriser -- limits, tile grid, scratch and bin sizes, the staged chunk's LDS and every refusal
of its three entry points (csrc/mesh_raster_plan.h) -- as a stand-alone program under ASan / UBSan (tests/native/mesh_raster_host.cpp)."""
import shutil

import pytest

from tests.test_sanitizers import SAN, _run

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')


def test_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'mesh_raster_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'vqnerf_release_amd/csrc', 'tests/native/mesh_raster_host.cpp', '-o', exe], exe, tmp_path)
    assert 'mesh raster plan ok: 3500 shapes, 68 refusals' in out


def test_python_restates_the_limits():
    from tests import abi_headers
    from vqnerf_release_amd import _C
    defined = abi_headers.defines('vqn_mesh_raster.h')
    mirrors = {'VQN_RASTER_TILE': _C.RASTER_TILE, 'VQN_RASTER_SUBPIXEL_BITS': _C.RASTER_SUBPIXEL_BITS, 'VQN_RASTER_MAX_SIDE': _C.RASTER_MAX_SIDE,
               'VQN_RASTER_CHUNK': _C.RASTER_CHUNK, 'VQN_RASTER_STATS': _C.RASTER_STATS, 'VQN_RASTER_MAX_CHANNELS': _C.RASTER_MAX_CHANNELS}
    assert defined == mirrors                                                     # (COORD_LIMIT is an expression: below)
    text = open(abi_headers.INCLUDE + '/vqn_mesh_raster.h').read()
    assert '#define VQN_RASTER_COORD_LIMIT (1 << 23)' in text and _C.RASTER_COORD_LIMIT == 1 << 23
    assert len(_C.RASTER_STAT_NAMES) == _C.RASTER_STATS
    from tests import mesh_raster_model as model
    assert (model.SUBPIXEL, model.COORD_LIMIT, model.STATS) == (1 << _C.RASTER_SUBPIXEL_BITS, _C.RASTER_COORD_LIMIT, _C.RASTER_STATS)
