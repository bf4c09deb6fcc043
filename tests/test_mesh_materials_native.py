"""CPU: the host-only C++ of the mesh-material kernels -- limits, bitmap geometry, face blocks, the label clean-up's scratch layout and
refusals (csrc/mesh_materials_plan.h) -- as a stand-alone program under ASan / UBSan (tests/native/mesh_materials_host.cpp)."""
import shutil

import pytest

from tests.test_sanitizers import SAN, _run

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')


def test_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'mesh_materials_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'vqnerf_release_amd/csrc', 'tests/native/mesh_materials_host.cpp', '-o', exe], exe, tmp_path)
    assert 'mesh materials plan ok: 376 shapes, 13 refusals' in out
