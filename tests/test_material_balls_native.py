"""CPU: the host-only C++ of the material-ball kernel -- grid, probe chunks, sheet geometry, sizes and refusals
(csrc/material_balls_plan.h) -- as a stand-alone program under ASan / UBSan (tests/native/material_balls_host.cpp)."""
import shutil

import pytest

from tests.test_sanitizers import SAN, _run

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')


def test_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'material_balls_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'vqnerf_release_amd/csrc', 'tests/native/material_balls_host.cpp', '-o', exe], exe, tmp_path)
    assert 'material balls plan ok: 384 probe / light shapes, 413 refusals' in out
