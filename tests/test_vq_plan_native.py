"""CPU: the host-only C++ of the VQ host side -- tiling, LDS bytes, which assign kernel runs, the grids and the form of the EMA
statistics (csrc/vq_plan.h, with the grid rule of csrc/launch.h) -- as a stand-alone program under ASan / UBSan
(tests/native/vq_plan_host.cpp): a table of shapes against the decisions the entry points took before the plan existed, every
refusal once and both sides of every threshold."""
import shutil

import pytest

from tests.test_sanitizers import SAN, _run

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')


def test_vq_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'vq_plan_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'include', '-I', 'vqnerf_release_amd/csrc', 'tests/native/vq_plan_host.cpp', '-o', exe],
               exe, tmp_path)
    assert 'vq plan ok: 79 rows' in out
