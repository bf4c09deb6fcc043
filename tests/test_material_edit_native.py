"""CPU: the host-only C++ of the material selection kernel -- the packing and validation of a selection program
(csrc/material_edit_plan.h) -- as a stand-alone program under ASan / UBSan (tests/native/material_edit_host.cpp): the maximal program,
ordinary ones and every refused one, each with its reason."""
import shutil

import pytest

from tests.test_sanitizers import SAN, _run

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')


def test_program_packing_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'material_edit_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'vqnerf_release_amd/csrc', 'tests/native/material_edit_host.cpp', '-o', exe], exe, tmp_path)
    assert 'material edit plan ok: the maximal program, 16 refusals' in out
