"""CPU: the host-only C++ of the device JPEG encoder -- the tables, the geometry, the header bytes and every refusal
(csrc/jpeg_plan.h) -- as a stand-alone program under ASan / UBSan (tests/native/jpeg_plan_host.cpp): the headers of two geometries
against tables written by the float64 model, slot sizes at their bounds, and each refusal with its reason."""
import os
import re
import shutil

import pytest

from tests import jpeg_model
from tests.test_sanitizers import SAN, _run

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')


def test_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'jpeg_plan_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'vqnerf_release_amd/csrc', 'tests/native/jpeg_plan_host.cpp', '-o', exe], exe, tmp_path)
    assert 'jpeg plan ok: 2 headers, 15 refusals' in out


def test_the_programs_header_tables_are_the_models():
    """the two tables in the program are what the model writes today"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'tests', 'native', 'jpeg_plan_host.cpp')).read()
    for name, args in (('kHeaderA', (17, 23, 75, '420', 2)), ('kHeaderB', (800, 640, 90, '444', 100))):
        body = re.search(name + r'\[\d+\] = \{(.*?)\};', src, re.S).group(1)
        assert bytes(int(v, 16) for v in re.findall(r'0x[0-9a-f]{2}', body)) == jpeg_model.header(*args)
