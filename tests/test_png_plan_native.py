"""CPU: the host-only C++ of the device PNG encoder -- the geometry, the bytes in front of IDAT, the prefabricated tables with their
canonical codes and pre-encoded block headers, the candidate distances and every refusal (csrc/png_plan.h) -- as a stand-alone
program under ASan / UBSan (tests/native/png_plan_host.cpp).  No Python code runs under a sanitizer."""
import os
import re
import shutil

import pytest

from tests import png_model
from tests.test_sanitizers import SAN, _run

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'png_plan_host')
    out = _run(['g++', '-std=c++17'] + SAN + ['-I', 'vqnerf_release_amd/csrc', 'tests/native/png_plan_host.cpp', '-o', exe], exe, tmp_path)
    assert 'png plan ok: 2 heads, 2 table headers, 18 refusals' in out


def _table(src, name):
    body = re.search(name + r'\[\d+\] = \{(.*?)\};', src, re.S).group(1)
    return bytes(int(v, 16) for v in re.findall(r'0x[0-9a-f]{2}', body))


def test_the_programs_tables_are_the_models():
    """the bytes in the program are what the model writes today"""
    src = open(os.path.join(ROOT, 'tests', 'native', 'png_plan_host.cpp')).read()
    assert _table(src, 'kHeadA') == png_model.head(17, 23, 3)
    assert _table(src, 'kHeadB') == png_model.head(800, 640, 2)
    tabs = png_model.tables()
    for k in (0, 13):
        bits = png_model.Bits()
        bits.put(0, 1)
        bits.bits.extend(tabs[k].header.bits)
        assert _table(src, f'kTableHeader{k}') == bits.tobytes()
    want = [int(v) for v in re.search(r'kHeaderBits\[15\] = \{(.*?)\};', src).group(1).split(',')]
    assert want == [1 + len(t.header) for t in tabs]
    t, f = tabs[3], tabs[14]
    assert (t.lit_codes[0], t.lit_lens[0], t.lit_codes[256], t.lit_lens[256], t.lit_codes[285], t.lit_lens[285], t.dist_codes[29],
            t.dist_lens[29]) == (0x0, 3, 0x7ee, 11, 0x1, 3, 0x15, 5)
    assert (f.lit_codes[0], f.lit_codes[144], f.lit_codes[256], f.lit_codes[280], f.dist_codes[29]) == (0x30, 0x190, 0x0, 0xc0, 0x1d)
