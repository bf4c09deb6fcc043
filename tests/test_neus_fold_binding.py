"""CPU: vqn_neus_fold_pack, the one entry point declared outside include/vqnerf_hip.h (include/vqn_neus_fold.h): its row of
`_C.ABI_FOLD` against that header, what `_C.lib()` installs for it, and that the library exports what the two public headers declare
and nothing else.  (tests/test_binding.py and tests/test_abi.py hold the 91 functions of include/vqnerf_hip.h the same way.)"""
import os
import re
import shutil
import subprocess

from vqnerf_release_amd import _C
from tests.test_binding import _kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototypes(header):
    txt = open(os.path.join(ROOT, 'include', header)).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', ' ', txt, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r'([\w\s*]+?)\s*\b(vqn_\w+)\s*\(([^)]*)\)\s*;', txt):
        params = [p for p in params.split(',') if p.strip() not in ('', 'void')]
        out[name] = (_kind(ret, True), ''.join(_kind(p) for p in params))
    return out


def test_fold_signature_matches_its_header():
    declared = _prototypes('vqn_neus_fold.h')
    assert declared == _C.ABI_FOLD
    assert not set(declared) & set(_C.ABI)                       # one table per header, no name in both


def test_lib_installs_the_fold_signature_and_exports_only_declared_names():
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    lib = _C.lib()
    for name, (ret, params) in _C.ABI_FOLD.items():
        f = getattr(lib, name)
        assert f.restype is _C._CTYPES[ret] and list(f.argtypes) == [_C._CTYPES[k] for k in params], name
    assert all(hasattr(lib, n) for n in _C.ABI)
    if shutil.which('nm') is None:                               # (no binutils: the exact export list cannot be read)
        return
    nm = subprocess.run(['nm', '-D', '--defined-only', _C.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if ' T vqn_' in l)
    assert exported == sorted(list(_C.ABI) + list(_C.ABI_FOLD))
