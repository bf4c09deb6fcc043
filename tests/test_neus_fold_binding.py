"""CPU: the entry points declared outside include/vqnerf_hip.h, in the area headers beside it (include/vqn_neus_fold.h for
vqn_neus_fold_pack, vqn_mesh.h, vqn_eval.h, vqn_material_edit.h, vqn_image_codec.h): their tables in `_C.ABI_BY_HEADER` against those
headers, what `_C.lib()` installs for them, and that the library exports what the public headers declare and nothing else.
(tests/test_abi_headers.py states the same per header; tests/test_binding.py and tests/test_abi.py hold the 91 functions of
include/vqnerf_hip.h.)"""
import os
import shutil
import subprocess

from tests import abi_headers
from vqnerf_release_amd import _C

AREA = {h: t for h, t in _C.ABI_BY_HEADER.items() if h != 'vqnerf_hip.h'}


def test_fold_signature_matches_its_header():
    assert abi_headers.prototypes('vqn_neus_fold.h') == AREA['vqn_neus_fold.h'] == {'vqn_neus_fold_pack': ('l', 'ppplppiippiplpp')}
    for header, table in AREA.items():
        assert abi_headers.prototypes(header) == table, header
        assert not set(table) & set(_C.ABI)                      # one table per header, no name in both


def test_lib_installs_the_fold_signature_and_exports_only_declared_names():
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    lib = _C.lib()
    for table in AREA.values():
        for name, (ret, params) in table.items():
            f = getattr(lib, name)
            assert f.restype is _C._CTYPES[ret] and list(f.argtypes) == [_C._CTYPES[k] for k in params], name
    assert all(hasattr(lib, n) for n in _C.ABI)
    if shutil.which('nm') is None:                               # (no binutils: the exact export list cannot be read)
        return
    nm = subprocess.run(['nm', '-D', '--defined-only', _C.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if ' T vqn_' in l)
    assert exported == sorted(list(_C.ABI) + [n for table in AREA.values() for n in table])
