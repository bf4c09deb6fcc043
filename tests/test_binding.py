"""CPU: the package's ctypes binding (vqnerf_release_amd/_C.py) -- its signature table against include/vqnerf_hip.h, and the one scratch
policy of the fused kernels."""
import os

import torch

from tests import abi_headers
from vqnerf_release_amd import _C


def test_signature_table_matches_the_header():
    declared = abi_headers.prototypes('vqnerf_hip.h')
    assert len(declared) == 91
    assert sorted(_C.ABI) == sorted(declared)
    wrong = {n: (_C.ABI[n], declared[n]) for n in declared if _C.ABI[n] != declared[n]}
    assert not wrong, wrong


def test_lib_installs_the_table():
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    lib = _C.lib()
    for name, (ret, params) in _C.ABI.items():
        f = getattr(lib, name)
        assert f.restype is _C._CTYPES[ret], name
        assert list(f.argtypes) == [_C._CTYPES[k] for k in params], name


def _fresh_scratch(monkeypatch):
    monkeypatch.setattr(_C, '_scratch_cache', {})
    monkeypatch.setattr(_C, '_scratch_held', [])


def test_scratch_reuses_and_grows_one_buffer_per_key(monkeypatch):
    _fresh_scratch(monkeypatch)
    a = _C._scratch('fine', 1024, 'cpu', stream=7, capturing=False)
    assert a.numel() == 1024 and a.dtype == torch.uint8
    assert _C._scratch('fine', 512, 'cpu', stream=7, capturing=False) is a         # a smaller request reuses the buffer
    assert _C._scratch('bwd', 512, 'cpu', stream=7, capturing=False) is not a      # other tag, other stream: other buffers
    assert _C._scratch('fine', 512, 'cpu', stream=8, capturing=False) is not a
    b = _C._scratch('fine', 4096, 'cpu', stream=7, capturing=False)                # grown: the uncaptured buffer is dropped
    assert b.numel() == 4096 and not _C._scratch_held
    assert not any(e[0] is a for e in _C._scratch_cache.values())
    assert len(_C._scratch_cache) == 3


def test_scratch_handed_to_a_capture_outlives_its_replacement(monkeypatch):
    _fresh_scratch(monkeypatch)
    a = _C._scratch('refl_bwd', 1024, 'cpu', stream=7, capturing=True)           # recorded into a graph
    assert _C._scratch('refl_bwd', 256, 'cpu', stream=7, capturing=False) is a   # reuse keeps it held
    b = _C._scratch('refl_bwd', 2048, 'cpu', stream=7, capturing=False)
    assert b is not a and len(_C._scratch_held) == 1 and _C._scratch_held[0] is a
    c = _C._scratch('refl_bwd', 4096, 'cpu', stream=7, capturing=False)          # b was never captured: dropped, not held
    assert c is not b and len(_C._scratch_held) == 1
    assert len(_C._scratch_cache) == 1
