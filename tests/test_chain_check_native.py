"""CPU: the descriptor rules of the Dense-stack kernels (csrc/chain_launch.h: chain_check_desc, one statement for the f32 and the
split-precision engine) as a stand-alone program under ASan / UBSan (tests/native/chain_check_host.cpp): the C planner's programs of
the shipped networks are accepted, every rule number refuses a program with exactly that field broken, and the two differences
between the engines are what they are said to be.  The Python packer's descriptors of the same networks reach the program as files
of int32 and must be accepted under their engine's rules.  No Python code runs under a sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

from tests.decomp_util import make_config, shipped_chain_programs
from tests.test_sanitizers import ROOT, SAN, _run
from vqnerf_release_amd.decomp.nerfactor.models import get_model_class

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not found')


def test_descriptor_rules_under_asan_ubsan(tmp_path):
    args = []
    model = get_model_class('vq_nfr')(make_config())
    model.build_nets(device='cpu', seed=5)
    for mode, name, (_, desc), _ in shipped_chain_programs(model):
        assert desc.dtype.name == 'int32' and desc.size == 272
        path = tmp_path / f'{mode}_{name}.i32'
        desc.tofile(path)
        args.append(f'{mode}:{path}')
    assert len(args) == 8
    exe = str(tmp_path / 'chain_check_host')
    build = ['g++', '-std=c++17'] + SAN + ['-I', 'include', '-I', 'vqnerf_release_amd/csrc', 'tests/native/chain_check_host.cpp',
                                           'vqnerf_release_amd/csrc/neus_pack_plan.cpp', 'vqnerf_release_amd/csrc/chain_pack_plan.cpp',
                                           'vqnerf_release_amd/csrc/error.cpp', '-o', exe]
    _run(build, exe, tmp_path)                                   # builds; runs once without the packer's descriptors
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=ROOT, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout
    print(out.strip())
    m = re.search(r'chain descriptor rules ok: (\d+) descriptors accepted, (\d+) refusals checked', out)
    assert m, out
    # 4 planned in C + the base program under both rules + 8 from the packer + the engine-difference cases f32 takes; 36 one-field
    # refusals under both rules + the 7 engine-difference cases f16s refuses + the one f32 refuses
    assert (int(m.group(1)), int(m.group(2))) == (4 + 2 + 8 + 6, 2 * 36 + 7 + 1)
