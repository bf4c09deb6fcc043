"""The host side of vqn_neus_train_bwd and vqn_neus_train_bwd_x3 (csrc/neus_launch.h: train_bwd_args; the engines' own descriptor
rules in csrc/neus_train_bwd.hip and csrc/neus_train_bwd_x3.hip) without a device: every refusal comes back with its return code,
under the name of the entry point that was called, before anything touches the GPU.

EVERY call of the two entry points below carries exactly one defect, so none of them launches: the pointers are dummies."""
import ctypes

import numpy as np
import pytest

from vqnerf_release_amd import _C

TB_MAX_L = 12
EARG, ESHAPE = -1, -2
ENTRIES = ('vqn_neus_train_bwd', 'vqn_neus_train_bwd_x3')
DESC_MSG = {'vqn_neus_train_bwd': 'unsupported shape: invalid backward descriptor',
            'vqn_neus_train_bwd_x3': 'unsupported shape: invalid backward descriptor for the x3 engine (layers of at most 256 outputs)'}

_DUMMY = ctypes.create_string_buffer(64)
PTR = ctypes.addressof(_DUMMY)                # non-null, never dereferenced: every call is refused first


def make_desc(nL=3, nC=2, skip=1, emb_rows=6, emb_feats=27, e_tiles=2, max_tiles=5, feat_tiles=5, outf_tiles=6, squeeze=1, scale=1.0,
              ts=None, tc=None):
    """The 76 int32 words of TrainBwdDesc.  The defaults are a descriptor BOTH engines take: 27 embedding features are 6 rows of the
    x3 image (3 per 16 features) and 6 of the f32 image (at most 8 features per row, e_tiles * 4 >= rows), 5 tiles everywhere."""
    d = np.zeros(16 + 5 * TB_MAX_L, np.int32)
    d[0:10] = [nL, nC, skip, emb_rows, emb_feats, e_tiles, max_tiles, feat_tiles, outf_tiles, squeeze]
    d[14] = np.float32(scale).view(np.int32)
    d[15] = np.float32(1.0 / scale if scale else 0.0).view(np.int32)
    n_ts, n_tc = min(max(nL, 0), TB_MAX_L), min(max(nC, 0), TB_MAX_L)
    d[16:16 + n_ts] = ts if ts is not None else [min(max_tiles, 5)] * n_ts
    d[16 + TB_MAX_L:16 + TB_MAX_L + n_tc] = tc if tc is not None else [min(max_tiles, 3)] * n_tc
    return d


def query(entry, desc):
    return getattr(_C.lib(), entry + '_scratch_bytes')(None if desc is None else desc.ctypes.data)


def per_workgroup(desc):
    """two images of S_0..S_{nL-1} and g_feat, 4 max_tiles KB each"""
    return 2 * (int(desc[0]) + 1) * 4 * int(desc[6]) * 1024


def call(entry, desc, P=1, rgb=PTR, scratch_bytes=None, n_saved=None, n_outs=None, desc_ptr=True):
    """-> (return code, message).  Defaults: everything as the descriptor asks, scratch for one workgroup."""
    nL, nC = int(desc[0]), int(desc[1])
    n_saved = 2 * nL + nC if n_saved is None else n_saved
    n_outs = (nC + 1) + 2 + 2 * nL if n_outs is None else n_outs
    saved = (ctypes.c_void_p * max(n_saved, 1))(*[PTR] * n_saved)
    outs = (ctypes.c_void_p * max(n_outs, 1))(*[PTR] * n_outs)
    scratch_bytes = per_workgroup(desc) if scratch_bytes is None else scratch_bytes
    weights = (PTR, PTR) if entry.endswith('_x3') else (PTR,)
    lib = _C.lib()
    rc = getattr(lib, entry)(desc.ctypes.data if desc_ptr else None, *weights, PTR, PTR, rgb, PTR, PTR, P, PTR, scratch_bytes, saved, n_saved,
                             outs, n_outs, None)
    return rc, lib.vqn_last_error().decode()


def assert_refused(entry, rc, msg, want_rc, want_text):
    assert rc == want_rc and msg.startswith(entry + ': ') and want_text in msg, (entry, rc, msg)


# every case: the descriptor is refused by both engines, whatever else is right
SHARED_DESC_RULES = {
    'nL<2': dict(nL=1, skip=1),
    'nL=TB_MAX_L': dict(nL=TB_MAX_L, skip=1),
    'nC<1': dict(nC=0),
    'skip=0': dict(skip=0),
    'skip=nL': dict(skip=3),
    'feat_tiles>max_tiles': dict(feat_tiles=6, outf_tiles=7),
    'outf_tiles<feat_tiles': dict(outf_tiles=4),
    'ts[l]=0': dict(ts=[5, 0, 5]),
    'tc[l]>max_tiles': dict(tc=[3, 6]),
    'scale=0': dict(scale=0.0),
    'scale<0': dict(scale=-1.0),
    'max_tiles=9': dict(max_tiles=9),
}


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('rule', sorted(SHARED_DESC_RULES))
def test_descriptor_rules_both_engines_share(entry, rule):
    desc = make_desc(**SHARED_DESC_RULES[rule])
    assert query(entry, desc) == -1
    rc, msg = call(entry, desc, scratch_bytes=1 << 40)
    assert_refused(entry, rc, msg, ESHAPE, DESC_MSG[entry])
    assert msg == f'{entry}: {DESC_MSG[entry]}'


def test_the_valid_descriptor_asks_both_engines_for_the_same_scratch():
    desc = make_desc()
    need = [query(e, desc) for e in ENTRIES]
    assert need[0] == need[1] > 0
    assert need[0] % per_workgroup(desc) == 0              # a whole number of workgroups (one per CU)
    assert query(ENTRIES[0], None) == -1 and query(ENTRIES[1], None) == -1


def test_four_tiles_are_the_x3_engine_s_alone():
    desc = make_desc(max_tiles=4, feat_tiles=4, outf_tiles=5)
    f32, x3 = ENTRIES
    assert query(f32, desc) == -1
    rc, msg = call(f32, desc)
    assert_refused(f32, rc, msg, ESHAPE, DESC_MSG[f32])
    assert query(x3, desc) > 0 and query(x3, desc) % per_workgroup(desc) == 0
    # ... and its entry point takes the descriptor: it gets as far as the scratch check (one byte short, so nothing is launched)
    rc, msg = call(x3, desc, scratch_bytes=per_workgroup(desc) - 1)
    assert_refused(x3, rc, msg, EARG, 'scratch too small')


def test_each_engine_checks_the_embedding_rows_by_its_own_image():
    f32, x3 = ENTRIES
    desc = make_desc(emb_rows=5, emb_feats=39)             # 39 features: 5 rows of the f32 image, 9 of the x3 image
    assert query(f32, desc) > 0 and query(x3, desc) == -1
    desc = make_desc(emb_rows=9, emb_feats=39)
    assert query(f32, desc) == -1 and query(x3, desc) > 0


@pytest.mark.parametrize('entry', ENTRIES)
def test_argument_refusals_name_the_entry_point(entry):
    desc = make_desc()
    nL, nC = 3, 2
    rc, msg = call(entry, desc, desc_ptr=False)
    assert_refused(entry, rc, msg, EARG, 'null pointer')
    rc, msg = call(entry, desc, P=0)
    assert_refused(entry, rc, msg, EARG, 'P >= 1')
    for n in (2 * nL + nC - 1, 2 * nL + nC + 1):
        rc, msg = call(entry, desc, n_saved=n)
        assert_refused(entry, rc, msg, EARG, 'saved: [U_1..U_nL, GH_0..GH_{nL-1}, C_1..C_nC]')
    for n in (nC + 3 + 2 * nL - 1, nC + 3 + 2 * nL + 1):
        rc, msg = call(entry, desc, n_outs=n)
        assert_refused(entry, rc, msg, EARG, 'outs: [DC_0..DC_nC, GOUTF, ED, UD_1..UD_nL, AB_0..AB_{nL-1}]')
    # rgb exactly when the colour net ends in a sigmoid
    rc, msg = call(entry, desc, rgb=None)
    assert_refused(entry, rc, msg, EARG, 'rgb: ')
    rc, msg = call(entry, make_desc(squeeze=0), rgb=PTR)
    assert_refused(entry, rc, msg, EARG, 'rgb: ')


@pytest.mark.parametrize('entry', ENTRIES)
def test_scratch_short_of_one_workgroup_is_refused_before_the_device_is_touched(entry):
    """(behind hipFuncSetAttribute this check used to answer with a HIP error on a machine without a device)"""
    desc = make_desc()
    for short in (per_workgroup(desc) - 1, 0):
        rc, msg = call(entry, desc, scratch_bytes=short)
        assert rc == EARG and msg == f'{entry}: bad argument: scratch too small (see {entry}_scratch_bytes)', (rc, msg)
