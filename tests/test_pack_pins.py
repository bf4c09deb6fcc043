"""CPU: every weight-independent pack product that reaches a kernel -- gather indices and descriptors of the training engines --
pinned by SHA-256.

The constants below were taken from the code of the commit BEFORE the engine-layout table (`geo.packing.EngineLayout`) and the one
flat-gather builder (`GatherPack`) replaced the per-engine copies of the layout rules; they are not regenerated from the code under
test.  A digest covers dtype, shape and the bytes of the contiguous array, so any reordering, retyping or off-by-one of an index or a
descriptor word shows."""
import hashlib

import numpy as np
import pytest
import torch

from tests.decomp_util import make_config

CPU = torch.device('cpu')


def _digest(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a))
    return hashlib.sha256(('%s%s' % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def _neus_engine(which):
    from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork
    from vqnerf_release_amd.geo.train_programs import NeusTrainEngine
    # 'skip160': the smallest shape the fused backward accepts with a skip layer; 'full': the 8 x 256 / 4 x 256 nets; 'small': interpreted
    hid, n_s, skip, n_c = {'skip160': (160, 3, (2,), 2), 'full': (256, 8, (4,), 4), 'small': (64, 4, (2,), 2)}[which]
    sdf = SDFNetwork(d_in=3, d_out=hid + 1, d_hidden=hid, n_layers=n_s, skip_in=skip, multires=6, bias=0.5, scale=1.5,
                     geometric_init=True, weight_norm=True)
    col = RenderingNetwork(d_feature=hid, mode='idr', d_in=9, d_out=3, d_hidden=hid, n_layers=n_c, weight_norm=True, multires_view=4,
                           squeeze_out=True)
    return NeusTrainEngine(sdf, col)


def _bwd_f32(which):
    e = _neus_engine(which)
    assert e._fused_backward_shape() and e.skip > 0
    gidx, desc = e._bwd_static(CPU)
    return [gidx, desc]


def _bwd_x3(which):
    e = _neus_engine(which)
    assert e._fused_backward_shape() and e.skip > 0
    # (one builder parameterised by the engine's layout replaces the two per-engine ones)
    gidx, n_steps, fidx, desc = e._bwd_static_x3(CPU) if hasattr(e, '_bwd_static_x3') else e._bwd_static(CPU, 'x3')
    return [gidx, np.int64(n_steps), fidx, desc]


def _fused_fwd(which):
    gi_s, d_s, gi_c, d_c = _neus_engine(which)._fused_static(CPU)
    return [gi_s, d_s, gi_c, d_c]


def _programs(static):
    L, gidx, descs = static
    return [gidx, np.int64(L.size)] + [descs[n][0] for n in sorted(descs)]


def _neus_programs():
    e = _neus_engine('small')
    assert not e.fused_forward() and not e.fused_backward()
    return _programs(e._static(CPU))


def _refl(which):
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.refl_train import ReflStackEngine
    if which in ('zx', 'no_zx'):                               # the stage-3 stack of tests/test_decomp_host.py, with and without the second input
        m = get_model_class('ref_nfr')(make_config(model='ref_nfr'))
        m.build_nets(device='cpu', seed=1)
        eng = ReflStackEngine([m.net['rgb_enc']], 0, [m.net['diff_out'], m.net['rough_out']], m.z_dim, 'cpu', zx=which == 'zx')
    else:                                                      # stage 2: encoder with its skip-concat + three heads ('A'), heads alone ('B')
        m = get_model_class('vq_nfr')(make_config())
        m.build_nets(device='cpu', seed=1)
        if which == 'A':
            eng = ReflStackEngine([m.net['fine_enc'], m.net['bottleneck']], m.embedder['xyz'].n_freqs,
                                  [m.net[n] for n in ('diff_main', 'spec_main', 'rough_main')], m.z_dim, 'cpu')
        else:
            eng = ReflStackEngine(None, 0, [m.net[n] for n in ('diff_vq', 'spec_vq', 'rough_vq')], m.z_dim, 'cpu')
    L, gidx, n_steps, fidx, d = eng._static()
    return [gidx, np.int64(n_steps), fidx, d, np.int64(L.size)]


def _decomp_programs(which):
    from vqnerf_release_amd.decomp.nerfactor.models import get_model_class
    from vqnerf_release_amd.decomp.train_programs import EncoderEngine, HeadsEngine
    m = get_model_class('vq_nfr')(make_config())
    m.build_nets(device='cpu', seed=1)
    if which == 'enc':
        eng = EncoderEngine(m.net['fine_enc'], m.net['bottleneck'], m.embedder['xyz'].n_freqs, 'cpu')
    else:
        eng = HeadsEngine([m.net[n] for n in ('diff_main', 'spec_main', 'rough_main')], m.z_dim, 'cpu')
    return _programs(eng._static(['prog_fwd', 'prog_bwd']))


CASES = {
    'neus_bwd_f32_skip160': lambda: _bwd_f32('skip160'),
    'neus_bwd_x3_skip160': lambda: _bwd_x3('skip160'),
    'neus_bwd_f32_full': lambda: _bwd_f32('full'),
    'neus_bwd_x3_full': lambda: _bwd_x3('full'),
    'neus_fused_fwd_skip160': lambda: _fused_fwd('skip160'),
    'neus_programs_small': _neus_programs,
    'refl_zx': lambda: _refl('zx'),
    'refl_no_zx': lambda: _refl('no_zx'),
    'refl_stage2_enc_heads': lambda: _refl('A'),
    'refl_stage2_heads': lambda: _refl('B'),
    'decomp_programs_encoder': lambda: _decomp_programs('enc'),
    'decomp_programs_heads': lambda: _decomp_programs('heads'),
}

PINS = {
    'neus_bwd_f32_skip160': ['893ae4809709c808fc52f86b340d311259fc868c16928d05f751f6cf8e8232ee',
        '94623b38dd2ecf1ca6869a5a24e6074010f20d20b977f5c6e0e16bbcf7b9d53a'],
    'neus_bwd_x3_skip160': ['0f535d3c87d5f2d6ec78c0b72af6d6a59aca7aa6d70ca9caeda7e03c21b6823c',
        '6bb81cd279cce8330ecbd2c27e638c8e2b798980a8986ca5251efcff9d2758c7',
        'c0156cb3cf74832452534860b2653349472803dc7f15211809f00f034b2f2b59',
        '075fa661b4618cc4a5122478ad57601278091e32cd2d0e218a8319c00ee258bd'],
    'neus_bwd_f32_full': ['1ea3855a23b64ef859ae72214efac2e69de1d9ee10ccd48c58a88926e4e221ff',
        '08bd98ef601c08153d94a570293b27624f3d8e5e9a8c9d077459feb98955b960'],
    'neus_bwd_x3_full': ['a4d845dee80920bff63f6d1d7f3fdd8bb9e4cceb68f4c521d4ca9706df0074c1',
        'bcce97070d794c14286ab3d4cc19e0aeba02e16707050968eea54a0a63677041',
        '0d169976c05065e5cf420ed92676ce9ba29fd8ca4a3de2503edd12adeb6edc7f',
        '5a9a378b1fcbe322e5d450ff2374f4b208535bd58b44034292634219c9153f6c'],
    'neus_fused_fwd_skip160': ['6e8fbdef7a2426d3c9a968328098d6cc28b069cb71e79a61798e53558b74b178',
        'b1a006922af23c09ca1e9d01cada5c89e800a8c9b0a85467f5f412f7206c18d0',
        'e52523a3215ef1fb40d432a8c00fa65888c166bb8e4ea0298ce38d86e4f16bb0',
        '61b1f524bef879096420171cc4dbaafd307f59d821d4339d0f1dda4cc98ff320'],
    'neus_programs_small': ['2e361c1695a90c65d09440c5f924867a213968f322c8c9b419641895adc2403c',
        'c95d79ebadc3d4910c333bbd9885632b697688d94978c47e9a847b694b8ce5a6',
        '730aed4869f03c271ad877ac67aeb07dcf54e01eead43cf9b82efac19db66b4b',
        'fb34ad7dd4a2f790f29a9e499bd9531aababb7e53c6a3647c01e40afee1bba41',
        '67f3824f1290ae4b6a97e52f156f5fa91a4ff7f2d2c32c5339f88f6ca4d9467c'],
    'refl_zx': ['2215e41dbc3a3f6b9023d404877d0acdacfa301bc4227ca3ca6f8b5e1c0763da',
        '0c189e881779db79ada9d4ec108d7e80bdf7b32d5ccf1f63a21253dc2ace0ab6',
        '4caa8bd6cf07c54eed76232879c7ada3cc86f5484be5d786c1b1fb3c5f37861b',
        'c9a3f817b86abe186211c4f49745cf392b2fac120ad11d8c49b20ce9f4cb9ba2',
        '73a00bcfd64ec0448c78d6f7a30b13d1c7465c1006e08dde2f5b170af214a512'],
    'refl_no_zx': ['a823537e433faabd245172596d22574168ab319a0719b4f4b23b3c31b4247ebe',
        '796360dbf3b54481ba145f7be239006ffa5512e61198b8516d4b57de1a3fd7a9',
        '647088ba6e30333c4a4fde69a56c288411cace412b4922a0021c6a3f4975708c',
        'ac34e81ca3efbc4bad4d0710fba04dddd1a705c828151d5dc93954eeb1a7fdad',
        '133ea53470518a413f137805c6de5d522db7b8c2a66b900de50876f7d8f7fdaa'],
    'refl_stage2_enc_heads': ['4110bf33fdb28ca8f0add15beee06e383d7dccfab95be2dbb78117027b6edde8',
        '10b51bd446b8b0fabf0108fd16db5c54d66d34973ef1bc73643e6b1516cd5119',
        'a743305b6a00809fcb99a5ff716e9811561680e516baf71b08bd1c1fee2edf90',
        'de60e76af47bdf879433426bd97cb08ac275cef37a290c541e08d44b31160e71',
        'd28698434d06bf2d261a3e98248a332903358e332d267ea046eac2c605ac5604'],
    'refl_stage2_heads': ['d47348f8f4bc33438f84c833e88935faf9b0c17e92b69057d82ab696e2eb31e3',
        '7ba265fcd2ae828c503de58bbd723b6a3c58a792db97b0f29010007bef32a9d1',
        '32d8b261adc3355803179239502a1bc14b4b499db183161756139bfe4960cc71',
        'c03f21b15cf6951d6e0dbc4cd500c0525ac883b4a15fbedc182c1e0d72c9e66d',
        '79e13c72882ccced2c71496c8509b670e3f0a67f5d31831c5ebcc48b66070d7e'],
    'decomp_programs_encoder': ['87966d0436fc84976573d2eb91ca31699ec2092df20241806c61b527d8f9f23b',
        '75885407e26767f90380ef22092abff145cc63fee489edcdec22bc2cbb47f788',
        '3642349f007bfbeedfe8f68791fd9c3d1353fc007a6fb6ba54524274968d3615',
        '41f4fd52eb388d686eaa022ec7dcd7d7be056ae6851639c37489df9c654fadbf'],
    'decomp_programs_heads': ['e86b03b973de12e1d17e599facfd30117923d6e26955292a800b82a4bd7fb9d1',
        'ab562fc6191d589d235adf46f4049e0cd7ed0912b77a4c91f2023201bfd513e2',
        '46fd73f25bf933304ebafe4351de563b992d8f6e4b58e9b699f847c80f014fe4',
        '260a9b4261ee2c6b89ec5b9149d0916e0e6c1a66ec4156108903ffa5117ea117'],
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_static_pack_products_are_those_of_the_per_engine_builders(name):
    got = [_digest(a) for a in CASES[name]()]
    assert got == PINS[name], name
