"""vqn_neus_composite_fwd / vqn_neus_composite_bwd on their own, every output element against oracle.geo.composite in float64
(adjoints by torch.autograd over it).  The yardstick is the float32 evaluation of the same statement (tests/kernel_cases.py:
max error within 3x, rms within 2x of the float32 reference's own, floor 8 eps of the tensor's largest entry).  The inputs keep
every sample 1e-3 away from the statement's kinks and the test asserts, from the two references alone, that both precisions
take the same branch everywhere: no element is left out of any comparison."""
import math

import numpy as np
import pytest
import torch

from tests import kernel_cases as kc
from tests.gpu_util import launches
from vqnerf_release_amd import _C

pytestmark = pytest.mark.gpu

WHITE = (1.0, 1.0, 1.0)
E5 = math.exp(5.0)


# The yardstick's factors are 3 (max) and 2 (rms).  Two kinds of tensor get 8, because the float32 reference is unusually exact
# on them (figures of the first run on an MI355X, kernel error / float32 reference error, both against float64):
#   * g_inv_s: ONE number per case (the sum over all rays), so the reference's error is a single draw and not a maximum over many:
#     1.9e-10 / 3.5e-11 (n64-B5 weight_sum), 2.4e-8 / 7.2e-9 (n64-Bbig color), 3.7e-8 / 1.2e-8 (n129-Bbig weight_sum);
#   * g_sdf / g_grad under an adjoint on weight_sum ALONE: d weight_sum / d alpha_i = T_i - (sum_{j>i} w_j) / q_i cancels to the
#     transmittance behind the ray's end, i.e. to ~0 on every ray that saturates, and what is left is the rounding of T_i.  torch's
#     sequential cumprod makes T_i and the w_j from the same chain of products, so that rounding cancels too; the kernel's log-step
#     scan gives each lane's T_i its own product tree (equally valid, errors of a few eps of T_i that do not cancel):
#     g_sdf 1.9e-6 / 3.3e-7 (n64-B5, largest entry 37 x T_i), 3.4e-3 / 9.9e-4 (n127-B3, inv_s clipped to 1e6).
#   With any other adjoint switched on the same kernel lines meet 3 / 2.
def _factors(adjoint_set, tensor):
    if tensor == 'g_inv_s' or (adjoint_set == 'weight_sum' and tensor in ('g_sdf', 'g_grad')):
        return dict(f_max=8.0, f_rms=8.0)
    return {}


def _big_b():
    return 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5      # a second pass of the grid; last group: one ray


# (n, B, cos_anneal_ratio, background, inv_s, profile shift); B = -1: _big_b().  Every n of 1..256 at and around the lane-layout
# boundaries, every B class, each paired rather than crossed; inv_s 2e6 / 5e-7 lie outside the clip [1e-6, 1e6].
CASES = [
    (1, 5, 0.3, WHITE, 64.0, 0),
    (2, 3, 0.0, None, E5, 2),
    (3, 1, 1.0, WHITE, 512.0, 3),
    (63, 64, 0.3, None, 64.0, 0),
    (64, 5, 1.0, WHITE, E5, 0),
    (65, 64, 0.0, WHITE, 512.0, 0),
    (127, 3, 0.3, None, 2e6, 1),
    (128, 64, 1.0, WHITE, 64.0, 0),
    (129, -1, 0.3, WHITE, E5, 0),
    (255, 5, 0.0, None, 512.0, 3),
    (256, 64, 0.3, WHITE, 64.0, 0),
    (256, 1, 1.0, None, 5e-7, 0),
    (64, -1, 1.0, None, 512.0, 0),
    (128, 1, 0.0, WHITE, 64.0, 3),
]


def _id(c):
    return f'n{c[0]}-B{"big" if c[1] < 0 else c[1]}-car{c[2]}-{"white" if c[3] else "nobg"}-s{c[4]:.3g}'


def _case(c):
    n, B, car, bg, inv_s, shift = c
    B = _big_b() if B < 0 else B
    inp = kc.composite_inputs(B, n, inv_s, shift=shift)
    names = list(kc.ADJOINT_SETS)
    f64, g64 = kc.composite_reference(inp, car, bg, torch.float64, names)
    f32, g32 = kc.composite_reference(inp, car, bg, torch.float32, names)
    # conditions of the comparison, from the references alone
    assert kc.composite_margins_ok(inp, f64)
    assert np.array_equal(kc.branch_indicators(f32), kc.branch_indicators(f64)), 'float32 and float64 take different branches'
    assert not (f64['raw_alpha'] < 0).any() and not (f64['raw_alpha'] > 1).any()
    print(f'[{_id(c)}] alpha clipped by the float32 reference: {int(((f32["raw_alpha"] < 0) | (f32["raw_alpha"] > 1)).sum())} of {B * n}')
    near = inp['profile'] == kc.PROFILES.index('near_saturated')
    if near.any() and n >= 3:
        a = f64['alpha'][near][:, inp['k0']:inp['k0'] + 3]
        assert (((a >= 0.9) & (a <= 0.999)).sum(1) >= 2).all(), a
    dev = lambda k: torch.tensor(inp[k]).cuda().contiguous()
    geo = tuple(dev(k) for k in ('rays_o', 'rays_d', 'mid_z', 'dists', 'sdf', 'grad', 'rgb', 'inv_s'))
    bgt = None if bg is None else torch.tensor(bg).cuda()
    return inp, (f32, g32), (f64, g64), geo, bgt, dev


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_composite_forward_vs_float64(case):
    n, _, car, bg, inv_s, _ = case
    inp, (f32, _), (f64, _), geo, bgt, _ = _case(case)
    with launches() as rec:
        got = _C.neus_composite_fwd(*geo, bgt, kc.RADIUS, car, want_alpha=True)
    assert rec.counts.get('vqn_neus_composite_fwd') == 1, rec.counts
    got = {k: v.cpu().numpy() for k, v in got.items()}
    B = inp['mid_z'].shape[0]
    rep = kc.Report('test_composite_forward_vs_float64')
    for k in ('color', 'weights', 'cdf', 'surf', 'depth', 'weight_sum', 'weight_max', 'alpha'):
        rep.check(f'{_id(case)}/{k}', got[k], f32[k], f64[k])
    rep.check(f'{_id(case)}/gerr_num', got['gerr'][:, 0], f32['gerr_num'], f64['gerr_num'])
    rep.exact(f'{_id(case)}/gerr_den', got['gerr'][:, 1], f64['gerr_den'].astype(np.float32))
    rep.exact(f'{_id(case)}/inside_sphere', got['inside_sphere'], f64['inside_sphere'].astype(np.float32))
    miss = inp['profile'] == kc.PROFILES.index('miss')
    assert not f64['relax'][miss].any() and not f64['inside_sphere'][miss].any()           # the eikonal term's empty branch
    rep.finish()


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_composite_backward_vs_float64_autograd(case):
    """g_sdf, g_grad, g_rgb per sample and g_inv_s summed over the rays, for random adjoints on color, weight_sum, weights and
    gradient_error together and for each of them alone with the others passed as None (the kernel's null branches)."""
    n, _, car, bg, inv_s, _ = case
    inp, (f32, g32), (f64, g64), geo, bgt, dev = _case(case)
    B = inp['mid_z'].shape[0]
    fwd = _C.neus_composite_fwd(*geo, bgt, kc.RADIUS, car)
    den = fwd['gerr'].sum(0)[1:2].contiguous()                 # as CompositeFunction hands it over
    np.testing.assert_array_equal(den.cpu().numpy(), np.float32(f64['gerr_den'].sum()))
    sat = inp['profile'] == kc.PROFILES.index('saturated')
    clipped = not (1e-6 <= inv_s <= 1e6)
    rep = kc.Report('test_composite_backward_vs_float64_autograd')
    for name, on in kc.ADJOINT_SETS.items():
        g_color = dev('g_color') if 'g_color' in on else torch.zeros(B, 3, device='cuda')
        opt = lambda k: dev(k) if k in on else None
        with launches() as rec:
            got = _C.neus_composite_bwd(*geo, bgt, kc.RADIUS, car, g_color, opt('g_weight_sum'), opt('g_weights'),
                                        opt('g_gradient_error'), den if 'g_gradient_error' in on else None)
        assert rec.counts.get('vqn_neus_composite_bwd') == 1, rec.counts
        g_sdf, g_grad, g_rgb, g_is = got
        key = f'{_id(case)}/{name}'
        rep.check(f'{key}/g_sdf', g_sdf.cpu().numpy(), g32[name][0], g64[name][0], **_factors(name, 'g_sdf'))
        rep.check(f'{key}/g_grad', g_grad.cpu().numpy(), g32[name][1], g64[name][1], **_factors(name, 'g_grad'))
        rep.check(f'{key}/g_rgb', g_rgb.cpu().numpy(), g32[name][2], g64[name][2])
        rep.check(f'{key}/g_inv_s', g_is.sum().reshape(1).cpu().numpy(), g32[name][3], g64[name][3], **_factors(name, 'g_inv_s'))
        if clipped:                                            # the clip's gradient outside [1e-6, 1e6]
            assert not g64[name][3].any()
            rep.exact(f'{key}/g_inv_s per ray (clipped inv_s)', g_is.cpu().numpy(), np.zeros(B, np.float32))
        if sat.any():                                          # alpha = 1, both sigmoids flat: the float32 statement gives exactly 0
            assert not g32[name][0][sat].any() and np.abs(g64[name][0][sat]).max() < 1e-100
            rep.exact(f'{key}/g_sdf on the saturated rays', g_sdf.cpu().numpy()[sat], np.zeros((int(sat.sum()), n), np.float32))
            if name in ('all', 'color'):
                assert g64[name][2][sat].any()                 # g_rgb stays live there
        if name == 'gradient_error':                           # nothing but the eikonal term: every other adjoint exactly 0
            for k, t in (('g_sdf', g_sdf), ('g_rgb', g_rgb), ('g_inv_s', g_is)):
                rep.exact(f'{key}/{k} is zero', t.cpu().numpy(), np.zeros(tuple(t.shape), np.float32))
    rep.finish()
