"""vqn_brdf_shade_bwd and vqn_brdf_shade_fwd on their own at every light count (256, 512, 1024: the three template forms), one and
two material sets, with and without visibility rows: adjoints per point and per light, forward sums per point, against
oracle.decomp's statements in float64 (adjoints by torch.autograd).  Yardstick: the float32 evaluation of the same statements
(tests/kernel_cases.py).  Shading has no value discontinuity (the front-lit gate multiplies by the cosine it tests), so no element
is left out.  Every tensor is judged twice: over all points, where the glossy peaks of small roughness set the float32 reference's
error, and over the points with rough >= 0.3 in every set, where that error is at rounding level and a small wrong term shows."""
import numpy as np
import pytest
import torch

from tests import kernel_cases as kc
from tests.gpu_util import launches
from vqnerf_release_amd import _C

pytestmark = pytest.mark.gpu


def _big_n():
    return 16 * torch.cuda.get_device_properties(0).multi_processor_count + 7     # waves take several points, and not all the same number


# (L, n_sets, visibility rows, N (-1: _big_n()), edge shift)
BWD_CASES = [
    (256, 1, True, 1, 0), (256, 2, False, 3, 3), (256, 2, True, 500, 0), (256, 1, False, -1, 0),
    (512, 2, True, 5, 5), (512, 1, False, 500, 0), (512, 2, True, -1, 0), (512, 1, True, 1, 2),
    (1024, 1, False, 5, 0), (1024, 2, True, 500, 0), (1024, 2, False, 1, 6), (1024, 1, True, -1, 0), (1024, 2, False, 3, 7),
]
FWD_CASES = [c for c in BWD_CASES if c[0] != 512]


def _id(c):
    return f'L{c[0]}-sets{c[1]}-{"lvis" if c[2] else "novis"}-N{"big" if c[3] < 0 else c[3]}-e{c[4]}'


def _inputs(c):
    L, n_sets, with_lvis, N, shift = c
    N = _big_n() if N < 0 else N
    inp = kc.shade_inputs(N, L, n_sets, with_lvis, shift=shift)
    dev = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float32)).cuda().contiguous()
    geo = (dev(inp['xyz']), dev(inp['normal']), dev(inp['rayo']), dev(inp['lvis']), dev(inp['lxyz']), dev(inp['lareas']), dev(inp['light']))
    mats = [tuple(dev(m) for m in ms) for ms in inp['mats']]
    smooth = np.all([ms[2][:, 0] >= 0.3 for ms in inp['mats']], 0)
    return inp, geo, mats, dev, smooth


# The yardstick's factors are 3 (max) and 2 (rms).  The tensors that carry the GGX lobe get 8: t = cos_m^2 (a2 - 1) + 1 cancels to
# ~a2 = rough^4 on a glossy peak, one or two such points set the error of the whole tensor, max and rms alike, and the float32
# reference (IEEE division and square root) is then unusually exact next to a kernel on the 1-ulp hardware reciprocals (figures of
# the first run on an MI355X, kernel error / float32 reference error, both against float64):
#   rgb       5.5e-6 / 1.0e-6 (L1024 N3), 8.5e-5 / 1.8e-5 (L256 49 probes), 2.2e-2 / 7.1e-3 (L512 Nbig); rms 1.6e-3 / 7.8e-4 (L512 N500)
#   rgb_spec  5.5e-6 / 9.6e-7 (L1024 N3)
#   g_rough   7.7e-7 / 1.2e-7 (L512 N5); rms 2.4e-2 / 1.1e-2 (L512 N500)
#   g_light   rms 3.7e-3 / 1.8e-3 (L512 N500; max 0.14 / 0.064 is inside 3x)
# g_albedo, g_spec, rgb_diff and rgb_probes meet 3 / 2.
LOBE = ('rgb0', 'rgb1', 'rgb_spec', 'g_rough0', 'g_rough1', 'g_light')


def _factors(key):
    return dict(f_max=8.0, f_rms=8.0) if key.rsplit('/', 1)[-1] in LOBE else {}


def _check_points(rep, key, got, r32, r64, smooth):
    rep.check(key, got, r32, r64, **_factors(key))
    if smooth.any():
        rep.check(key + '[rough>=0.3]', got[smooth], r32[smooth], r64[smooth], **_factors(key))


@pytest.mark.parametrize('case', BWD_CASES, ids=_id)
def test_shade_backward_vs_float64_autograd(case):
    """g_albedo, g_spec, g_rough of every point and set and g_light of every light, loss = sum_s <g_sum_s, rgb_s> with random
    g_sum_s of both signs; and the forward's plain sums (raw = 1) the backward is the reverse of.  At N = 1 three of the
    workgroup's four waves own no point: g_light equals the reference only if they write zero partials."""
    inp, geo, mats, dev, smooth = _inputs(case)
    L, n_sets = case[0], case[1]
    r64, r32 = kc.shade_reference(inp, torch.float64), kc.shade_reference(inp, torch.float32)
    n0 = sum(int((ms[2] == 0.0).sum()) for ms in inp['mats'])
    assert kc.rough0_limit(inp, r64) <= n0 and kc.rough0_limit(inp, r32) <= n0
    g_sums = [dev(g) for g in inp['g_sums']]
    with launches() as rec:
        fwd = _C.brdf_shade_fwd(*geo, mats, want_normal=True, raw=1)
        grads, g_light = _C.brdf_shade_bwd(*geo, mats, g_sums)
    assert rec.counts.get('vqn_brdf_shade_fwd') == 1 and rec.counts.get('vqn_brdf_shade_bwd') == 1, rec.counts
    rep = kc.Report('test_shade_backward_vs_float64_autograd')
    k = _id(case)
    rep.exact(f'{k}/normal', fwd['normal'].cpu().numpy(), r32['normal'])
    for s in range(n_sets):
        _check_points(rep, f'{k}/rgb{s}', fwd['rgb'][s].cpu().numpy(), r32['rgb'][s], r64['rgb'][s], smooth)
        for j, name in enumerate(('g_albedo', 'g_spec', 'g_rough')):
            _check_points(rep, f'{k}/{name}{s}', grads[s][j].cpu().numpy(), r32['g'][s][j], r64['g'][s][j], smooth)
    rep.check(f'{k}/g_light', g_light.cpu().numpy(), r32['g_light'], r64['g_light'], **_factors(f'{k}/g_light'))
    # the edges whose adjoints are exact zeros
    E = kc.EDGES.index
    for s in range(n_sets):
        dark = (inp['edge'] == E('all_behind')) | (inp['edge'] == E('zero_gsum'))
        if inp['lvis'] is not None:
            dark |= inp['edge'] == E('lvis0')
        for j, name in enumerate(('g_albedo', 'g_spec', 'g_rough')):
            assert not r64['g'][s][j][dark].any()
            rep.exact(f'{k}/{name}{s} at the dark points', grads[s][j].cpu().numpy()[dark], np.zeros_like(r32['g'][s][j][dark]))
        r0 = inp['mats'][s][2][:, 0] == 0.0
        rep.exact(f'{k}/g_rough{s} at rough = 0', grads[s][2].cpu().numpy()[r0], np.zeros((int(r0.sum()), 1), np.float32))
    rep.finish()


@pytest.mark.parametrize('gamma', [None, (1.3, 0.8)], ids=['clip', 'gamma'])
@pytest.mark.parametrize('case', FWD_CASES, ids=_id)
def test_shade_forward_256_1024_vs_float64(case, gamma):
    """The display forward (gamma curve / [0, 1] clip inside the kernel) at 256 and 1024 lights: rgb per set, the diffuse / specular
    split of set 0, the camera-facing normal."""
    inp, geo, mats, dev, smooth = _inputs(case)
    r64 = kc.shade_reference(inp, torch.float64, grads=False, gamma=gamma, clip=True)
    r32 = kc.shade_reference(inp, torch.float32, grads=False, gamma=gamma, clip=True)
    gam = None if gamma is None else torch.tensor(gamma).cuda()
    with launches() as rec:
        got = _C.brdf_shade_fwd(*geo, mats, gamma=gam, want_normal=True, want_split=True)
    assert rec.counts.get('vqn_brdf_shade_fwd') == 1, rec.counts
    rep = kc.Report('test_shade_forward_256_1024_vs_float64')
    k = f'{_id(case)}/{"gamma" if gamma else "clip"}'
    rep.exact(f'{k}/normal', got['normal'].cpu().numpy(), r32['normal'])
    for s in range(case[1]):
        _check_points(rep, f'{k}/rgb{s}', got['rgb'][s].cpu().numpy(), r32['rgb'][s], r64['rgb'][s], smooth)
    _check_points(rep, f'{k}/rgb_diff', got['rgb_diff'].cpu().numpy(), r32['rgb_diff'], r64['rgb_diff'], smooth)
    _check_points(rep, f'{k}/rgb_spec', got['rgb_spec'].cpu().numpy(), r32['rgb_spec'], r64['rgb_spec'], smooth)
    rep.finish()


# n_probes on both sides of the probe-table-in-LDS limit n_probes * (L / 256) * 3 KB <= 144 KB; at 1024 lights two material sets
# never take the LDS form
@pytest.mark.parametrize('L,n_sets,n_probes', [(256, 1, 48), (256, 2, 49), (512, 1, 24), (512, 2, 25), (1024, 1, 12), (1024, 1, 13),
                                               (1024, 2, 12), (1024, 2, 13)])
def test_shade_relight_probes_vs_float64(L, n_sets, n_probes):
    """The relighting pass (probes=): material set 0 under every probe in one launch, against the oracle's loop of one
    render_integrate per probe; the ordinary outputs of the same launch are compared too."""
    case = (L, n_sets, True, 37, 0)
    inp, geo, mats, dev, smooth = _inputs(case)
    rng = np.random.default_rng(n_probes)
    probes = rng.uniform(0, 2, (n_probes, L, 3)).astype(np.float32)
    with launches() as rec:
        got = _C.brdf_shade_fwd(*geo, mats, want_normal=True, probes=dev(probes))
    assert rec.counts.get('vqn_brdf_shade_fwd') == 1, rec.counts
    assert tuple(got['rgb_probes'].shape) == (37, n_probes, 3)
    rep = kc.Report('test_shade_relight_probes_vs_float64')
    k = f'L{L}-sets{n_sets}-probes{n_probes}'
    r64 = kc.shade_reference(inp, torch.float64, grads=False, clip=True)
    r32 = kc.shade_reference(inp, torch.float32, grads=False, clip=True)
    for s in range(n_sets):
        _check_points(rep, f'{k}/rgb{s}', got['rgb'][s].cpu().numpy(), r32['rgb'][s], r64['rgb'][s], smooth)
    one = dict(inp, mats=inp['mats'][:1])
    p64 = np.stack([kc.shade_reference(one, torch.float64, grads=False, clip=True, light=p)['rgb'][0] for p in probes], 1)
    p32 = np.stack([kc.shade_reference(one, torch.float32, grads=False, clip=True, light=p)['rgb'][0] for p in probes], 1)
    _check_points(rep, f'{k}/rgb_probes', got['rgb_probes'].cpu().numpy(), p32, p64, smooth)
    rep.finish()


@pytest.mark.parametrize('L', [256, 512, 1024])
def test_shade_backward_without_points(L):
    """A training batch without a foreground point: the forward accepts N = 0, so the backward must too -- empty per-point
    adjoints and a zero g_light -- and ShadeFunction must differentiate through it."""
    from vqnerf_release_amd.decomp.nerfactor.models.nfr_unit import ShadeFunction
    inp, geo, mats, dev, _ = _inputs((L, 1, True, 4, 0))
    e = lambda *s: torch.empty(s, device='cuda')
    geo0 = (e(0, 3), e(0, 3), e(0, 3), e(0, L)) + geo[4:]
    grads, g_light = _C.brdf_shade_bwd(*geo0, [(e(0, 3), e(0, 3), e(0, 1))], [e(0, 3)])
    assert tuple(grads[0][0].shape) == (0, 3) and tuple(grads[0][2].shape) == (0, 1)
    np.testing.assert_array_equal(g_light.cpu().numpy(), np.zeros((L, 3), np.float32))
    light = geo[6].clone().requires_grad_(True)
    a, s, r = (t.requires_grad_(True) for t in (e(0, 3), e(0, 3), e(0, 1)))
    normal, rgb = ShadeFunction.apply(geo0[:6], light, a, s, r)
    assert tuple(rgb.shape) == (0, 3)
    (rgb.sum() + 0.0 * light.sum()).backward()
    np.testing.assert_array_equal(light.grad.cpu().numpy(), np.zeros((L, 3), np.float32))
    assert tuple(a.grad.shape) == (0, 3)
