"""The per-ray sampling kernels at their declared limits (n <= 256 samples, n_new <= 64, any ray count): vqn_neus_merge and
vqn_neus_section_mids exactly, vqn_neus_upsample against oracle.geo.up_sample in float64."""
import numpy as np
import pytest
import torch

from tests import kernel_cases as kc
from tests.gpu_util import launches, record_observed
from vqnerf_release_amd import _C

pytestmark = pytest.mark.gpu


def _big_b(extra):
    return 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + extra     # beyond one pass of the grid, ragged last group


def _b(B, extra=3):
    return _big_b(extra) if B < 0 else B


@pytest.mark.parametrize('n,m,B', [(1, 1, 1), (1, 64, 5), (63, 16, 5), (64, 63, -1), (65, 64, 5), (192, 16, 1), (256, 64, -1), (256, 1, 5),
                                   (64, 64, 1), (192, 63, 5)])
def test_merge_is_the_stable_sort(n, m, B):
    z, sdf, z_new, sdf_new = kc.merge_inputs(_b(B), n, m)
    want_z, want_sdf = kc.merge_reference(z, sdf, z_new, sdf_new)
    if n + m > 8:
        assert (np.diff(want_z, axis=1) == 0).any()              # the case does hold equal depths
    c = lambda a: torch.tensor(a).cuda()
    with launches() as rec:
        got_z, got_sdf = _C.neus_merge(c(z), c(sdf), c(z_new), c(sdf_new))
        only_z, none = _C.neus_merge(c(z), None, c(z_new), None)
    assert rec.counts.get('vqn_neus_merge') == 2 and none is None, rec.counts
    np.testing.assert_array_equal(got_z.cpu().numpy(), want_z)
    np.testing.assert_array_equal(got_sdf.cpu().numpy(), want_sdf)
    np.testing.assert_array_equal(only_z.cpu().numpy(), want_z)


@pytest.mark.parametrize('n,m,inv_s', kc.UPSAMPLE_GRID)
def test_upsample_vs_float64(n, m, inv_s):
    """Every new depth within the project's 2e-5 of the float64 oracle on the rays where the float32 and float64 oracles agree to
    1e-5 themselves; the others (at most one of the eight profiles) are reported and left out."""
    c = kc.upsample_case(n, m, inv_s)
    left_out = np.flatnonzero(~c['agree'])
    assert (~c['agree'][:8]).sum() <= 1, left_out
    if len(left_out):
        print(f'[upsample n{n} m{m} s{inv_s:g}] rays left out (the oracles disagree): {left_out.tolist()}')
    g = lambda a: torch.tensor(a).cuda()
    u = torch.linspace(0.5 / m, 1.0 - 0.5 / m, m, dtype=torch.float32).cuda()          # the oracle's own u (sample_pdf_det), made on the CPU
    with launches() as rec:
        got = _C.neus_upsample(g(c['o']), g(c['d']), g(c['z']), g(c['sdf']), kc.UPSAMPLE_R_LIMIT, inv_s, u)
    assert rec.counts.get('vqn_neus_upsample') == 1, rec.counts
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[8:], got[:5])            # the repeated rays of the ragged last groups
    err = np.abs(got.astype(np.float64) - c['ref64'])[c['agree']]
    record_observed('test_upsample_vs_float64', f'n{n}-m{m}-s{inv_s:g}', err.max(), 2e-5)
    assert err.max() <= 2e-5, (err.max(), np.abs(c['ref32'] - c['ref64'])[c['agree']].max())


@pytest.mark.parametrize('n,B', [(1, 1), (1, 7), (2, 5), (64, 13), (256, -1)])
@pytest.mark.parametrize('per_ray', [False, True])
def test_section_mids_exact(n, B, per_ray):
    B = _b(B)
    rng = np.random.default_rng(n + B)
    z = torch.tensor(np.sort(rng.uniform(2.0, 6.0, (B, n)), 1).astype(np.float32))
    sd = torch.tensor(rng.uniform(0.01, 0.1, (B, 1)).astype(np.float32))
    tail = sd if per_ray else torch.full((B, 1), 0.03125)
    dists = torch.cat([z[:, 1:] - z[:, :-1], tail], -1)
    mid = z + dists * 0.5
    with launches() as rec:
        got_mid, got_d = _C.neus_section_mids(z.cuda(), 0.03125, sd.cuda() if per_ray else None)
    assert rec.counts.get('vqn_neus_section_mids') == 1, rec.counts
    np.testing.assert_array_equal(got_d.cpu().numpy(), dists.numpy())
    np.testing.assert_array_equal(got_mid.cpu().numpy(), mid.numpy())
