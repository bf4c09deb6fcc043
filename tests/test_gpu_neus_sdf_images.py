"""GPU: the three- and four-image forms of the SDF-only NeuS kernel (neus_pointsN_kernel, csrc/neus_mlp.hip) against the two-image form,
bit for bit: same per-point arithmetic in the same order, so every output must be the same float.

The form is chosen once per process (VQN_NEUS_SDF_IMAGES), so every setting runs in a child process of its own -- this file, run as a
script, is the child: it evaluates every case below and leaves the outputs in an .npz.  The four children (unset, 2, 3, 4) are started
together on first use and shared by all tests.

Cases.  Nets: the shipped shape (8 x 256, skip 4, multires 6, weight_norm, geometric init, bias 0.85: max_tiles 8, four images fit) and a
160-wide one (max_tiles 5, the narrowest the forms take).  Point counts around every tile (32) and group (64 / 96 / 128) boundary, and
32 * 4 * 7 + 5 (a ragged last group): direct points and rays with S = 1 at exactly those counts; rays with S = 16 / 64 at ceil(P / S) rays
for each count (P = rays * S); and one count (P_BIG) at which every workgroup of a 256-CU device walks more than one group, so that what
an iteration leaves in LDS meets the next one.  The two-image form itself is held to
the oracle by test_gpu_neus_mlp.py.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_LIST = [1, 31, 32, 33, 95, 96, 97, 127, 128, 129, 383, 385, 32 * 4 * 7 + 5]
NETS = {'shipped': 256, 'w160': 160}
FALLBACK_NET, FALLBACK_P = ('w128', 128), [1, 33, 129, 32 * 4 * 7 + 5]          # max_tiles = 4: below what the forms take
P_BIG = 2 * 256 * 4 * 32 + 5 * 32 + 7       # two groups of four tiles for each of 256 workgroups and a ragged tail: the loop over groups runs twice
SETTINGS = ['default', '2', '3', '4']


def _ray_counts(S):
    return sorted({(P + S - 1) // S for P in P_LIST})


def _case_keys(net):
    keys = [f'{net}/pts/{P}' for P in P_LIST] + [f'{net}/ray1/{P}' for P in P_LIST]
    keys += [f'{net}/ray{S}/{B}' for S in (16, 64) for B in _ray_counts(S)]
    return keys + [f'{net}/pts/{P_BIG}']


# ---------------------------------------------------------------------------------------------------------------------------------------
# the child: every case under this process's setting -> npz

def _cfg(width):
    from oracle import geo as og
    cfg = {k: dict(v) for k, v in og.FULL_CFG.items()}
    cfg['sdf'].update(d_hidden=width, d_out=width + 1, bias=0.85)
    return cfg


def _pack(width):
    import torch  # noqa: F401
    from oracle import geo as og
    from vqnerf_release_amd.geo import packing as pk
    cfg = _cfg(width)
    c = cfg['sdf']
    p = og.to_torch(og.make_sdf_params(cfg, 0))
    sp = pk.SdfPackPlan(og.sdf_dims(cfg), c['skip_in'], c['multires'], c['scale'], max_tiles=(width + 31) // 32)
    assert sp.max_tiles == (width + 31) // 32
    Ws = [og.wn_weight(p, l).cuda() for l in range(sp.n_lin)]
    bs = [p[f'lin{l}.bias'].cuda() for l in range(sp.n_lin)]
    wb, desc = sp.pack(Ws, bs)
    return desc, wb


def _rays(B, S, seed):
    import torch
    from oracle import geo as og
    o, d, near, far = map(torch.tensor, og.make_rays(B, seed))
    z = near + (far - near) * torch.linspace(0, 1, S)[None, :]
    return o.cuda(), d.contiguous().cuda(), z.contiguous().cuda()


def _shell_points(n_img, seed):
    """32 * n_img * 3 points, radius 0.1 and 1.9 alternating per tile of 32: neighbouring images hold very different activations"""
    rng = np.random.default_rng(seed)
    n = 32 * n_img * 3
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = np.where((np.arange(n) // 32) % 2 == 0, 0.1, 1.9)[:, None]
    return (v * r).astype(np.float32)


def _child(out_path):
    import torch
    from vqnerf_release_amd import _C
    out = {}
    for net, width in list(NETS.items()) + [FALLBACK_NET]:
        desc, wb = _pack(width)
        fallback = net == FALLBACK_NET[0]
        rng = np.random.default_rng(11)
        for P in (FALLBACK_P if fallback else P_LIST + [P_BIG]):
            pts = torch.tensor(rng.uniform(-1.2, 1.2, (P, 3)).astype(np.float32)).cuda()
            out[f'{net}/pts/{P}'] = _C.neus_sdf_points(desc, wb, pts=pts)
            if not fallback:
                o, d, z = _rays(P, 1, 2)
                out[f'{net}/ray1/{P}'] = _C.neus_sdf_points(desc, wb, rays_o=o, rays_d=d, z=z)
        if fallback:
            continue
        for S in (16, 64):
            for B in _ray_counts(S):
                o, d, z = _rays(B, S, 3)
                out[f'{net}/ray{S}/{B}'] = _C.neus_sdf_points(desc, wb, rays_o=o, rays_d=d, z=z)
        for n_img in (3, 4):
            pts = torch.tensor(_shell_points(n_img, 5)).cuda()
            out[f'{net}/shells{n_img}/a'] = _C.neus_sdf_points(desc, wb, pts=pts)
            out[f'{net}/shells{n_img}/b'] = _C.neus_sdf_points(desc, wb, pts=pts)
    torch.cuda.synchronize()
    np.savez(out_path, **{k: v.cpu().numpy() for k, v in out.items()})


# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def runs():
    """{setting: {case: tensor}} -- one child process per setting, all four at once"""
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        procs = {}
        for s in SETTINGS:
            env = dict(os.environ)
            env.pop('VQN_NEUS_SDF_IMAGES', None)
            env.pop('VQN_NEUS_TILE32', None)
            if s != 'default':
                env['VQN_NEUS_SDF_IMAGES'] = s
            procs[s] = subprocess.Popen([sys.executable, os.path.abspath(__file__), os.path.join(tmp, s + '.npz')], env=env, cwd=ROOT,
                                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        res = {}
        for s, pr in procs.items():
            log, _ = pr.communicate(timeout=600)
            assert pr.returncode == 0, f'child (VQN_NEUS_SDF_IMAGES {s}) failed:\n{log[-3000:]}'
            with np.load(os.path.join(tmp, s + '.npz')) as z:
                res[s] = {k: torch.tensor(z[k]) for k in z.files}
    return res


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == torch.float32 and bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize('images', ['3', '4'])
@pytest.mark.parametrize('net', list(NETS))
def test_bit_equal_to_two_images(runs, net, images):
    keys = _case_keys(net)
    assert set(keys) <= set(runs['2']) and len(keys) == 2 * len(P_LIST) + len(_ray_counts(16)) + len(_ray_counts(64)) + 1
    bad = [k for k in keys if not _same(runs[images][k], runs['2'][k])]
    assert not bad, f'{images} images differ from two images at {bad}'
    # the cases are not degenerate: the two-image outputs vary from point to point
    assert runs['2'][f'{net}/pts/{P_LIST[-1]}'].std() > 1e-2


@pytest.mark.parametrize('images', ['3', '4'])
@pytest.mark.parametrize('net', list(NETS))
def test_in_place_layers_keep_images_and_calls_apart(runs, net, images):
    """neighbouring tiles with very different activations, the call repeated: a missing barrier around the in-place write-back shows as
    one image's (or the previous call's) rows in another's sums"""
    for n_img in (3, 4):
        a, b, ref = runs[images][f'{net}/shells{n_img}/a'], runs[images][f'{net}/shells{n_img}/b'], runs['2'][f'{net}/shells{n_img}/a']
        assert a.numel() == 32 * n_img * 3
        assert _same(a, b), 'the same call twice gives different results'
        assert _same(a, ref), f'{images} images differ from two images'
        assert _same(runs['2'][f'{net}/shells{n_img}/b'], ref)
        t = ref.reshape(-1, 32).mean(1)                      # the probe is what it claims: the tiles alternate between two sdf levels
        assert t[0::2].max() < t[1::2].min() - 0.5          # (radius 0.1: inside, 1.9: outside a surface of radius ~ 0.85)


def test_narrow_net_falls_back(runs):
    """max_tiles = 4 under VQN_NEUS_SDF_IMAGES=4 (and 3): the existing form, the default's results"""
    for P in FALLBACK_P:
        k = f'{FALLBACK_NET[0]}/pts/{P}'
        assert _same(runs['4'][k], runs['default'][k]) and _same(runs['3'][k], runs['default'][k]) and _same(runs['2'][k], runs['default'][k])


def test_default_form(runs):
    """the library has no introspection of the chosen form, and all forms give the same bits by design: what can be held is that the
    default setting gives those bits too, on every case"""
    for net in NETS:
        bad = [k for k in _case_keys(net) if not _same(runs['default'][k], runs['4'][k]) or not _same(runs['default'][k], runs['2'][k])]
        assert not bad, bad


if __name__ == '__main__':
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _child(sys.argv[1])
