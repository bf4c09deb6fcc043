"""GPU: the workgroup form of the f32 fine NeuS kernel (neus_points2w_kernel, csrc/neus_mlp.hip: two in-place 32-point images per
256-thread workgroup, two independent workgroups on a CU) against the two-image form it stands in for (neus_points2_kernel), bit for
bit: same per-point arithmetic in the same order, so every output must be the same float.  No tolerance anywhere in this file.

The form is chosen once per process (VQN_NEUS_FORM), so every setting runs in a child process of its own, under a time limit of its
own -- this file, run as a script, is the child: it evaluates every case below and leaves the outputs in an .npz.  The children are
started together on first use and shared by all tests.  `images` (VQN_NEUS_FORM=images) is the reference, `default` the workgroup
form wherever the library takes it.

Cases.  Nets (8 layers, skip 4, multires 6, as shipped) of d_hidden
  64   2 tiles: below what the form takes -- the ping-pong one-image kernel under both settings (the fall-back);
  160  5 tiles: wave 0 owns two tiles, the others one; two K slices of the embedding gradient;
  256  the shipped shape: the 7-tile layer (waves with one tile and with two), the ragged K of the skip layer, four K slices of 8 and
       of 7 row groups.
vqn_neus_fine_points in its point and ray forms (S = 1 and S = 16), on unfolded and folded colour packs and gradient-only (a col_desc
with n_lin == 0), at P in {1, 31, 33, 97, 4099}; a 48-ray NeuSRenderer.render of the shipped shape; vqn_neus_sdf_points, whose form
the setting must not change.  The second trip through the persistent loop (stale accumulators, LDS left by the previous pair): P = 97
on a scratch that holds exactly one workgroup's two stashes, so that ONE workgroup walks both pairs of tiles.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_LIST = [1, 31, 33, 97, 4099]
P_LOOP_SDF = 70001
WIDTHS = {'w64': 64, 'w160': 160, 'w256': 256}
SETTINGS = {'default': {}, 'images': {'VQN_NEUS_FORM': 'images'}}
KNOBS = ('VQN_NEUS_FORM', 'VQN_NEUS_SDF_IMAGES', 'VQN_NEUS_TILE32', 'VQN_NEUS_FOLD')
CHILD_TIMEOUT_S = 300
RENDER_RAYS = 48


def _sdf_keys(net):
    return [f'{net}/sdf/{form}/{P}' for form in ('pts', 'ray1') for P in P_LIST] + [f'{net}/sdf/ray16/112', f'{net}/sdf/pts/{P_LOOP_SDF}']


def _fine_keys(net):
    keys = []
    for pack in ('unfolded', 'folded'):
        keys += [f'{net}/fine/{pack}/pts/{P}.{o}' for P in P_LIST for o in ('sdf', 'grad', 'rgb')]
        keys += [f'{net}/fine/{pack}/{form}.{o}' for form in ('ray1/97', 'ray16/112', 'one_stash/97', 'again/97') for o in ('sdf', 'grad', 'rgb')]
    keys += [f'{net}/fine/gradonly/pts/{P}.{o}' for P in P_LIST for o in ('sdf', 'grad')]
    return keys + [f'{net}/fine/gradonly/one_stash/97.{o}' for o in ('sdf', 'grad')]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the child: every case under this process's setting -> npz

def _build(width):
    import torch
    from oracle import geo as og
    from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork, SingleVarianceNetwork
    from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
    cfg = {k: dict(v) for k, v in og.FULL_CFG.items()}
    cfg['sdf'].update(d_hidden=width, d_out=width + 1, bias=0.85)
    cfg['color'].update(d_feature=width, d_hidden=width)
    c, cc = cfg['sdf'], cfg['color']
    sdf = SDFNetwork(d_in=3, d_out=c['d_out'], d_hidden=c['d_hidden'], n_layers=c['n_layers'], skip_in=tuple(c['skip_in']),
                     multires=c['multires'], bias=c['bias'], scale=c['scale'], geometric_init=True, weight_norm=True)
    sdf.load_state_dict({k: torch.tensor(v) for k, v in og.make_sdf_params(cfg, 0).items()})
    col = RenderingNetwork(d_feature=cc['d_feature'], mode=cc['mode'], d_in=cc['d_in'], d_out=cc['d_out'], d_hidden=cc['d_hidden'],
                           n_layers=cc['n_layers'], weight_norm=True, multires_view=cc['multires_view'], squeeze_out=cc['squeeze_out'])
    col.load_state_dict({k: torch.tensor(v) for k, v in og.make_color_params(cfg, 1).items()})
    return NeuSRenderer(None, sdf.cuda(), SingleVarianceNetwork(0.3).cuda(), col.cuda(), **cfg['renderer'])


def _rays(B, S, seed):
    import torch
    from oracle import geo as og
    o, d, near, far = map(torch.tensor, og.make_rays(B, seed))
    z = near + (far - near) * torch.linspace(0, 1, S)[None, :]
    return dict(rays_o=o.cuda(), rays_d=d.contiguous().cuda(), z=z.contiguous().cuda())


def _points(P, seed):
    import torch
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(P, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return dict(pts=torch.tensor(rng.uniform(-1.2, 1.2, (P, 3)).astype(np.float32)).cuda(), dirs=torch.tensor(dirs.astype(np.float32)).cuda())


def _fine_on_one_stash(d_s, wb_s, d_c, wb_c, pts, dirs):
    """vqn_neus_fine_points on a scratch of exactly two images' stashes: ONE workgroup, which walks every pair of tiles"""
    import torch
    from vqnerf_release_amd import _C
    P = pts.shape[0]
    buf = torch.empty((2 * (int(d_s[0]) - 1) * 4 * int(d_s[5]) * 1024,), dtype=torch.uint8, device='cuda')     # two images of (n_lin - 1) * 4 max_tiles rows
    sdf, grad, rgb = (torch.empty(s, dtype=torch.float32, device='cuda') for s in ((P,), (P, 3), (P, 3)))
    _C._call('vqn_neus_fine_points', _C._host(d_s), _C._ptr(wb_s), _C._host(d_c), _C._ptr(wb_c), None, None, None, _C._ptr(pts),
             _C._ptr(dirs), P, 1, _C._ptr(buf), buf.numel(), _C._ptr(sdf), _C._ptr(grad), _C._ptr(rgb))
    return sdf, grad, rgb


def _child(out_path):
    import torch
    from oracle import geo as og
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo import packing
    out = {}
    for net, width in WIDTHS.items():
        ren = _build(width)
        with torch.no_grad():
            wb_s, d_s, wb_c, d_c = ren._packs()
            _, _, fw, fd = ren._packs(fold=True)
        assert fd[13] > 0 and int(d_s[5]) == (width + 31) // 32
        for P in P_LIST + [P_LOOP_SDF]:
            out[f'{net}/sdf/pts/{P}'] = _C.neus_sdf_points(d_s, wb_s, pts=_points(P, 11)['pts'])
        for P in P_LIST:
            out[f'{net}/sdf/ray1/{P}'] = _C.neus_sdf_points(d_s, wb_s, **_rays(P, 1, 2))
        out[f'{net}/sdf/ray16/112'] = _C.neus_sdf_points(d_s, wb_s, **_rays(7, 16, 3))
        no_col = np.zeros(packing.COL_DESC_INTS, np.int32)
        packs = {'unfolded': (d_s, wb_s, d_c, wb_c), 'folded': (d_s, wb_s, fd, fw), 'gradonly': (d_s, wb_s, no_col, wb_s)}
        for pack, a in packs.items():
            res = {f'pts/{P}': _C.neus_fine_points(*a, **_points(P, 5)) for P in P_LIST}
            res['one_stash/97'] = _fine_on_one_stash(*a, **_points(97, 5))
            if pack != 'gradonly':
                res['ray1/97'] = _C.neus_fine_points(*a, **_rays(97, 1, 2))
                res['ray16/112'] = _C.neus_fine_points(*a, **_rays(7, 16, 3))
                res['again/97'] = _C.neus_fine_points(*a, **_points(97, 5))
            for k, (s, g, c) in res.items():
                out[f'{net}/fine/{pack}/{k}.sdf'], out[f'{net}/fine/{pack}/{k}.grad'] = s, g
                if pack != 'gradonly':
                    out[f'{net}/fine/{pack}/{k}.rgb'] = c
        if net == 'w256':
            o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(RENDER_RAYS, 2)]
            with torch.no_grad():
                r = ren.render(o, d, near, far, 2.0, perturb_overwrite=0, background_rgb=torch.ones(1, 3, device='cuda'), cos_anneal_ratio=1.0)
            out.update({f'render/{k}': v.float() for k, v in r.items() if torch.is_tensor(v)})
    torch.cuda.synchronize()
    np.savez(out_path, **{k: v.cpu().numpy() for k, v in out.items()})


# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def runs():
    """{setting: {case: tensor}} -- one child process per setting, each under its own time limit"""
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        procs = {}
        for s, knobs in SETTINGS.items():
            env = {k: v for k, v in os.environ.items() if k not in KNOBS}
            env.update(knobs)
            procs[s] = subprocess.Popen([sys.executable, os.path.abspath(__file__), os.path.join(tmp, s + '.npz')], env=env, cwd=ROOT,
                                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        res, failed = {}, []
        for s, pr in procs.items():
            try:
                log, _ = pr.communicate(timeout=CHILD_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                pr.kill()
                log, _ = pr.communicate()
                failed.append(f'child {s} passed its time limit of {CHILD_TIMEOUT_S} s:\n{log[-3000:]}')
                continue
            if pr.returncode != 0:
                failed.append(f'child {s} failed ({pr.returncode}):\n{log[-3000:]}')
                continue
            with np.load(os.path.join(tmp, s + '.npz')) as z:
                res[s] = {k: torch.tensor(z[k]) for k in z.files}
        assert not failed, '\n'.join(failed)
    return res


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == torch.float32 and bool(torch.isfinite(a).all()) and torch.equal(a, b)


def _differing(runs, setting, keys):
    assert set(keys) <= set(runs['images']), sorted(set(keys) - set(runs['images']))
    return [k for k in keys if not _same(runs[setting][k], runs['images'][k])]


@pytest.mark.parametrize('net', list(WIDTHS))
def test_sdf_points_bit_equal(runs, net, setting='default'):
    keys = _sdf_keys(net)
    assert len(keys) == 2 * len(P_LIST) + 2
    bad = _differing(runs, setting, keys)
    assert not bad, f'the workgroup form differs from the two-image form at {bad}'
    assert runs['images'][f'{net}/sdf/pts/4099'].std() > 1e-2            # not degenerate: the outputs vary from point to point


@pytest.mark.parametrize('net', list(WIDTHS))
def test_fine_points_bit_equal(runs, net, setting='default'):
    keys = _fine_keys(net)
    assert len(keys) == 2 * 3 * (len(P_LIST) + 4) + 2 * (len(P_LIST) + 1)
    bad = _differing(runs, setting, keys)
    assert not bad, f'the workgroup form differs from the two-image form at {bad}'
    ref = runs['images']
    for pack in ('unfolded', 'folded'):
        for o in ('rgb', 'grad'):                                      # not degenerate: (nearly) every output a value of its own
            t = ref[f'{net}/fine/{pack}/pts/4099.{o}']
            assert t.unique().numel() > t.numel() // 2
        for o in ('sdf', 'grad', 'rgb'):                               # the same call twice, and one workgroup over four tiles: the same results
            assert _same(runs[setting][f'{net}/fine/{pack}/again/97.{o}'], ref[f'{net}/fine/{pack}/pts/97.{o}'])
            assert _same(runs[setting][f'{net}/fine/{pack}/one_stash/97.{o}'], ref[f'{net}/fine/{pack}/pts/97.{o}'])


def test_render_bit_equal(runs, setting='default'):
    keys = [k for k in runs['images'] if k.startswith('render/')]
    assert {'render/color_fine', 'render/gradients', 'render/weight_sum'} <= set(keys)
    bad = _differing(runs, setting, keys)
    assert not bad, f'the workgroup form differs from the two-image form at {bad}'
    assert tuple(runs['images']['render/color_fine'].shape) == (RENDER_RAYS, 3)


def test_both_settings_ran_every_case(runs):
    assert set(runs['default']) == set(runs['images']) and len(runs['images']) > 3 * (len(_sdf_keys('w64')) + len(_fine_keys('w64')))


if __name__ == '__main__':
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _child(sys.argv[1])
