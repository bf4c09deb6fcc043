"""GPU: the folded colour input of the f32 fine kernel (csrc/neus_fold.hip, csrc/neus_mlp.hip neus_points2_kernel<true, false, true>).

  * the device-built fold buffer against the float64 statement of tests/test_neus_fold_host.py: the copied colour pack bit for bit,
    every element of the three appended blocks within 1 ulp of the correctly rounded value;
  * out_sdf and out_grad of vqn_neus_fine_points, and every key of NeuSRenderer.render but `color_fine`, bit-equal folded vs unfolded
    (ragged P, explicit (pts, dirs) and ray forms, full-size and small networks, two cos_anneal ratios);
  * out_rgb against a float64 evaluation of the same networks (torch CPU double, as tests/test_gpu_neus_x3.py): the bound is
    2 x the error of the UNFOLDED kernel on the same inputs, measured once on MI355X with VQN_NEUS_FOLD=0 and kept in
    profiles/observed_errors_neus_fold.json (not the folded kernel's own error);
  * staleness: after each kind of weight write a folded render equals, bit for bit, the render of a fresh model on freshly built
    packs.  Writers as tests/test_gpu_weight_caches.py (whose geo-render-f32 row runs folded too); `broadcast_module` is the
    `data_copy` writer on every rank (a write into `.data` + weights_changed()), `replay` a raw write + weights_stepped().

Observed on MI355X (max |rgb - float64|, P = 1000 points): see the JSON; the test prints both figures before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import vqnerf_release_amd
from tests.test_neus_fold_host import fold_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, 'profiles', 'observed_errors_neus_fold.json')
P_ERR = 1000                                   # ragged: not a multiple of 64


def _build(name):
    from tests.test_gpu_neus_render import _build as b
    return b(name)


def _points(P, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.2, 1.2, (P, 3))
    dirs = rng.normal(size=(P, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return pts, dirs


def _pairs(ren):
    """(unfolded, folded) argument tuples (sdf_desc, wbuf_sdf, col_desc, wbuf_col) of neus_fine_points"""
    with torch.no_grad():
        wb_s, d_s, wb_c, d_c = ren._packs()
        _, _, fw, fd = ren._packs(fold=True)
    assert fw is not wb_c and fd[13] > 0
    return (d_s, wb_s, d_c, wb_c), (d_s, wb_s, fd, fw)


def rgb_errors_vs_float64(name, fold):
    """max |out_rgb - float64 rgb| of the fine kernel at P_ERR explicit points (and the same for sdf, grad)"""
    from oracle import geo as og
    from vqnerf_release_amd import _C
    cfg, sdf, col, var, ren = _build(name)
    pts, dirs = _points(P_ERR, 11)
    unf, fol = _pairs(ren)
    a = fol if fold else unf
    s, g, rgb = _C.neus_fine_points(*a, pts=torch.tensor(pts, dtype=torch.float32).cuda(), dirs=torch.tensor(dirs, dtype=torch.float32).cuda())
    x = torch.tensor(pts, dtype=torch.float32).double()            # the f32 inputs the kernel saw, evaluated in float64
    d = torch.tensor(dirs, dtype=torch.float32).double()
    p_sdf = og.to_torch(og.make_sdf_params(cfg, 0), torch.float64)
    p_col = og.to_torch(og.make_color_params(cfg, 1), torch.float64)
    with torch.no_grad():
        out = og.sdf_forward(p_sdf, cfg, x)
    grads = og.sdf_gradient(p_sdf, cfg, x)
    with torch.no_grad():
        want = og.color_forward(p_col, cfg, x, grads, d, out[:, 1:])
    return {'rgb': float((rgb.double().cpu() - want).abs().max()), 'sdf': float((s.double().cpu() - out[:, 0]).abs().max()),
            'grad': float((g.double().cpu() - grads).abs().max())}


@pytest.mark.parametrize('name', ['full', 'small'])
def test_fold_buffer_is_the_correctly_rounded_float64_fold(name):
    from vqnerf_release_amd import _C
    from tests.gpu_util import launches
    cfg, sdf, col, var, ren = _build(name)
    with torch.no_grad():
        wb_s, d_s, wb_c, d_c = ren._packs()
        with launches() as rec:
            _, _, fw, fd = ren._packs(fold=True)
    assert rec.ran('vqn_neus_fold_pack')
    sl, cl = getattr(sdf, f'lin{sdf.num_layers - 2}'), col.lin0
    with torch.no_grad():
        w8, b8 = sl.effective_weight().float().cpu().numpy(), sl.bias.float().cpu().numpy()
        wc0, bc0 = cl.effective_weight().float().cpu().numpy(), cl.bias.float().cpu().numpy()
    extra = int(d_c[3])
    blocks = fold_reference(w8, b8, wc0, bc0, extra)
    n0 = wb_c.numel()
    got = fw.cpu()
    assert torch.equal(got[:n0].view(torch.int32), wb_c.cpu().view(torch.int32))                 # the existing region: byte for byte
    assert got.numel() == n0 + sum(b.size for b in blocks)
    want_desc = np.array(d_c, np.int32).copy()
    want_desc[13:16] = [n0 // 4, (n0 + blocks[0].size) // 4, (n0 + blocks[0].size + blocks[1].size) // 4]
    np.testing.assert_array_equal(np.asarray(fd), want_desc)                                      # every existing field untouched
    off = n0
    for what, blk in zip(('Wfold', 'bfold', 'extras'), blocks):
        g = got[off:off + blk.size].numpy().astype(np.float64)
        want32 = blk.astype(np.float32)                                                           # the correctly rounded value
        ulp = np.spacing(np.abs(want32)).astype(np.float64)
        worst = float((np.abs(g - want32.astype(np.float64)) / ulp).max())
        print(f'[observed] fold buffer {name} {what}: worst {worst:.2f} ulp, {int((g != want32).sum())} of {blk.size} differ')
        assert worst <= 1.0, what
        off += blk.size
    assert np.array_equal(got[off - blocks[2].size:off].numpy(), blocks[2].astype(np.float32))     # a plain gather: exact


@pytest.mark.parametrize('form', ['pts', 'rays'])
@pytest.mark.parametrize('name', ['full', 'small'])
def test_sdf_and_gradient_are_bit_equal_folded_vs_unfolded(name, form):
    from vqnerf_release_amd import _C
    cfg, sdf, col, var, ren = _build(name)
    unf, fol = _pairs(ren)
    if form == 'pts':
        pts, dirs = _points(1000, 3)
        kw = dict(pts=torch.tensor(pts, dtype=torch.float32).cuda(), dirs=torch.tensor(dirs, dtype=torch.float32).cuda())
    else:
        from oracle import geo as og
        o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(37, 2)]
        z = (near + (far - near) * torch.linspace(0, 1, 27, device='cuda')[None, :]).contiguous()      # P = 999
        kw = dict(rays_o=o.contiguous(), rays_d=d.contiguous(), z=z)
    s0, g0, c0 = _C.neus_fine_points(*unf, **kw)
    s1, g1, c1 = _C.neus_fine_points(*fol, **kw)
    assert torch.equal(s0, s1) and torch.equal(g0, g1)
    diff = float((c0 - c1).abs().max())
    print(f'[observed] {name} {form}: max |rgb folded - unfolded| = {diff:.3e}')
    assert diff <= 2e-4                      # (the golden tolerance of tests/test_gpu_neus_mlp.py; the float64 bound is the test below)
    assert bool(torch.isfinite(c1).all())


@pytest.mark.parametrize('name', ['full', 'small'])
def test_render_keys_are_bit_equal_but_the_colour(name, monkeypatch):
    from oracle import geo as og
    from tests.gpu_util import launches
    cfg, sdf, col, var, ren = _build(name)
    o, d, near, far = [torch.tensor(a).cuda() for a in og.make_rays(21, 2)]
    for car in (0.0, 1.0):
        kw = dict(perturb_overwrite=0, background_rgb=torch.ones(1, 3, device='cuda'), cos_anneal_ratio=car)
        with torch.no_grad():
            with launches() as rec:
                a = ren.render(o, d, near, far, 2.0, **kw)
            assert rec.ran('vqn_neus_fine_points')
            monkeypatch.setenv('VQN_NEUS_FOLD', '0')
            b = ren.render(o, d, near, far, 2.0, **kw)
            monkeypatch.delenv('VQN_NEUS_FOLD')
        for k in a:
            if k != 'color_fine':
                assert torch.equal(a[k], b[k]), k
        assert float((a['color_fine'] - b['color_fine']).abs().max()) <= 2e-4


@pytest.mark.parametrize('name', ['full', 'small'])
def test_rgb_error_against_float64_is_within_twice_the_unfolded_kernels(name):
    with open(OBSERVED) as f:
        obs = json.load(f)['unfolded'][name]
    got = rgb_errors_vs_float64(name, fold=True)
    print(f'[observed] {name}: folded max |rgb - f64| = {got["rgb"]:.3e}; unfolded (recorded) {obs["rgb"]:.3e}; bound {2 * obs["rgb"]:.3e}')
    assert got['rgb'] <= 2.0 * obs['rgb']
    assert got['sdf'] <= 2.0 * obs['sdf'] and got['grad'] <= 2.0 * obs['grad']          # (bit-equal to the unfolded kernel's anyway)


WRITERS = ['inplace', 'data_copy', 'multi_copy', 'torch_adam', 'hip_adam', 'load_state_dict', 'replace', 'data_copy_frozen', 'replay']


@pytest.mark.parametrize('writer', WRITERS)
def test_no_stale_fold_after_a_weight_write(writer):
    from tests.gpu_util import launches
    from tests.test_gpu_weight_caches import _GeoPath, _write, _named, _targets
    path = _GeoPath('render', 'f32')
    h = path.build()
    if writer.endswith('_frozen'):
        for mod in h.nets_written:
            for p in mod.parameters():
                p.requires_grad_(False)
    out0 = path.run(h)['rgb'].clone()
    assert h.ren._fold is not None                                    # the first render built the fold
    if writer == 'replay':                                            # what a replayed training graph does: raw writes, then weights_stepped()
        for (_, _, p), t in zip(_named(h), _targets(h, 1)):
            p.data.copy_(t)
        vqnerf_release_amd.weights_stepped()
    else:
        _write(path, h, writer)
    with launches() as rec:
        out1 = path.run(h)['rgb']
    assert rec.ran('vqn_neus_fold_pack') and rec.ran('vqn_neus_fine_points')
    fresh = path.build()
    path.load(fresh, h)
    out_fresh = path.run(fresh)['rgb']
    assert torch.equal(out1, out_fresh), float((out1 - out_fresh).abs().max())
    assert float((out1 - out0).abs().max()) > 1e-2                    # the weights really moved (10 x the render tolerance)
