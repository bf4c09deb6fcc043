"""GPU: a point's outputs do not depend on the tile or image slot it lands in.

The fused NeuS kernels (csrc/neus_mlp*.hip) walk the points in tiles of 32 and, in their two-image forms, hold two tiles per
workgroup (image 0 and image 1).  Dropping the first 32 points of a batch of 97 moves every remaining point from one image slot to
the other and leaves 65 points: three tiles, so the last pair has a phantom second tile.  Dropping 64 leaves 33 points: one pair
whose second tile holds a single point.  The arithmetic per point is the same in every slot, so
the outputs must agree bit for bit -- what a slip in the image indexing of a kernel breaks.  Per engine, the widths cover each
kernel form: f32 64 (one image), 160 (two images, 5 tiles), 320 (one-image fall-back); f16s 64 (two images), 320 (one image);
x3 64 and 256 (always two images)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [('f32', 64), ('f32', 160), ('f32', 320), ('f16s', 64), ('f16s', 320), ('x3', 64), ('x3', 256)]
_packs = {}


def _net(mode, width):
    """(sdf_desc, wbuf_sdf, col_desc, wbuf_col) of a shallow network pair of the given hidden width, built once per case."""
    if (mode, width) not in _packs:
        from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork
        feat = min(width, 256)
        torch.manual_seed(width)
        sdf = SDFNetwork(d_in=3, d_out=feat + 1, d_hidden=width, n_layers=4, skip_in=(2,), multires=6, bias=0.5, scale=1.0,
                         geometric_init=True, weight_norm=True).cuda()
        col = RenderingNetwork(d_feature=feat, mode='idr', d_in=9, d_out=3, d_hidden=width, n_layers=2, weight_norm=True,
                               multires_view=4, squeeze_out=True).cuda()
        wb_s, d_s = sdf.packs(max_tiles=col.max_tiles(), mode=mode)
        wb_c, d_c = col.packs(feat_tiles=sdf.plan(mode=mode).tiles[-1], mode=mode)
        _packs[(mode, width)] = (d_s, wb_s, d_c, wb_c)
    return _packs[(mode, width)]


@pytest.mark.parametrize('mode,width', CASES)
def test_outputs_do_not_depend_on_the_slot(mode, width):
    from vqnerf_release_amd import _C
    d_s, wb_s, d_c, wb_c = _net(mode, width)
    rng = np.random.default_rng(17)
    n = 97                                                             # tiles 32 + 32 + 32 + 1
    pts = torch.tensor(rng.uniform(-1, 1, (n, 3)).astype(np.float32)).cuda()
    dirs = torch.nn.functional.normalize(torch.tensor(rng.normal(size=(n, 3)).astype(np.float32)), dim=-1).cuda()
    whole = _C.neus_fine_points(d_s, wb_s, d_c, wb_c, pts=pts, dirs=dirs, mode=mode) + (_C.neus_sdf_points(d_s, wb_s, pts=pts, mode=mode),)
    assert all(bool(torch.isfinite(t).all()) for t in whole)
    for k in (32, 64):                                                 # 65 points: image 1 -> image 0, phantom last tile; 33: one ragged pair
        p, d = pts[k:].contiguous(), dirs[k:].contiguous()
        part = _C.neus_fine_points(d_s, wb_s, d_c, wb_c, pts=p, dirs=d, mode=mode) + (_C.neus_sdf_points(d_s, wb_s, pts=p, mode=mode),)
        for name, a, b in zip(('sdf', 'grad', 'rgb', 'sdf (sdf-only kernel)'), part, whole):
            assert torch.equal(a, b[k:]), (mode, width, k, name, float((a - b[k:]).abs().max()))


@pytest.mark.parametrize('mode,width', [('f32', 160), ('f16s', 64), ('x3', 64)])
def test_ray_form_does_not_depend_on_the_slot(mode, width):
    """7 rays of 16 samples (112 points); without the first 2 rays the remaining 80 points start one tile earlier."""
    from vqnerf_release_amd import _C
    d_s, wb_s, d_c, wb_c = _net(mode, width)
    rng = np.random.default_rng(19)
    B, S = 7, 16
    o = torch.tensor(rng.uniform(-0.2, 0.2, (B, 3)).astype(np.float32)).cuda()
    d = torch.nn.functional.normalize(torch.tensor(rng.normal(size=(B, 3)).astype(np.float32)), dim=-1).cuda()
    z = torch.tensor(np.sort(rng.uniform(0.05, 1.0, (B, S)).astype(np.float32), axis=1)).cuda()
    whole = _C.neus_fine_points(d_s, wb_s, d_c, wb_c, rays_o=o, rays_d=d, z=z, mode=mode) + \
        (_C.neus_sdf_points(d_s, wb_s, rays_o=o, rays_d=d, z=z, mode=mode),)
    o2, d2, z2 = o[2:].contiguous(), d[2:].contiguous(), z[2:].contiguous()
    part = _C.neus_fine_points(d_s, wb_s, d_c, wb_c, rays_o=o2, rays_d=d2, z=z2, mode=mode) + \
        (_C.neus_sdf_points(d_s, wb_s, rays_o=o2, rays_d=d2, z=z2, mode=mode),)
    for name, a, b in zip(('sdf', 'grad', 'rgb', 'sdf (sdf-only kernel)'), part, whole):
        assert torch.equal(a, b[2 * S:]), (mode, name, float((a - b[2 * S:]).abs().max()))
