"""GPU: the mesh rasteriser (csrc/mesh_raster.hip through _C.raster_count / raster_resolve / raster_interpolate) equals the plain-loop
model of tests/mesh_raster_model.py bit for bit -- face, depth, bary, the counters of dropped triangles -- with guard bands around
every output and scratch array untouched and two runs identical; refusals launch nothing."""
import numpy as np
import pytest
import torch

from tests import mesh_raster_model as model
from tests.test_mesh_raster_model import IDENTITY, look_at

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5a5a5a5a
DEPTH_P = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)          # w = z: (x z, y z, z) lands near pixel (x, y) at depth z


def _C():
    from vqnerf_release_amd import _C as c
    return c


def _guarded(shape, dtype=torch.int32):
    """-> (whole int32 buffer, the view of `shape` between two guard bands)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device='cuda')
    return whole, whole[GUARD: GUARD + n].view(dtype).reshape(shape)


def _guards_intact(bufs):
    for name, (whole, view) in bufs.items():
        n = view.numel()
        assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + n:] == SENTINEL).all(), name


def _run_once(verts, tris, P, H, W, near, cull):
    C = _C()
    v = torch.as_tensor(np.asarray(verts, np.float32).reshape(-1, 3), device='cuda')
    t = torch.as_tensor(np.asarray(tris, np.int32).reshape(-1, 3), device='cuda')
    ty, tx = C.raster_tiles(H, W)
    bufs = {'pverts': _guarded((v.shape[0], 3)), 'tile_count': _guarded((ty * tx,)), 'stats': _guarded((C.RASTER_STATS,))}
    pverts, tile_count, stats = C.raster_count(v, t, P, H, W, near, cull, out=tuple(bufs[k][1] for k in ('pverts', 'tile_count', 'stats')))
    ends = torch.cumsum(tile_count, 0, dtype=torch.int64)
    n_pairs = int(ends[-1])
    bufs.update({'cursor': _guarded((ty * tx,)), 'bin': _guarded((n_pairs,)), 'face': _guarded((H, W)),
                 'depth': _guarded((H, W), torch.float32), 'bary': _guarded((H, W, 3), torch.float32)})
    C.raster_resolve(t, pverts, H, W, cull, (ends - tile_count).to(torch.int32), n_pairs,
                     out=tuple(bufs[k][1] for k in ('cursor', 'bin', 'face', 'depth', 'bary')))
    torch.cuda.synchronize()
    _guards_intact(bufs)
    assert ((bufs['bin'][1] >= 0) & (bufs['bin'][1] < t.shape[0])).all()           # every slot of the bin was filled
    assert torch.equal(bufs['cursor'][1], tile_count)                              # ... by the pairs that were counted
    return {k: bufs[k][1].cpu().numpy().copy() for k in ('face', 'depth', 'bary', 'stats', 'tile_count')}, n_pairs


def run(verts, tris, P, H, W, near=1e-3, cull=0):
    """two guarded runs, identical -> the first's arrays"""
    a, n_pairs = _run_once(verts, tris, P, H, W, near, cull)
    b, _ = _run_once(verts, tris, P, H, W, near, cull)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    a['pairs'] = n_pairs
    return a


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check(verts, tris, P, H, W, near=1e-3, cull=0):
    """the device equals the model bit for bit -> (device arrays, model arrays)"""
    got = run(verts, tris, P, H, W, near, cull)
    want = model.rasterize(np.asarray(verts, np.float32), np.asarray(tris, np.int32).reshape(-1, 3), P, H, W, near=near, cull=cull)
    np.testing.assert_array_equal(got['stats'], want['stats'])
    np.testing.assert_array_equal(got['face'], want['face'])
    np.testing.assert_array_equal(bits(got['depth']), bits(want['depth']))
    np.testing.assert_array_equal(bits(got['bary']), bits(want['bary']))
    return got, want


def lift(xy, z):
    """pixel positions [n, 2] at depths [n] -> vertices for DEPTH_P"""
    xy, z = np.asarray(xy, np.float64), np.asarray(z, np.float64)
    return np.concatenate([xy * z[:, None], z[:, None]], 1).astype(np.float32)


@pytest.mark.parametrize('cull', [0, 1, -1])
@pytest.mark.parametrize('winding', [1, -1])
def test_one_triangle_ownership_and_culling(winding, cull):
    verts = np.array([[2, 2, 0], [12, 2, 0], [2, 12, 0]], np.float32)             # on pixel centres; the long edge passes through samples
    tris = [[0, 1, 2][::winding]]
    got, _ = check(verts, tris, IDENTITY, 16, 16, cull=cull)
    # [0, 1, 2] has a positive area2 (s = +1), the reversed triangle a negative one
    if cull == winding:
        assert (got['face'] == -1).all() and np.isinf(got['depth']).all() and got['stats'].tolist() == [0, 0, 0, 1]
        return
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing='ij')
    inside = (j > 2) & (i > 2) & (i + j <= 14)                                    # left and top edges are not owned, the long edge is
    np.testing.assert_array_equal(got['face'] == 0, inside)
    assert got['face'][7, 7] == 0 and got['face'][2, 5] == -1 and got['face'][5, 2] == -1


def test_equal_depth_goes_to_the_lowest_face_index():
    verts = lift([[1.5, 1.0], [13.25, 3.5], [4.0, 14.5]], [2.0, 3.0, 5.0])
    got, _ = check(verts, [[0, 1, 2], [0, 1, 2], [0, 1, 2]], DEPTH_P, 16, 16)
    assert (got['face'] >= 0).sum() > 40 and set(np.unique(got['face'])) == {-1, 0}
    got, _ = check(verts, [[2, 1, 0], [0, 1, 2]], DEPTH_P, 16, 16)                # (the same plane from the other side: the model decides)
    assert (got['face'] >= 0).sum() > 40


@pytest.mark.parametrize('windings', [(1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_a_shared_edge_through_samples_is_covered_once(windings):
    verts = np.array([[2, 2, 0], [12, 2, 0], [12, 12, 0], [2, 12, 0]], np.float32)
    tris = [[0, 1, 2][::windings[0]], [0, 2, 3][::windings[1]]]
    got, _ = check(verts, tris, IDENTITY, 16, 16)
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing='ij')
    np.testing.assert_array_equal(got['face'] >= 0, (j > 2) & (j <= 12) & (i > 2) & (i <= 12))
    diag = got['face'][np.arange(3, 13), np.arange(3, 13)]
    assert len(set(diag.tolist())) == 1 and diag[0] in (0, 1)                     # the seam belongs to one of the two, all along


def _random_scene(n, seed):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.3, 1.3, (n, 1, 3))
    verts = (centre + rng.uniform(-0.5, 0.5, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


@pytest.mark.parametrize('H,W', [(40, 24), (1, 1), (17, 1)])
def test_random_triangles_on_partial_tiles(H, W):
    verts, tris = _random_scene(300, 1)
    P = look_at((0.5, -0.4, 3.0), 14.0, (W / 2 - 0.3, H / 2 + 0.2))[0].astype(np.float32)
    got, _ = check(verts, tris, P, H, W, near=0.5)
    if (H, W) == (40, 24):
        assert (got['face'] >= 0).mean() > 0.3 and len(np.unique(got['face'])) > 20


@pytest.mark.parametrize('n', ['chunk-1', 'chunk', 'chunk+1', '2chunk+3'])
def test_chunk_boundaries_and_a_triangle_in_every_bin(n):
    chunk = _C().RASTER_CHUNK
    n = {'chunk-1': chunk - 1, 'chunk': chunk, 'chunk+1': chunk + 1, '2chunk+3': 2 * chunk + 3}[n]
    rng = np.random.default_rng(n)
    H, W = 24, 40
    # each small triangle surrounds one pixel centre of tile (0, 0), so it is in that tile's list and in no other
    c = rng.integers(1, 15, (n, 1, 2)).astype(np.float64)
    around = np.array([[-0.6, -0.4], [0.7, -0.5], [0.1, 0.8]])
    xy = (c + around[None] + rng.uniform(-0.1, 0.1, (n, 3, 2))).reshape(-1, 2)
    small = lift(xy, rng.uniform(1.0, 4.0, 3 * n))
    big = lift([[-50.0, -30.0], [200.0, -30.0], [-50.0, 150.0]], [6.0, 7.0, 8.0])  # behind the small ones, over the whole image
    verts = np.concatenate([small, big])
    tris = np.concatenate([np.arange(3 * n, dtype=np.int32).reshape(n, 3), [[3 * n, 3 * n + 1, 3 * n + 2]]]).astype(np.int32)
    order = rng.permutation(n + 1)                                                # the big one somewhere inside the list
    got, _ = check(verts, tris[order], DEPTH_P, H, W)
    assert got['tile_count'].tolist() == [n + 1, 1, 1, 1, 1, 1]
    assert (got['face'] >= 0).all() and len(np.unique(got['face'][:16, :16])) > 30


def test_dropped_triangles_are_counted_and_touch_nothing():
    limit = _C().RASTER_COORD_LIMIT / 256.0
    seen = lift([[3.0, 2.0], [12.5, 4.0], [5.0, 13.0]], [2.0, 2.5, 3.0])
    verts = np.concatenate([
        seen,
        lift([[3.0, 3.0], [9.0, 3.0], [3.0, 9.0]], [-1.0, -1.0, -1.0]),          # 3: behind the camera
        lift([[4.0, 4.0], [9.0, 4.0], [4.0, 9.0]], [1.0, 1.0, 0.4]),             # 6: straddles near = 0.5
        lift([[4.0, 4.0], [limit + 1.0, 4.0], [4.0, 9.0]], [1.0, 1.0, 1.0]),     # 9: beyond the coordinate limit
        lift([[2.0, 2.0], [6.0, 6.0], [10.0, 10.0]], [1.0, 1.0, 1.0]),           # 12: no area
    ])
    V = len(verts)
    dropped = [[3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [0, 1, V], [0, -1, 2]]
    got, _ = check(verts, dropped + [[0, 1, 2]], DEPTH_P, 16, 16, near=0.5)
    assert got['stats'].tolist() == [2, 3, 1, 0] and got['pairs'] == 1
    alone = run(seen, [[0, 1, 2]], DEPTH_P, 16, 16, near=0.5)
    np.testing.assert_array_equal(np.where(got['face'] == 6, 0, got['face']), alone['face'])
    assert got['depth'].tobytes() == alone['depth'].tobytes() and got['bary'].tobytes() == alone['bary'].tobytes()
    # the culled counter: the same list with both windings of the visible triangle, one of them culled
    got, _ = check(verts, dropped + [[0, 1, 2], [2, 1, 0]], DEPTH_P, 16, 16, near=0.5, cull=1)
    assert got['stats'].tolist() == [2, 3, 1, 1] and set(np.unique(got['face'])) == {-1, 7}
    # exactly at the limits: w == near is usable, |256 sx| == the limit is not
    edge = np.concatenate([lift([[3.0, 2.0], [12.5, 4.0], [5.0, 13.0]], [0.5, 0.5, 0.5]), np.array([[limit, 4.0, 1.0]], np.float32)])
    got, _ = check(edge, [[0, 1, 2], [0, 1, 3]], DEPTH_P, 16, 16, near=0.5)
    assert got['stats'].tolist() == [0, 1, 0, 0] and (got['face'] == 0).any()


def test_empty_meshes_give_the_background():
    for verts, tris in ((np.zeros((0, 3)), np.zeros((0, 3))), (np.ones((5, 3)), np.zeros((0, 3))), (np.zeros((0, 3)), [[0, 1, 2], [3, 4, 5]])):
        got, _ = check(verts, tris, DEPTH_P, 20, 33)
        assert (got['face'] == -1).all() and np.isinf(got['depth']).all() and (got['depth'] > 0).all() and not got['bary'].any()
        assert got['pairs'] == 0 and got['stats'].tolist() == [len(tris), 0, 0, 0]


def test_refusals_launch_nothing():
    C = _C()
    verts, tris = _random_scene(20, 2)
    v, t = torch.as_tensor(verts, device='cuda'), torch.as_tensor(tris, device='cuda')
    H, W = 20, 33
    ty, tx = C.raster_tiles(H, W)

    def buffers():
        return {'pverts': _guarded((60, 3)), 'tile_count': _guarded((ty * tx,)), 'stats': _guarded((C.RASTER_STATS,)), 'cursor': _guarded((ty * tx,)),
                'bin': _guarded((100,)), 'face': _guarded((H, W)), 'depth': _guarded((H, W), torch.float32), 'bary': _guarded((H, W, 3), torch.float32),
                'out': _guarded((H, W, 3), torch.float32), 'out17': _guarded((H, W, 17), torch.float32)}

    def untouched(bufs):
        torch.cuda.synchronize()
        for name, (whole, _) in bufs.items():
            assert (whole == SENTINEL).all(), name

    b = buffers()
    count_out = tuple(b[k][1] for k in ('pverts', 'tile_count', 'stats'))
    for kw, rc in ((dict(near=0.0), -1), (dict(near=-1.0), -1), (dict(near=float('inf')), -1), (dict(near=float('nan')), -1), (dict(cull=2), -1),
                   (dict(cull=-2), -1), (dict(H=0), -2), (dict(W=0), -2), (dict(H=C.RASTER_MAX_SIDE + 1), -2), (dict(W=C.RASTER_MAX_SIDE + 1), -2)):
        a = dict(H=H, W=W, near=1e-3, cull=0)
        a.update(kw)
        with pytest.raises(C.VqnError, match=r'rc=%d\)' % rc):
            C.raster_count(v, t, DEPTH_P, a['H'], a['W'], a['near'], a['cull'], out=count_out)
    untouched(b)
    offsets = torch.zeros((ty * tx,), dtype=torch.int32, device='cuda')
    pverts = torch.zeros((60, 3), dtype=torch.int32, device='cuda')
    resolve_out = tuple(b[k][1] for k in ('cursor', 'bin', 'face', 'depth', 'bary'))
    for kw, rc in ((dict(n_pairs=-1), -1), (dict(n_pairs=20 * ty * tx + 1), -1), (dict(cull=3), -1), (dict(H=0), -2), (dict(W=C.RASTER_MAX_SIDE + 1), -2),
                   (dict(n_pairs=1 << 31), -2)):
        a = dict(H=H, W=W, cull=0, n_pairs=10)
        a.update(kw)
        with pytest.raises(C.VqnError, match=r'rc=%d\)' % rc):
            C.raster_resolve(t, pverts, a['H'], a['W'], a['cull'], offsets, a['n_pairs'], out=resolve_out)
    untouched(b)
    face = torch.zeros((H, W), dtype=torch.int32, device='cuda')
    bary = torch.zeros((H, W, 3), dtype=torch.float32, device='cuda')
    with pytest.raises(C.VqnError, match=r'rc=-2\)'):
        C.raster_interpolate(face, bary, t, torch.zeros((60, 17), device='cuda'), torch.zeros((17,), device='cuda'), out=b['out17'][1])
    untouched(b)
    # the same buffers take a call that is not refused (the sentinels above were not a dead path)
    C.raster_count(v, t, DEPTH_P, H, W, 1e-3, 0, out=count_out)
    torch.cuda.synchronize()
    assert (b['stats'][1] != SENTINEL).all()


# ---- interpolate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_', [1, 3, 16])
def test_interpolate_equals_the_model(C_):
    C = _C()
    verts, tris = _random_scene(60, 3)
    H, W = 24, 40
    P = look_at((0.5, -0.4, 3.0), 14.0, (W / 2, H / 2))[0].astype(np.float32)
    got = run(verts, tris, P, H, W, near=0.5)
    rng = np.random.default_rng(C_)
    attr = rng.normal(size=(len(verts), C_)).astype(np.float32)
    background = rng.normal(size=C_).astype(np.float32)
    t = torch.as_tensor(tris, device='cuda')
    face, bary = torch.as_tensor(got['face'], device='cuda'), torch.as_tensor(got['bary'], device='cuda')
    for nearest in (False, True):
        whole, out = _guarded((H, W, C_), torch.float32)
        C.raster_interpolate(face, bary, t, torch.as_tensor(attr, device='cuda'), torch.as_tensor(background, device='cuda'), nearest, out=out)
        torch.cuda.synchronize()
        _guards_intact({'out': (whole, out)})
        want = model.interpolate(got['face'], got['bary'], tris, attr, background, nearest=nearest)
        np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(want))
        assert (out.cpu().numpy()[got['face'] < 0] == background).all() and (got['face'] < 0).any() and (got['face'] >= 0).any()


def test_interpolate_nearest_breaks_a_tie_towards_the_lowest_corner():
    from vqnerf_release_amd.geo import mesh_render
    verts = np.array([[2, 2, 0], [10, 2, 0], [6, 10, 0]], np.float32)             # symmetric about x = 6
    tris = np.array([[0, 1, 2]], np.int32)
    v, t = torch.as_tensor(verts, device='cuda'), torch.as_tensor(tris, device='cuda')
    r = mesh_render.rasterize(v, t, IDENTITY, 12, 12)
    b = r['bary'][3, 6].tolist()
    assert b[0] == b[1] > b[2] > 0 and r['stats'] == {'bad_index': 0, 'unusable_vertex': 0, 'zero_area': 0, 'culled': 0, 'pairs': 1}
    labels = torch.tensor([5, 9, 7], device='cuda')
    out = mesh_render.interpolate(r, t, labels, background=-1.0, nearest=True)
    assert out.shape == (12, 12) and out[3, 6] == 5.0 and out[9, 6] == 7.0 and out[0, 0] == -1.0
    want = model.interpolate(r['face'].cpu().numpy(), r['bary'].cpu().numpy(), tris, np.array([[5], [9], [7]], np.float32), [-1.0], nearest=True)
    np.testing.assert_array_equal(out.cpu().numpy(), want[..., 0])
    m = model.rasterize(verts, tris, IDENTITY, 12, 12)
    assert torch.equal(r['face'].cpu(), torch.as_tensor(m['face'])) and r['depth'].cpu().numpy().tobytes() == m['depth'].tobytes()
