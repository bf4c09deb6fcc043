"""CPU: the plain-loop model of the mesh rasteriser (tests/mesh_raster_model.py) is right -- exactly-once coverage of a triangulated
rectangle, agreement with an independent float64 ray caster -- and geo/mesh_render.camera_from_rays recovers the camera of a ray set."""
import math

import numpy as np
import pytest
import torch

from tests import mesh_raster_model as model

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float32)       # w = 1, (sx, sy) = (x, y): vertices in pixels


def test_a_triangulated_rectangle_is_covered_exactly_once():
    """5 x 4 quads, each cut along one of its diagonals with one of the two windings per triangle; the inner vertices sit off the pixel
    centres, the border on them.  Every sample inside is covered once; the right and bottom borders are owned, the left and top are not."""
    rng = np.random.default_rng(0)
    x0, x1, y0, y1 = 2, 17, 1, 13
    xs, ys = np.linspace(x0, x1, 6), np.linspace(y0, y1, 5)
    gx, gy = np.meshgrid(xs, ys, indexing='xy')                                   # [5, 6]
    jitter = rng.integers(-200, 201, (2, 5, 6)) / 256.0
    jitter[:, [0, -1], :] = 0
    jitter[:, :, [0, -1]] = 0
    gx, gy = gx + jitter[0], gy + jitter[1]
    gx[2, 2], gy[2, 2] = 8.0, 7.0                                                 # one inner vertex on a pixel centre
    verts = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(30)], 1).astype(np.float32)
    assert np.array_equal(verts[:, :2] * 256, np.rint(verts[:, :2] * 256))        # snapping moves nothing: the borders stay straight
    tris = []
    for r in range(4):
        for c in range(5):
            a, b, d, e = r * 6 + c, r * 6 + c + 1, (r + 1) * 6 + c, (r + 1) * 6 + c + 1
            pair = [[a, b, e], [a, e, d]] if (r + c) % 2 else [[a, b, d], [b, e, d]]
            for t in pair:
                tris.append(t[::-1] if rng.integers(2) else t)
    tris = np.asarray(tris, np.int32)
    H, W = 16, 20
    cover = np.zeros((H, W), np.int64)
    out = model.rasterize(verts, tris, IDENTITY, H, W, cull=0, coverage=cover)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    want = ((j > x0) & (j <= x1) & (i > y0) & (i <= y1)).astype(np.int64)
    np.testing.assert_array_equal(cover, want)
    assert np.array_equal(out['face'] >= 0, want == 1) and out['stats'].tolist() == [0, 0, 0, 0]
    assert np.array_equal(out['depth'][want == 1], np.ones(int(want.sum()), np.float32))
    np.testing.assert_allclose(out['bary'].sum(-1)[want == 1], 1.0, atol=2e-7)


# ---- an independent float64 ray caster -----------------------------------------------------------------------------------------------
def icosahedron():
    p = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1],
                  [-p, 0, -1], [-p, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    return v / np.linalg.norm(v[0]), f


def look_at(eye, focal, centre):
    """-> (P float64 [3, 4] with a unit third row, R [3, 3] world -> camera, K)"""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, [0.0, 1.0, 0.1]); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    K = np.array([[focal, 0, centre[0]], [0, focal, centre[1]], [0, 0, 1.0]])
    return K @ np.concatenate([R, (-R @ eye)[:, None]], 1), R, K


def moller_trumbore(o, d, v0, v1, v2):
    """-> t of the hit of the ray o + t d with the triangle, or None"""
    e1, e2 = v1 - v0, v2 - v0
    h = np.cross(d, e2)
    a = e1 @ h
    if abs(a) < 1e-14:
        return None
    s = o - v0
    u = (s @ h) / a
    q = np.cross(s, e1)
    v = (d @ q) / a
    t = (e2 @ q) / a
    return t if u >= 0 and v >= 0 and u + v <= 1 and t > 0 else None


def segment_distance(p, a, b):
    ab = b - a
    s = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(p - (a + s * ab))


@pytest.mark.parametrize('eye', [(0.4, 0.3, 3.0), (-2.1, 1.2, 1.7), (1.0, -2.6, -0.9)])
def test_the_model_agrees_with_a_float64_ray_caster(eye):
    H = W = 64
    verts, faces = icosahedron()
    P, R, K = look_at(eye, 64.0, (31.25, 32.5))
    out = model.rasterize(verts.astype(np.float32), faces, P.astype(np.float32), H, W, near=1e-3, cull=0)
    assert out['stats'].tolist() == [0, 0, 0, 0]
    hom = np.concatenate([verts, np.ones((12, 1))], 1) @ P.T
    scr = hom[:, :2] / hom[:, 2:]                                                 # the unsnapped projections
    edge_set = sorted({tuple(sorted((int(f[k]), int(f[(k + 1) % 3])))) for f in faces for k in range(3)})
    assert len(edge_set) == 30
    eye = np.asarray(eye, np.float64)
    Kinv = np.linalg.inv(K)
    skipped = 0
    for i in range(H):
        for j in range(W):
            p = np.array([j, i], np.float64)
            if min(segment_distance(p, scr[a], scr[b]) for a, b in edge_set) <= 2.0 / 256.0:
                skipped += 1                                                      # the band that vertex snapping can move
                continue
            d = R.T @ (Kinv @ np.array([j, i, 1.0]))
            hits = [(t, n) for n, f in enumerate(faces) for t in [moller_trumbore(eye, d, *verts[f])] if t is not None]
            if not hits:
                assert out['face'][i, j] == -1 and np.isinf(out['depth'][i, j]), (i, j)
                continue
            t, n = min(hits)
            assert out['face'][i, j] == n, (i, j)
            depth = t * (R[2] @ d)                                                # along the optical axis
            # 1 / depth is affine over the face's screen footprint: 1 / depth = g . (u, v, 1).  Snapping moves every vertex by at most
            # 0.5 / 256 px per axis, which to first order is a shift of the sample by a convex combination of those moves, less than
            # 1 / 256 px: |d depth| <= depth^2 |g_uv| / 256, plus the f32 rounding of the result
            g = np.linalg.solve(np.concatenate([scr[faces[n]], np.ones((3, 1))], 1), 1.0 / hom[faces[n], 2])
            tol = depth ** 2 * np.hypot(g[0], g[1]) / 256.0 + 4 * np.finfo(np.float32).eps * depth
            assert abs(float(out['depth'][i, j]) - depth) <= tol, (i, j, float(out['depth'][i, j]), depth, tol)
            b = out['bary'][i, j].astype(np.float64)
            assert abs(b.sum() - 1.0) < 1e-6 and (b >= 0).all()
    assert skipped <= 0.02 * H * W, skipped


def test_interpolate_model_nearest_and_background():
    face = np.array([[0, -1, 0]], np.int32)
    bary = np.array([[[0.25, 0.5, 0.25], [0, 0, 0], [0.5, 0.5, 0.0]]], np.float32)
    attr = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], np.float32)
    lin = model.interpolate(face, bary, [[0, 1, 2]], attr, [7.0, 8.0])
    np.testing.assert_array_equal(lin[0], np.array([[2.25, 22.5], [7.0, 8.0], [1.5, 15.0]], np.float32))
    near = model.interpolate(face, bary, [[0, 1, 2]], attr, [7.0, 8.0], nearest=True)
    np.testing.assert_array_equal(near[0], np.array([[2.0, 20.0], [7.0, 8.0], [1.0, 10.0]], np.float32))     # the tie goes to corner 0


# ---- camera_from_rays ----------------------------------------------------------------------------------------------------------------
def _datasets(tmp_path):
    pytest.importorskip('PIL.Image')
    from tests.test_datasets import _write_blender_set, _write_dtu_set
    from vqnerf_release_amd.geo import conf as hocon
    from vqnerf_release_amd.geo.models import dtuset, nerfset
    a, b = tmp_path / 'blender', tmp_path / 'dtu'
    a.mkdir(), b.mkdir()
    _write_blender_set(str(a))
    _write_dtu_set(b)
    return {'nerfset': nerfset.Dataset(hocon.parse_string('dataset { data_dir = %s\n longint = false }' % a)['dataset'], device='cpu'),
            'dtuset': dtuset.Dataset(hocon.parse_string('dataset { data_dir = %s }' % b)['dataset'], device='cpu')}


def test_camera_from_rays_projects_every_ray_to_its_own_pixel(tmp_path):
    from vqnerf_release_amd.geo import mesh_render
    for name, ds in _datasets(tmp_path).items():
        for level in (1, 2):
            for idx in range(ds.n_images):
                o, v = ds.gen_rays_at(idx, resolution_level=level)[:2]
                H, W = v.shape[:2]
                assert (H, W) == (ds.H // level, ds.W // level)
                P = mesh_render.camera_from_rays(o, v)
                assert P.dtype == np.float32 and P.shape == (3, 4) and abs(np.linalg.norm(P[2, :3].astype(np.float64)) - 1.0) < 1e-6
                x = (o + 2.0 * v).double().numpy().reshape(-1, 3)
                h = x @ P[:, :3].astype(np.float64).T + P[:, 3].astype(np.float64)
                i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
                assert (h[:, 2] > 0).all(), (name, level)
                err = np.maximum(np.abs(h[:, 0] / h[:, 2] - j.reshape(-1)), np.abs(h[:, 1] / h[:, 2] - i.reshape(-1))).max()
                assert err < 1e-3, (name, level, idx, err)
                # w is the distance along the optical axis: the unit third row against the ray of the largest w / |x - o|
                axis = P[2, :3].astype(np.float64)
                assert ((v.double().numpy().reshape(-1, 3) @ axis) <= 1.0 + 1e-6).all()


def test_camera_from_rays_refuses_a_bent_ray_set(tmp_path):
    from vqnerf_release_amd.geo import mesh_render
    ds = _datasets(tmp_path)['nerfset']
    o, v = ds.gen_rays_at(0)
    H, W = v.shape[:2]
    i, j = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    r2 = ((i - H / 2) ** 2 + (j - W / 2) ** 2) / (H * W)
    centre = v[H // 2, W // 2]
    bent = v + 0.05 * r2[..., None] * (v - centre)                                # a radial term: rays pushed outward with r^2
    bent = bent / bent.norm(dim=-1, keepdim=True)
    with pytest.raises(ValueError, match='pin-hole'):
        mesh_render.camera_from_rays(o, bent)
    with pytest.raises(ValueError, match='origin'):
        mesh_render.camera_from_rays(o + 0.01 * r2[..., None], v)
