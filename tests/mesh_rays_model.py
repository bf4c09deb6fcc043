"""The plain statement of the mesh ray caster (include/vqn_mesh_rays.h) in numpy float32: which triangles are kept and the counters of
the dropped ones, the triangles listed per grid cell, and the queries -- cast, occluded, light_visibility -- by brute force over ALL kept
triangles: there is no grid in the model's queries, so the device's walk is judged by what it must find.  Every product and sum is one
float32 numpy operation, so it rounds on its own as the kernel's (fp contraction off) does.  The loops run over the triangles; the rays
are the array axis.  Helpers only, no tests."""
import numpy as np

F = np.float32
STATS = 3
MARGIN = F(1.0 / 16.0)
MIN_DIR = F(2.0 ** -60)
MISS_KEY = (np.uint64(0x7f800000) << np.uint64(32)) | np.uint64(0xffffffff)


def cross(a, b):
    """a x b, components fl(fl(a.y b.z) - fl(a.z b.y)) ...; a, b: tuples of three float32 arrays or scalars"""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def classify(verts, tris):
    """-> (cause int [T]: 0 kept, else 1 + the slot of stats; stats int32 [3])"""
    verts, tris = np.asarray(verts, F).reshape(-1, 3), np.asarray(tris, np.int32).reshape(-1, 3)
    V = verts.shape[0]
    cause = np.zeros(tris.shape[0], np.int32)
    for t, (a, b, c) in enumerate(tris):
        if not all(0 <= i < V for i in (a, b, c)):
            cause[t] = 1
            continue
        v0, v1, v2 = verts[a], verts[b], verts[c]
        if not (np.isfinite(v0).all() and np.isfinite(v1).all() and np.isfinite(v2).all()):
            cause[t] = 2
            continue
        n = cross(v1 - v0, v2 - v0)
        if n[0] == 0 and n[1] == 0 and n[2] == 0:
            cause[t] = 3
    return cause, np.array([(cause == k + 1).sum() for k in range(STATS)], np.int32)


def cell_clamp(x, n):
    """floor(x) clamped into [0, n - 1], the clamp in float32"""
    return int(np.minimum(np.maximum(np.floor(F(x)), F(0)), F(n - 1)))


def cell_counts(verts, tris, origin, h, dims):
    """-> int32 [cells]: the kept triangles listed in each cell (x fastest)"""
    verts, tris = np.asarray(verts, F).reshape(-1, 3), np.asarray(tris, np.int32).reshape(-1, 3)
    origin, h = np.asarray(origin, F), F(h)
    cause, _ = classify(verts, tris)
    count = np.zeros((dims[2], dims[1], dims[0]), np.int32)
    for t in np.nonzero(cause == 0)[0]:
        v = verts[tris[t]]
        lo, hi = v.min(0), v.max(0)
        c0 = [cell_clamp((lo[a] - origin[a]) / h - MARGIN, dims[a]) for a in range(3)]
        c1 = [cell_clamp((hi[a] - origin[a]) / h + MARGIN, dims[a]) for a in range(3)]
        count[c0[2]:c1[2] + 1, c0[1]:c1[1] + 1, c0[0]:c1[0] + 1] += 1
    return count.reshape(-1)


def ray_valid(o, d, tmin, tmax):
    with np.errstate(invalid='ignore'):
        dmax = np.abs(d).max(1)
        return (np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(tmin) & (tmin >= 0) & (tmin < tmax) & (dmax >= MIN_DIR))


def hit(v0, v1, v2, o, d, tmin, tmax):
    """the statement of a hit of rays (o, d [n, 3]; tmin, tmax [n]) on one triangle -> (hit bool [n], t, u, v float32 [n])"""
    with np.errstate(all='ignore'):
        e1, e2 = v1 - v0, v2 - v0
        dd = (d[:, 0], d[:, 1], d[:, 2])
        p = cross(dd, e2)
        det = dot3(e1, p)
        inv = F(1) / det
        s = (o[:, 0] - v0[0], o[:, 1] - v0[1], o[:, 2] - v0[2])
        u = dot3(s, p) * inv
        q = cross(s, e1)
        v = dot3(dd, q) * inv
        t = dot3(e2, q) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & ((u + v) <= 1) & (t > tmin) & (t < tmax)
    return ok, t, u, v


def _rays(o, d, tmin, tmax):
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    n = o.shape[0]
    return o, d, np.broadcast_to(np.asarray(tmin, F), (n,)).copy(), np.broadcast_to(np.asarray(tmax, F), (n,)).copy()


def cast(verts, tris, o, d, tmin=0.0, tmax=np.inf):
    """-> dict(face int32 [n], t float32 [n], uv float32 [n, 2]): the least key (bits of t, face) over every kept triangle"""
    verts, tris = np.asarray(verts, F).reshape(-1, 3), np.asarray(tris, np.int32).reshape(-1, 3)
    o, d, tmin, tmax = _rays(o, d, tmin, tmax)
    n = o.shape[0]
    cause, _ = classify(verts, tris)
    valid = ray_valid(o, d, tmin, tmax)
    key = np.full(n, MISS_KEY, np.uint64)
    uv = np.zeros((n, 2), F)
    for f in np.nonzero(cause == 0)[0]:
        ok, t, u, v = hit(verts[tris[f, 0]], verts[tris[f, 1]], verts[tris[f, 2]], o, d, tmin, tmax)
        k = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        better = ok & valid & (k < key)
        key[better] = k[better]
        uv[better, 0], uv[better, 1] = u[better], v[better]
    return {'face': (key & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32), 't': (key >> np.uint64(32)).astype(np.uint32).view(F),
            'uv': uv}


def occluded(verts, tris, o, d, tmin=0.0, tmax=np.inf):
    """-> bool [n]: any kept triangle is hit"""
    verts, tris = np.asarray(verts, F).reshape(-1, 3), np.asarray(tris, np.int32).reshape(-1, 3)
    o, d, tmin, tmax = _rays(o, d, tmin, tmax)
    cause, _ = classify(verts, tris)
    valid = ray_valid(o, d, tmin, tmax)
    occ = np.zeros(o.shape[0], bool)
    for f in np.nonzero(cause == 0)[0]:
        occ |= hit(verts[tris[f, 0]], verts[tris[f, 1]], verts[tris[f, 2]], o, d, tmin, tmax)[0] & valid
    return occ


def light_rays(points, normals, lights, bias):
    """the rays of every (point, light) as the header builds them -> (o [n, L, 3], d [n, L, 3], dist [n, L], front bool [n, L])"""
    p, nrm, l = (np.asarray(a, F).reshape(-1, 3) for a in (points, normals, lights))
    with np.errstate(all='ignore'):
        o = p + F(bias) * nrm
        dl = l[None, :, :] - o[:, None, :]
        dist = np.sqrt((dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2])
        d = dl / dist[..., None]
        front = ((d[..., 0] * nrm[:, None, 0] + d[..., 1] * nrm[:, None, 1]) + d[..., 2] * nrm[:, None, 2]) > 0
    return np.broadcast_to(o[:, None, :], d.shape), d, dist, front


def light_visibility(verts, tris, points, normals, lights, bias):
    """-> float32 [n, L]: 1 iff the light is in front of the point and the segment to it hits no kept triangle"""
    o, d, dist, front = light_rays(points, normals, lights, bias)
    occ = occluded(verts, tris, o.reshape(-1, 3), d.reshape(-1, 3), 0.0, dist.reshape(-1)).reshape(front.shape)
    return (front & ~occ).astype(F)


# ---- meshes the tests share ---------------------------------------------------------------------------------------------------------------
def icosahedron():
    g = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1],
                  [-g, 0, -1], [-g, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    return v / np.linalg.norm(v, axis=1, keepdims=True), f


def icosphere(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """-> (verts float32 [V, 3] on the sphere, tris int32 [20 * 4^s, 3]), closed, every edge shared by exactly two faces"""
    v, f = icosahedron()
    v = [tuple(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = (np.array(v[a]) + np.array(v[b])) / 2
                v.append(tuple(p / np.linalg.norm(p)))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = np.array(nf, np.int32)
    return (np.array(v) * radius + np.array(centre)).astype(F), np.asarray(f, np.int32)


def two_spheres():
    """the analytic scene: icospheres of radius 0.5 at the origin and 0.45 at (0, 0, 1.1), 320 faces each; 600 points on the first with
    their normals, 48 lights at radius 4; bias 0.02 -> dict"""
    va, fa = icosphere(2, 0.5)
    vb, fb = icosphere(2, 0.45, (0.0, 0.0, 1.1))
    rng = np.random.default_rng(0)
    n = rng.normal(size=(600, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    l = rng.normal(size=(48, 3))
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    return {'verts': np.concatenate([va, vb]), 'tris': np.concatenate([fa, fb + va.shape[0]]).astype(np.int32),
            'points': (0.5 * n).astype(F), 'normals': n.astype(F), 'lights': (4.0 * l).astype(F), 'bias': 0.02,
            'spheres': [((0.0, 0.0, 0.0), 0.5), ((0.0, 0.0, 1.1), 0.45)]}


def two_spheres_truth(scene, band=0.01):
    """float64, from the header's own rays: -> (front bool [n, L], occluded bool [n, L], skipped bool [n, L]: the closest approach of
    the segment to a sphere's centre is within `band` of its radius)"""
    o, d, dist, front = light_rays(scene['points'], scene['normals'], scene['lights'], scene['bias'])
    o, d, dist = o.astype(np.float64), d.astype(np.float64), dist.astype(np.float64)
    occ = np.zeros(front.shape, bool)
    skip = np.zeros(front.shape, bool)
    for c, r in scene['spheres']:
        oc = np.asarray(c)[None, None, :] - o
        s = np.clip((oc * d).sum(-1) / (d * d).sum(-1), 0.0, dist)
        closest = np.linalg.norm(oc - s[..., None] * d, axis=-1)
        occ |= closest < r
        skip |= np.abs(closest - r) < band
    return front, occ, skip
