"""The plain statement of the mesh rasteriser (include/vqn_mesh_raster.h, csrc/mesh_raster.hip): numpy float32 / float64 scalars in the
stated order, Python ints for the edge functions, one loop over all triangles per pixel, no tiles.  The kernel equals it bit for bit
(tests/test_gpu_mesh_raster.py); tests/test_mesh_raster_model.py holds the model itself to an independent ray caster.  Helpers only."""
import numpy as np

SUBPIXEL = 256
COORD_LIMIT = 1 << 23
STATS = 4                         # bad index, unusable vertex, zero area, culled

f32, f64 = np.float32, np.float64


def project(verts, P, near):
    """-> [(X, Y, w) | None per vertex]: Python ints and an np.float32; None: not usable"""
    P = np.asarray(P, f32)
    out = []
    with np.errstate(all='ignore'):
        for x, y, z in np.asarray(verts, f32).reshape(-1, 3):
            h = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
            w = h[2]
            fx, fy = (h[0] / w) * f32(SUBPIXEL), (h[1] / w) * f32(SUBPIXEL)
            usable = bool(np.isfinite(w)) and bool(w >= f32(near)) and bool(abs(fx) < f32(COORD_LIMIT)) and bool(abs(fy) < f32(COORD_LIMIT))
            out.append((int(np.rint(fx)), int(np.rint(fy)), w) if usable else None)
    return out


def setup(tris, pverts, cull):
    """-> (kept: [(face, (X, Y) x 3, (w) x 3, s, |area2|)], stats [4])"""
    V = len(pverts)
    kept, stats = [], [0] * STATS
    for t, idx in enumerate(np.asarray(tris).reshape(-1, 3).tolist()):
        if not all(0 <= i < V for i in idx):
            stats[0] += 1
            continue
        pv = [pverts[i] for i in idx]
        if any(p is None for p in pv):
            stats[1] += 1
            continue
        (X0, Y0, _), (X1, Y1, _), (X2, Y2, _) = pv
        area2 = (X1 - X0) * (Y2 - Y0) - (X2 - X0) * (Y1 - Y0)
        if area2 == 0:
            stats[2] += 1
            continue
        s = 1 if area2 > 0 else -1
        if s == cull:
            stats[3] += 1
            continue
        kept.append((t, [(p[0], p[1]) for p in pv], [p[2] for p in pv], s, abs(area2)))
    return kept, stats


def edges(xy, s, px, py):
    """-> (E [3], owns [3]) at the sample (px, py) in sub-pixel units; edge k runs from corner k + 1 to corner k + 2"""
    E, owns = [], []
    for k in range(3):
        (xs, ys), (xe, ye) = xy[(k + 1) % 3], xy[(k + 2) % 3]
        E.append(s * ((xe - xs) * (py - ys) - (ye - ys) * (px - xs)))
        dx, dy = s * (xe - xs), s * (ye - ys)
        owns.append(dy > 0 or (dy == 0 and dx < 0))
    return E, owns


def covered(E, owns):
    return all(e > 0 or (e == 0 and o) for e, o in zip(E, owns))


def shade(E, w, area_abs):
    """-> (depth f32, bary [3] f32) of a covered sample"""
    q = [f64(1.0) / f64(wk) for wk in w]
    S = (f64(E[0]) * q[0] + f64(E[1]) * q[1]) + f64(E[2]) * q[2]
    return f32(f64(area_abs) / S), [f32((f64(E[k]) * q[k]) / S) for k in range(3)]


def rasterize(verts, tris, P, H, W, near=1e-3, cull=0, coverage=None):
    """-> dict(face int32 [H, W], depth f32 [H, W], bary f32 [H, W, 3], stats int32 [4]).  coverage: an int array [H, W] that receives
    the number of triangles that cover each sample."""
    kept, stats = setup(tris, project(verts, P, near), cull)
    face = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), np.inf, f32)
    bary = np.zeros((H, W, 3), f32)
    boxes = [(min(x for x, _ in xy), max(x for x, _ in xy), min(y for _, y in xy), max(y for _, y in xy)) for _, xy, _, _, _ in kept]
    for i in range(H):
        py = SUBPIXEL * i
        row = [n for n, b in enumerate(boxes) if b[2] <= py <= b[3]]          # (a sample outside the box has a negative edge function)
        for j in range(W):
            px = SUBPIXEL * j
            best = None
            for n in row:
                if not boxes[n][0] <= px <= boxes[n][1]:
                    continue
                t, xy, w, s, area_abs = kept[n]
                E, owns = edges(xy, s, px, py)
                if not covered(E, owns):
                    continue
                if coverage is not None:
                    coverage[i, j] += 1
                d, b = shade(E, w, area_abs)
                key = (int(np.asarray(d, f32).view(np.uint32)) << 32) | t
                if best is None or key < best[0]:
                    best = (key, t, d, b)
            if best is not None:
                face[i, j], depth[i, j], bary[i, j] = best[1], best[2], best[3]
    return dict(face=face, depth=depth, bary=bary, stats=np.asarray(stats, np.int32))


def interpolate(face, bary, tris, attr, background, nearest=False):
    """-> f32 [H, W, C]: (b0 a0 + b1 a1) + b2 a2, or the attribute of the corner with the largest b (ties to the lowest corner)"""
    attr, tris = np.asarray(attr, f32), np.asarray(tris).reshape(-1, 3)
    H, W = face.shape
    V, C = attr.shape
    out = np.empty((H, W, C), f32)
    out[:] = np.asarray(background, f32)
    for i in range(H):
        for j in range(W):
            f = int(face[i, j])
            if not 0 <= f < len(tris) or not all(0 <= int(v) < V for v in tris[f]):
                continue
            b = bary[i, j]
            a = [attr[int(v)] for v in tris[f]]
            if nearest:
                k = 0 if (b[0] >= b[1] and b[0] >= b[2]) else (1 if b[1] >= b[2] else 2)
                out[i, j] = a[k]
            else:
                out[i, j] = (b[0] * a[0] + b[1] * a[1]) + b[2] * a[2]
    return out
