"""Plain-loop NumPy statement of the project's marching cubes (conventions: vqnerf_release_amd/csrc/mc_table.h), for the tests of the
device kernels: same table (parsed from the header as text), same vertex and triangle order, the same interpolation formula in a
chosen float type (float32 to compare with the kernels, float64 to measure what the discretisation alone costs)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'vqnerf_release_amd', 'csrc', 'mc_table.h')


def parse_header(path=HEADER):
    """-> (tri_count [256], tri_edges [256,15], edge_mask [256]) as int arrays"""
    txt = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)

    def body(name):
        m = re.search(name + r'(?:\[\d+\])+\s*=\s*\{(.*?)\};', txt, flags=re.S)
        return [int(t, 0) for t in re.findall(r'-?(?:0x[0-9a-fA-F]+|\d+)', m.group(1))]
    return (np.array(body('vqn_mc_tri_count')), np.array(body('vqn_mc_tri_edges')).reshape(256, 15), np.array(body('vqn_mc_edge_mask')))


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_owner(e):
    """edge e = 4 axis + (lo + 2 hi) -> (offset of its low corner, axis)"""
    a, k = divmod(e, 4)
    off = [0, 0, 0]
    others = [b for b in range(3) if b != a]
    off[others[0]], off[others[1]] = k & 1, k >> 1
    return tuple(off), a


def marching_cubes(u, threshold, dtype=np.float32):
    """-> (verts [V,3] dtype in index coordinates, tris [T,3] int32)"""
    tri_count, tri_edges, _ = parse_header()
    u = np.asarray(u, dtype=dtype)
    thr = dtype(threshold)
    inside = u > thr
    shape = u.shape
    # vertices: grid points in linear (C) order, axes in order, edges whose far end is inside the grid
    owns = np.zeros(shape + (3,), bool)
    owns[:-1, :, :, 0] = inside[:-1] != inside[1:]
    owns[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    owns[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    vid, verts = {}, []
    for i, j, k in np.argwhere(owns.any(-1)):
        for a in range(3):
            if not owns[i, j, k, a]:
                continue
            far = [i, j, k]
            far[a] += 1
            u0, u1 = u[i, j, k], u[tuple(far)]
            t = (thr - u0) / (u1 - u0)
            pos = [dtype(i), dtype(j), dtype(k)]
            pos[a] = pos[a] + t
            vid[(i, j, k, a)] = len(verts)
            verts.append(pos)
    # triangles: cells in linear order of their minimum corner, table order
    case = np.zeros(tuple(s - 1 for s in shape), np.int64)
    for c in range(8):
        x, y, z = corner_offset(c)
        case += inside[x: shape[0] - 1 + x, y: shape[1] - 1 + y, z: shape[2] - 1 + z].astype(np.int64) << c
    tris = []
    for i, j, k in np.argwhere(tri_count[case] > 0):
        c = case[i, j, k]
        for t in range(tri_count[c]):
            tri = []
            for e in tri_edges[c, 3 * t: 3 * t + 3]:
                (x, y, z), a = edge_owner(int(e))
                tri.append(vid[(i + x, j + y, k + z, a)])
            tris.append(tri)
    return np.array(verts, dtype=dtype).reshape(-1, 3), np.array(tris, dtype=np.int32).reshape(-1, 3)


# ---- properties of an indexed triangle mesh -------------------------------------------------------------------------------------
def directed_edge_counts(tris):
    """-> {(a, b): times the directed edge a -> b occurs in a triangle}"""
    out = {}
    for t in np.asarray(tris):
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            out[(int(a), int(b))] = out.get((int(a), int(b)), 0) + 1
    return out


def boundary_and_bad_edges(tris):
    """-> (undirected edges used once, undirected edges that are neither used once nor exactly twice in opposite directions)"""
    d = directed_edge_counts(tris)
    once, bad = [], []
    for a, b in {(min(k), max(k)) for k in d}:
        f, r = d.get((a, b), 0), d.get((b, a), 0)
        if f + r == 1:
            once.append((a, b))
        elif not (f == 1 and r == 1):
            bad.append((a, b))
    return once, bad


def euler_characteristic(n_verts, tris):
    d = directed_edge_counts(tris)
    return n_verts - len({(min(k), max(k)) for k in d}) + len(tris)


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


def area(verts, tris):
    v = np.asarray(verts, np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
