"""Plain union-find statement of the mesh components of vqnerf_release_amd/csrc/mesh_components.hip, for the tests of the device
kernels: two vertices are connected when a triangle uses both; the label of a vertex is the smallest vertex index of its component,
so a label array is comparable with the device's by exact equality.  Also the host statement of geo/mesh.py filter_components and the
fields the tests of both share."""
import numpy as np


def components(tris, n_verts):
    """-> labels [n_verts] int32, labels[v] = min of v's component"""
    parent = list(range(n_verts))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(tris).reshape(-1, 3).tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)           # the smaller index stays the root: a root is its tree's minimum
    return np.array([find(v) for v in range(n_verts)], dtype=np.int32)


def partition(labels, names=None):
    """-> the set of components, each a frozenset of vertex names (names[v]; default v itself)"""
    groups = {}
    for v, l in enumerate(np.asarray(labels).tolist()):
        groups.setdefault(l, []).append(v if names is None else int(names[v]))
    return {frozenset(g) for g in groups.values()}


def filter_components(verts, tris, keep_largest=None, min_faces=None):
    """Host statement of mesh.filter_components with an active filter -> (verts, tris, sizes in order, labels kept)"""
    tris = np.asarray(tris).reshape(-1, 3)
    labels = components(tris, len(verts))
    tri_label = labels[tris[:, 0]] if len(tris) else np.zeros(0, np.int32)
    ls, sizes = np.unique(tri_label, return_counts=True)
    order = sorted(zip(ls.tolist(), sizes.tolist()), key=lambda p: (-p[1], p[0]))         # size descending, then the smaller label
    kept = [l for r, (l, s) in enumerate(order) if (keep_largest is None or r < keep_largest) and (min_faces is None or s >= min_faces)]
    keep_tri = np.isin(tri_label, kept)
    keep_vert = np.isin(labels, kept)
    new_index = np.cumsum(keep_vert) - 1
    return verts[keep_vert], new_index[tris[keep_tri]].astype(np.int32), [s for _, s in order], kept


# ---- fields ---------------------------------------------------------------------------------------------------------------------------
def two_spheres(shape=(24, 20, 28)):
    """u [shape] float32, inside iff u > 0: two separate spheres of different size in [-1, 1]^3 on a grid of unequal dimensions"""
    X, Y, Z = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    ball = lambda r, c: r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)
    return np.maximum(ball(0.3, (-0.45, 0.0, 0.0)), ball(0.25, (0.5, 0.3, -0.2))).astype(np.float32)


LATTICE_N = 31                # grid points per axis; sphere (i, j, k) of the 6 x 6 x 6 lattice is centred at index 2.5 + 5 (i, j, k)


def sphere_lattice():
    """u [31,31,31] float32 in index units: 216 spheres, centres 5 cells apart at the centres of cells, radius 1.3 where i + j + k is
    even and 1.8 where it is odd.  Radius 1.3 holds the 8 corners of the centre cell (at 0.87; the next grid points are at 1.66):
    the sphere crosses one full cell.  Radius 1.8 holds those and the 24 points at 1.66 (the next are at 2.18).  Inside points stay
    within 1.5 of a centre, centres are 5 apart and 2.5 from the boundary: no two pieces touch and none is clipped."""
    ax = np.arange(LATTICE_N, dtype=np.float64)
    near = np.clip(np.floor(ax / 5.0), 0, 5)                 # lattice index of the nearest centre along one axis
    d = ax - (2.5 + 5.0 * near)
    D = np.sqrt(d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2)
    odd = (near[:, None, None] + near[None, :, None] + near[None, None, :]) % 2 == 1
    return (np.where(odd, 1.8, 1.3) - D).astype(np.float32)


def strip(n_verts):
    """triangle strip over vertices 0 .. n_verts - 1 along its length -> [n_verts - 2, 3] int32"""
    i = np.arange(n_verts - 2, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], 1)
