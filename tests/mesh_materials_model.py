"""The plain statement of include/vqn_mesh_materials.h in NumPy and Python loops over triangles and vertices: the label clean-up, the
face codes and the split by code, following the header's definitions literally -- no sorting tricks, no prefix sums -- plus a numpy
union-find for the region counts and an icosphere for CPU use.  Helpers only, no tests."""
import numpy as np


def _valid_tri(t, V):
    return all(0 <= int(i) < V for i in t)


def label_mode(tris, codes, K, self_weight=1, iters=1):
    """-> (codes after `iters` rounds, changed [iters])"""
    tris, cur = np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(codes, np.int64).copy()
    V = len(cur)
    changed = []
    for _ in range(iters):
        votes = np.zeros((V, K), np.int64)
        for t in tris:
            if not _valid_tri(t, V):
                continue
            for i in range(3):
                for other in (t[(i + 1) % 3], t[(i + 2) % 3]):
                    if 0 <= cur[other] < K:
                        votes[t[i], cur[other]] += 1
        new = cur.copy()
        for v in range(V):
            if 0 <= cur[v] < K:
                votes[v, cur[v]] += self_weight
            top = votes[v].max() if K else 0
            if top == 0:
                continue                                   # no vote at all: the vertex keeps its code
            if 0 <= cur[v] < K and votes[v, cur[v]] == top:
                continue
            new[v] = int(np.flatnonzero(votes[v] == top)[0])
        changed.append(int((new != cur).sum()))
        cur = new
    return cur.astype(np.int32), np.array(changed, np.int32)


def face_code(a, b, c):
    if a == b or a == c:
        return a
    if b == c:
        return b
    return min(a, b, c)


def face_codes(tris, codes, K):
    tris, codes = np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(codes, np.int64)
    V = len(codes)
    out = np.full(len(tris), -1, np.int32)
    for j, t in enumerate(tris):
        if _valid_tri(t, V) and all(0 <= codes[i] < K for i in t):
            out[j] = face_code(*[int(codes[i]) for i in t])
    return out


def split(tris, codes, K):
    """-> dict with the arrays of mesh.split_by_label"""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    fc = face_codes(tris, codes, K)
    face_src, vert_src, tris_local, face_offset, vert_offset = [], [], [], [0], [0]
    for k in range(K):
        faces = [j for j in range(len(tris)) if fc[j] == k]
        used = set()
        for j in faces:
            used.update(int(i) for i in tris[j])
        verts = [v for v in range(len(codes)) if v in used]
        rank = {v: r for r, v in enumerate(verts)}
        face_src += faces
        vert_src += verts
        tris_local += [[rank[int(i)] for i in tris[j]] for j in faces]
        face_offset.append(len(face_src))
        vert_offset.append(len(vert_src))
    return dict(face_code=fc, face_src=np.array(face_src, np.int32), vert_src=np.array(vert_src, np.int32),
                tris_local=np.array(tris_local, np.int32).reshape(-1, 3), face_offset=face_offset, vert_offset=vert_offset,
                face_count=list(np.diff(face_offset)), vert_count=list(np.diff(vert_offset)), n_faces=len(face_src),
                n_slots=len(vert_src), dropped=len(tris) - len(face_src))


def region_counts(tris, codes, K):
    """per code the connected regions: union-find over the vertices the triangles use, joined along triangle edges whose ends share a code"""
    tris, codes = np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(codes, np.int64)
    parent = list(range(len(codes)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    used = set()
    for t in tris:
        used.update(int(i) for i in t)
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            if codes[a] == codes[b]:
                ra, rb = find(int(a)), find(int(b))
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    out = [0] * K
    for r in {find(v) for v in used}:
        if 0 <= codes[r] < K:
            out[int(codes[r])] += 1
    return out


def icosphere(level=1):
    """-> (vertices float32 [V, 3] on the unit sphere, triangles int32 [T, 3], counter-clockwise from outside): an icosahedron, every
    triangle cut in four `level` times (V = 10 * 4^level + 2, T = 20 * 4^level)"""
    p = (1 + 5 ** 0.5) / 2
    verts = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
             (-p, 0, -1), (-p, 0, 1)]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in verts]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in tris:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = out
    return np.array(verts, np.float32), np.array(tris, np.int32)
