"""Mesh export of the NeuS surface on the device: the field on a regular grid through the fused SDF kernel, marching cubes through
csrc/marching_cubes.hip, a binary PLY writer.  Stands in for the reference's `mcubes.marching_cubes` + `trimesh` export
(geo/NeuS-ours2/models/renderer.py:10-36, nerf_runner.py:381-395); conventions: csrc/mc_table.h, DESIGN.md.

An extraction reads the host once (the vertex and triangle totals, to size the outputs); the field never leaves the device.

Clean-up and attributes, also on the device: connected components through csrc/mesh_components.hip
(`components`, `filter_components`: one more host read), per-vertex normals and colours through the fused NeuS kernel
(`vertex_normals`, `vertex_colors`), written by `write_ply` as nx ny nz / red green blue.
"""
import numpy as np
import torch

from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.util.math import safe_l2_normalize

FIELD_SLAB = 1 << 22          # grid points per SDF launch of extract_fields_device


def marching_cubes(u, threshold, origin=None, step=None):
    """Isosurface u = threshold of the device field u [nx,ny,nz] (f32; inside iff u > threshold) -> (verts [V,3] f32, tris [T,3] int32),
    device tensors, in index coordinates -- or, with origin / step (three floats each), at index * step + origin.  Vertices are ordered
    by (owning grid point, axis), triangles by (cell, table order), counter-clockwise seen from outside.  Nothing crossing: shapes (0, 3)."""
    _C.require_device(u, 'marching_cubes')
    u = u.detach()
    if (origin is None) != (step is None):
        raise _C.VqnError('marching_cubes: origin and step come together')
    vcount, tcount = _C.mc_classify(u, threshold)
    n = u.numel()
    vinc, tinc = torch.cumsum(vcount, 0, dtype=torch.int32), torch.cumsum(tcount, 0, dtype=torch.int32)
    if 5 * n >= 1 << 31:                                  # the int32 running sums could wrap: take the totals in int64
        totals = torch.stack([vcount.sum(), tcount.sum()])
    else:
        totals = torch.stack([vinc[-1], tinc[-1]])
    n_verts, n_tris = (int(t) for t in totals.tolist())   # the one host read
    if n_verts >= 1 << 31 or 3 * n_tris >= 1 << 31:
        raise _C.VqnError(f'marching_cubes: {n_verts} vertices / {n_tris} triangles do not fit int32 indices')
    voff, toff = vinc.sub_(vcount), tinc.sub_(tcount)     # exclusive prefix sums
    return _C.mc_emit(u, threshold, voff, toff, n_verts, n_tris, origin, step)


def _axes(bound_min, bound_max, resolution, device):
    # built exactly as models/renderer.py extract_fields builds them (host linspace, then the copy), so the coordinates agree bit for bit
    return [torch.linspace(bound_min[a], bound_max[a], resolution).to(device) for a in range(3)]


@torch.no_grad()
def extract_fields_device(bound_min, bound_max, resolution, sdf_network):
    """u = -sdf on the [resolution]^3 grid between the bounds, a device tensor: bit-identical to
    `extract_fields(bound_min, bound_max, resolution, lambda p: -sdf_network.sdf(p))`, in slabs of at most FIELD_SLAB points through
    the same SDF kernel, with no copy to the host."""
    device = next(sdf_network.parameters()).device
    R = int(resolution)
    X, Y, Z = _axes(bound_min, bound_max, R, device)
    u = torch.empty((R * R * R,), dtype=torch.float32, device=device)
    for s in range(0, R * R * R, FIELD_SLAB):
        lin = torch.arange(s, min(s + FIELD_SLAB, R * R * R), device=device)
        ij = torch.div(lin, R, rounding_mode='floor')
        pts = torch.stack([X[torch.div(ij, R, rounding_mode='floor')], Y[ij % R], Z[lin % R]], -1)
        u[s: s + pts.shape[0]] = sdf_network.sdf(pts).reshape(-1)
    return u.neg_().reshape(R, R, R)


def extract_geometry_device(bound_min, bound_max, resolution, threshold, sdf_network):
    """-> (vertices [V,3] f32 in world coordinates v / (R - 1) * (b_max - b_min) + b_min, triangles [T,3] int32), device tensors."""
    u = extract_fields_device(bound_min, bound_max, resolution, sdf_network)
    b_min = bound_min.detach().cpu().numpy().astype(np.float64)
    b_max = bound_max.detach().cpu().numpy().astype(np.float64)
    return marching_cubes(u, threshold, origin=b_min, step=(b_max - b_min) / (resolution - 1.0))


# ---- clean-up: connected components ----------------------------------------------------------------------------------------------
INFO_SIZES = 16               # component sizes reported by filter_components


def components(triangles, n_verts):
    """labels [n_verts] int32 (device) of the mesh with triangles [T,3] int32 (device): two vertices are connected when a triangle uses
    both, and labels[v] is the smallest vertex index of v's component -- canonical, so equal from run to run.  A vertex no triangle
    uses is its own component; T = 0 gives labels[v] = v.  Indices outside [0, n_verts) are a caller error (such an edge connects
    nothing).  No host read."""
    _C.require_device(triangles, 'components')
    return _C.mesh_components(triangles.detach(), int(n_verts))


def filter_components(vertices, triangles, keep_largest=None, min_faces=None):
    """Drop the small connected pieces of the device mesh (vertices [V,3] f32, triangles [T,3] int32) -> (vertices, triangles, info).

    The size of a component is its number of triangles.  Components are ordered by size, largest first, equal sizes by the smaller
    label (= smallest vertex index).  keep_largest = k keeps the first k, min_faces = m those with at least m triangles; with both, a
    component has to pass both.  Surviving vertices and triangles keep their relative order, triangle indices are rewritten, and
    vertices that no surviving triangle uses are dropped (so a vertex no triangle uses never survives an active filter).  An empty
    result has shapes (0, 3).  info = dict(n_components: components that own at least one triangle, sizes: their sizes in that
    order, at most the first INFO_SIZES, kept: how many survive).

    With neither filter the call is the identity: the same two tensor objects come back, nothing is launched, and info holds None.
    Otherwise: ONE host read (the surviving vertex and triangle totals with the info figures, in one copy), as marching_cubes."""
    if keep_largest is None and min_faces is None:
        return vertices, triangles, dict(n_components=None, sizes=None, kept=None)
    k = None if keep_largest is None else int(keep_largest)
    m = None if min_faces is None else int(min_faces)
    if (k is not None and k < 0) or (m is not None and m < 0):
        raise _C.VqnError(f'filter_components: keep_largest = {keep_largest} / min_faces = {min_faces} must not be negative')
    _C.require_device(triangles, 'filter_components')
    _C.require_device(vertices, 'filter_components')
    vertices, triangles = vertices.detach(), triangles.detach()
    dev = triangles.device
    V, T = vertices.shape[0], triangles.shape[0]
    if V == 0 or T == 0:
        return vertices.new_empty((0, 3)), triangles.new_empty((0, 3)), dict(n_components=0, sizes=[], kept=0)
    labels = _C.mesh_components(triangles, V).long()
    tri_label = labels[triangles[:, 0].long()]
    # triangles by label; 0 at every vertex that is not the root of a piece (integer adds: exact; torch.bincount would read the host)
    size = torch.zeros((V,), dtype=torch.int64, device=dev).scatter_add_(0, tri_label, torch.ones_like(tri_label))
    ids = torch.arange(V, device=dev)
    # order: size descending, then label ascending -- one key, distinct per piece (size <= T < 2^31 / 3, label < V < 2^31: no overflow)
    key = torch.where(size > 0, size * V + (V - 1 - ids), torch.full_like(size, -1))
    order = torch.argsort(key, descending=True)
    keep_label = size > 0
    if k is not None:
        rank = torch.empty_like(order)
        rank[order] = ids
        keep_label &= rank < k
    if m is not None:
        keep_label &= size >= m
    keep_tri = keep_label[tri_label]
    keep_vert = keep_label[labels]                                          # (size > 0: every vertex of such a piece is in a triangle)
    vinc, tinc = torch.cumsum(keep_vert, 0, dtype=torch.int32), torch.cumsum(keep_tri, 0, dtype=torch.int32)
    top = key[order[:INFO_SIZES]]
    figures = torch.cat([torch.stack([vinc[-1].long(), tinc[-1].long(), (size > 0).sum(), keep_label.sum()]),
                         torch.where(top >= 0, torch.div(top, V, rounding_mode='floor'), top)])
    n_v, n_t, n_comp, n_kept, *sizes = figures.tolist()                     # the one host read
    info = dict(n_components=n_comp, sizes=[s for s in sizes if s >= 0], kept=n_kept)
    new_index = vinc.sub_(keep_vert.to(torch.int32))                        # exclusive prefix sums
    tri_offset = tinc.sub_(keep_tri.to(torch.int32))
    out_t = _C.mesh_remap_tris(triangles, keep_tri, tri_offset, new_index, n_t)
    # kept vertex j of the output is input vertex src[j]: a scatter of the kept ids to their new places (the rest go to one spare slot)
    src = torch.zeros((n_v + 1,), dtype=torch.int64, device=dev)
    src.scatter_(0, torch.where(keep_vert, new_index.long(), torch.full_like(ids, n_v)), ids)
    return vertices[src[:n_v]], out_t, info


# ---- attributes: per-vertex normals and colours from the networks ----------------------------------------------------------------
NORMAL_EPS = 1e-6             # safe_l2_normalize's floor under the squared length (decomp/nerfactor/util/math.py)


def _unit(g):
    return safe_l2_normalize(g, axis=-1, eps=NORMAL_EPS)


@torch.no_grad()
def vertex_normals(vertices, sdf_network):
    """[V,3] f32 unit normals at the device vertices: the analytic SDF gradient of the fused kernel (`sdf_network.gradient`),
    g * rsqrt(max(|g|^2, NORMAL_EPS)).  They point towards increasing sdf, outwards, the side the triangles of marching_cubes are
    counter-clockwise from.  In slabs of at most FIELD_SLAB vertices; no host read."""
    _C.require_device(vertices, 'vertex_normals')
    v = vertices.detach().float().contiguous()
    out = torch.empty((v.shape[0], 3), dtype=torch.float32, device=v.device)
    for s in range(0, v.shape[0], FIELD_SLAB):
        out[s: s + FIELD_SLAB] = _unit(sdf_network.gradient(v[s: s + FIELD_SLAB]).squeeze(1))
    return out


@torch.no_grad()
def vertex_colors(vertices, sdf_network, color_network):
    """[V,3] uint8 (red, green, blue) at the device vertices: the colour network seen head-on.  Per slab of at most FIELD_SLAB
    vertices, one fused launch (vqn_neus_fine_points with the colour descriptor) at pts = vertices, dirs = -n with n the unit normal
    of vertex_normals; the kernel hands its own raw gradient to the colour net as `normals`, as render_core does.  Quantised as
    round(clip(c, 0, 1) * 255).  The colour net's channels are (blue, green, red) -- the datasets hold their images in cv2's order
    (models/nerfset.py, models/dtuset.py) and validate_image reverses on write -- so they are reversed here too.  No host read."""
    _C.require_device(vertices, 'vertex_colors')
    if not (sdf_network._hip_supported() and color_network._hip_supported()):
        raise _C.VqnError('vertex_colors: the fused NeuS kernel does not cover this network shape')
    v = vertices.detach().float().contiguous()
    wb_s, d_s = sdf_network.packs(max_tiles=color_network.max_tiles())
    wb_c, d_c = color_network.packs(feat_tiles=sdf_network.plan().tiles[-1])
    out = torch.empty((v.shape[0], 3), dtype=torch.uint8, device=v.device)
    for s in range(0, v.shape[0], FIELD_SLAB):
        pts = v[s: s + FIELD_SLAB]
        dirs = _unit(sdf_network.gradient(pts).squeeze(1)).neg_()
        _, _, c = _C.neus_fine_points(d_s, wb_s, d_c, wb_c, pts=pts, dirs=dirs)
        out[s: s + FIELD_SLAB] = torch.round(c.clip(0.0, 1.0) * 255.0).to(torch.uint8).flip(-1)
    return out


def _host_array(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: `element vertex` with float x, y, z and `element face` with `property list uchar int vertex_indices`
    (the layout trimesh writes for a bare triangle mesh).  vertices [V,3], triangles [T,3]: arrays or tensors.  normals [V,3]: float
    nx, ny, nz after z; colors [V,3] (0..255): uchar red, green, blue after those (trimesh's order, what MeshLab and Blender read)."""
    v = np.ascontiguousarray(_host_array(vertices).reshape(-1, 3), dtype='<f4')
    t = _host_array(triangles).reshape(-1, 3)
    faces = np.empty(len(t), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    faces['n'] = 3
    faces['v'] = t
    fields, props = [('p', '<f4', (3,))], 'property float x\nproperty float y\nproperty float z\n'
    if normals is not None:
        fields.append(('n', '<f4', (3,)))
        props += 'property float nx\nproperty float ny\nproperty float nz\n'
    if colors is not None:
        fields.append(('c', 'u1', (3,)))
        props += 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    rows = np.empty(len(v), dtype=fields)                                   # packed: 12 (+ 12) (+ 3) bytes per vertex
    rows['p'] = v
    for name, a in (('n', normals), ('c', colors)):
        if a is not None:
            a = _host_array(a).reshape(-1, 3)
            if len(a) != len(v):
                raise ValueError(f'write_ply: {len(a)} attribute rows for {len(v)} vertices')
            rows[name] = a
    header = ('ply\nformat binary_little_endian 1.0\n'
              f'element vertex {len(v)}\n' + props +
              f'element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n')
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(rows.tobytes())
        f.write(faces.tobytes())
