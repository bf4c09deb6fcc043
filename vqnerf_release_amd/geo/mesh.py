"""Mesh export of the NeuS surface on the device: the field on a regular grid through the fused SDF kernel, marching cubes through
csrc/marching_cubes.hip, a binary PLY writer.  Stands in for the reference's `mcubes.marching_cubes` + `trimesh` export
(geo/NeuS-ours2/models/renderer.py:10-36, nerf_runner.py:381-395); conventions: csrc/mc_table.h, DESIGN.md.

An extraction reads the host once (the vertex and triangle totals, to size the outputs); the field never leaves the device.

Clean-up and attributes, also on the device: connected components through csrc/mesh_components.hip
(`components`, `filter_components`: one more host read), per-vertex normals and colours through the fused NeuS kernel
(`vertex_normals`, `vertex_colors`), written by `write_ply` as nx ny nz / red green blue.

The sparse route (`plan_bricks`, `marching_cubes_bricks`, `extract_geometry_sparse`; csrc/marching_cubes_bricks.hip) evaluates the
network only on the 8^3-cell bricks the surface can pass through and returns the same bytes, also at resolutions the dense route
refuses; it reads the host twice.

For scoring a mesh (geo/geometry_eval.py): `read_ply` reads what `write_ply` writes and point-cloud files,
`sample_surface` draws points of the surface uniformly by area through csrc/geometry_eval.hip.

Material codes on the mesh (decomp/material_mesh.py): `smooth_labels` cleans per-vertex codes up by majority
vote over the mesh, `face_labels` gives one code per face, `split_by_label` cuts the mesh into one sub-mesh per code with a compact
vertex list each (csrc/mesh_materials.hip: integer kernels, one host read); `write_ply(extra=...)` / `read_ply(extra=...)` carry scalar
vertex properties, `write_obj` / `write_mtl` write the faces grouped by material.
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


# ---- the sparse route: only the bricks the surface can pass through (csrc/marching_cubes_bricks.hip) --------
BRICK = _C.BRICK_CELLS        # 8 cells per brick and axis; a brick stores (BRICK + 1)^3 points, its faces on both sides


def plan_bricks(resolution, brick=BRICK, axes=None):
    """How a grid of `resolution` points per axis (an int, or (nx, ny, nz)) is cut into bricks of `brick` cells.  Per axis a, as
    integer NumPy arrays: nb[a] = ceil((n - 1) / brick) bricks; brick b stores the points lo[a][b] .. hi[a][b] = brick * b ..
    min(brick * b + brick, n - 1) (the last brick is clipped to 1..brick cells; faces are stored on both sides); grid point i belongs
    to brick owner[a][i] = min(i // brick, nb - 1), a cell to the brick of its minimum corner, so every point has one owner and every
    cell lies in one brick with all 8 corners stored there; centre[a][b] = lo + (hi - lo) // 2 is the grid index of the brick's centre.
    With axes (the three coordinate arrays of the grid, as _axes builds them on the host): h [nbx,nby,nbz] float32, the largest
    distance from a brick's centre point to a stored corner of it, formed in float64 from those coordinates and rounded up."""
    from types import SimpleNamespace
    dims = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(d) for d in resolution)
    brick = int(brick)
    if len(dims) != 3 or min(dims) < 2 or brick < 1:
        raise ValueError(f'plan_bricks: three dimensions >= 2 and brick >= 1, got {dims}, {brick}')
    nb, lo, hi, centre, owner = [], [], [], [], []
    for n in dims:
        k = -(-(n - 1) // brick)
        l = np.arange(k, dtype=np.int64) * brick
        u = np.minimum(l + brick, n - 1)
        nb.append(k); lo.append(l); hi.append(u); centre.append(l + (u - l) // 2)
        owner.append(np.minimum(np.arange(n, dtype=np.int64) // brick, k - 1))
    plan = SimpleNamespace(dims=dims, brick=brick, nb=tuple(nb), lo=lo, hi=hi, centre=centre, owner=owner, h=None)
    if axes is not None:
        d2 = []
        for a in range(3):
            x = np.asarray(axes[a], dtype=np.float64)
            d2.append(np.maximum(np.abs(x[lo[a]] - x[centre[a]]), np.abs(x[hi[a]] - x[centre[a]])) ** 2)
        h64 = np.sqrt(d2[0][:, None, None] + d2[1][None, :, None] + d2[2][None, None, :])
        h32 = h64.astype(np.float32)
        # up: one float32 step wherever the rounded value is not already above (which also covers the roundings of the float64 sum)
        plan.h = np.where(h32.astype(np.float64) > h64, h32, np.nextafter(h32, np.float32(np.inf)))
    return plan


def _brick_grid(dims):
    """-> (dims, bricks per axis); dimensions < 2 are left to the library to refuse (they count as one brick here)"""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3:
        raise _C.VqnError(f'marching cubes on bricks: three dimensions, got {dims}')
    nb = tuple(max(1, -(-(d - 1) // BRICK)) for d in dims)
    if nb[0] * nb[1] * nb[2] >= 1 << 31:
        raise _C.VqnError(f'marching cubes on bricks: the brick grid {nb} must have < 2^31 entries')
    return dims, nb


def _mark(marks, name):
    """stage boundary for scripts/probe_mesh_sparse.py: (name of the stage that ends here, a recorded HIP event)"""
    if marks is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))


def brick_offsets(ub, brick_ijk, dims, threshold, marks=None):
    """The classify half of marching_cubes_bricks -> (slot, vert_offset, tri_offset, n_verts, n_tris, leaks): the slot map of the
    list, the exclusive prefix sums of the counts in the dense order (int32 [n * 729], stored at the brick entries), both totals and
    the leak count.  One device sort of the owned points' int64 keys, two prefix sums, ONE host read."""
    dims, nb = _brick_grid(dims)
    n = brick_ijk.shape[0]
    if n * _C.BRICK_POINTS >= 1 << 31:
        raise _C.VqnError(f'marching cubes on bricks: {n} bricks: n * 729 must be < 2^31')
    dev = ub.device
    b = brick_ijk.long()
    lin = ((b[:, 0] * nb[1] + b[:, 1]) * nb[2] + b[:, 2]).clamp_(0, nb[0] * nb[1] * nb[2] - 1)     # (a row outside the grid: caller error)
    slot = torch.full((nb[0] * nb[1] * nb[2],), -1, dtype=torch.int32, device=dev)
    slot[lin] = torch.arange(n, dtype=torch.int32, device=dev)
    vcount, tcount, keys, leaks = _C.mc_brick_classify(ub, brick_ijk, slot, dims, threshold)
    _mark(marks, 'classify')
    # the dense order: owned points by linear index (entries that are no owned point sort last and count nothing)
    order = torch.argsort(keys)
    del keys
    vs, ts = vcount[order].long(), tcount[order].long()
    vinc, tinc = torch.cumsum(vs, 0), torch.cumsum(ts, 0)
    n_verts, n_tris, n_leaks = torch.stack([vinc[-1], tinc[-1], leaks[0].long()]).tolist()      # the one host read
    if n_verts >= 1 << 31 or 3 * n_tris >= 1 << 31:
        raise _C.VqnError(f'marching cubes on bricks: {n_verts} vertices / {n_tris} triangles do not fit int32 indices')
    voff, toff = vcount, tcount                                                                   # (reused) back in brick order
    voff[order] = vinc.sub_(vs).to(torch.int32)
    toff[order] = tinc.sub_(ts).to(torch.int32)
    _mark(marks, 'sort_and_sums')
    return slot, voff, toff, n_verts, n_tris, n_leaks


def marching_cubes_bricks(ub, brick_ijk, dims, threshold, origin=None, step=None, marks=None):
    """marching_cubes of the field on a grid of dims = (nx, ny, nz) points, from its values on a list of bricks alone ->
    (verts, tris, leaks).  brick_ijk [n,3] int32 (device): brick coordinates, sorted by brick linear index, each once; ub [n,9,9,9]
    f32: the field on each brick's stored points (plan_bricks; entries past a clipped brick's extent are never read).  If every
    cell the surface passes through lies in a listed brick, verts and tris equal marching_cubes(u, threshold, origin, step) of the
    dense field bit for bit, in its order.  leaks (an int) counts the (brick, face) pairs where the surface runs into a brick that is
    not listed; with leaks > 0 the mesh is not the dense one (triangles at such a face hold index 0 in place of the missing vertex).
    One host read (both totals and leaks, in one copy).  marks: a list that receives (stage, HIP event) at every stage boundary."""
    _C.require_device(ub, 'marching_cubes_bricks')
    ub = ub.detach()
    if (origin is None) != (step is None):
        raise _C.VqnError('marching_cubes_bricks: origin and step come together')
    if brick_ijk.shape[0] == 0:
        _brick_grid(dims)
        return (torch.empty((0, 3), dtype=torch.float32, device=ub.device), torch.empty((0, 3), dtype=torch.int32, device=ub.device), 0)
    slot, voff, toff, n_verts, n_tris, leaks = brick_offsets(ub, brick_ijk, dims, threshold, marks)
    verts, tris = _C.mc_brick_emit(ub, brick_ijk, slot, dims, threshold, voff, toff, n_verts, n_tris, origin, step)
    _mark(marks, 'emit')
    return verts, tris, leaks


@torch.no_grad()
def extract_geometry_sparse(bound_min, bound_max, resolution, threshold, sdf_network, lipschitz=2.0, marks=None):
    """extract_geometry_device through the bricks the surface can pass through alone -> (vertices, triangles, info), the same bytes.

    u = -sdf is evaluated at every brick's centre point c; a brick is active iff |u(c) - threshold| <= lipschitz * h, h the largest
    distance from c to a stored point of the brick (plan_bricks).  If |sdf(x) - sdf(y)| <= lipschitz |x - y| an inactive brick has all
    its points on one side and owns no vertex and no triangle, so meshing the active bricks gives the dense mesh.  The field is then
    evaluated on the active bricks' points only.  Should the bound not hold -- the surface runs from an active brick into an inactive
    one -- VqnError is raised and no mesh returned; what cannot be seen is a closed piece lying wholly inside inactive bricks, which the
    premise excludes.  info = dict(bricks_total, bricks_active, points_evaluated, leaks).  Host reads: the active count, then the
    totals with the leak count.  marks: as marching_cubes_bricks."""
    device = next(sdf_network.parameters()).device
    R = int(resolution)
    _mark(marks, 'start')
    axes_host = [torch.linspace(bound_min[a], bound_max[a], R) for a in range(3)]                # as _axes
    X, Y, Z = [a.to(device) for a in axes_host]
    plan = plan_bricks(R, BRICK, axes=[a.numpy() for a in axes_host])
    dims, nb = _brick_grid(plan.dims)
    n_total = nb[0] * nb[1] * nb[2]
    cx, cy, cz = [torch.from_numpy(c).to(device) for c in plan.centre]
    uc = torch.empty((n_total,), dtype=torch.float32, device=device)
    for s in range(0, n_total, FIELD_SLAB):
        lin = torch.arange(s, min(s + FIELD_SLAB, n_total), device=device)
        bij = torch.div(lin, nb[2], rounding_mode='floor')
        pts = torch.stack([X[cx[torch.div(bij, nb[1], rounding_mode='floor')]], Y[cy[bij % nb[1]]], Z[cz[lin % nb[2]]]], -1)
        uc[s: s + pts.shape[0]] = sdf_network.sdf(pts).reshape(-1)
    uc.neg_()
    h = torch.from_numpy(plan.h).to(device).reshape(-1)
    active = (uc.double() - float(threshold)).abs() <= float(lipschitz) * h.double()
    lin = torch.nonzero(active).reshape(-1)                                                       # host read: the active count
    n = lin.shape[0]
    _mark(marks, 'centres')
    info = dict(bricks_total=n_total, bricks_active=n, points_evaluated=n_total + n * _C.BRICK_POINTS, leaks=0)
    if n * _C.BRICK_POINTS >= 1 << 31:
        raise _C.VqnError(f'extract_geometry_sparse: {n} active bricks: n * 729 must be < 2^31; lower lipschitz = {lipschitz} or the resolution')
    bij = torch.div(lin, nb[2], rounding_mode='floor')
    brick_ijk = torch.stack([torch.div(bij, nb[1], rounding_mode='floor'), bij % nb[1], lin % nb[2]], -1).to(torch.int32).contiguous()
    ub = torch.empty((n * _C.BRICK_POINTS,), dtype=torch.float32, device=device)
    _mark(marks, 'brick_list')
    for s in range(0, n * _C.BRICK_POINTS, FIELD_SLAB):
        pts = _C.mc_brick_points((X, Y, Z), dims, brick_ijk, s, min(FIELD_SLAB, n * _C.BRICK_POINTS - s))
        ub[s: s + pts.shape[0]] = sdf_network.sdf(pts).reshape(-1)
    _mark(marks, 'brick_field')
    ub = ub.neg_().reshape(n, BRICK + 1, BRICK + 1, BRICK + 1)
    b_min = bound_min.detach().cpu().numpy().astype(np.float64)
    b_max = bound_max.detach().cpu().numpy().astype(np.float64)
    vertices, triangles, leaks = marching_cubes_bricks(ub, brick_ijk, dims, threshold, origin=b_min, step=(b_max - b_min) / (R - 1.0),
                                                       marks=marks)
    info['leaks'] = leaks
    if leaks:
        raise _C.VqnError(f'extract_geometry_sparse: the surface runs into a skipped brick at {leaks} brick faces: the field changes '
                          f'faster than lipschitz = {lipschitz} allows; raise lipschitz')
    return vertices, triangles, info


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


_PLY_EXTRA_TYPES = {'int32': ('int', '<i4'), 'float32': ('float', '<f4'), 'uint8': ('uchar', 'u1')}


def write_ply(path, vertices, triangles, normals=None, colors=None, extra=None):
    """Binary little-endian PLY: `element vertex` with float x, y, z and `element face` with `property list uchar int vertex_indices`
    (the layout trimesh writes for a bare triangle mesh).  vertices [V,3], triangles [T,3]: arrays or tensors.  normals [V,3]: float
    nx, ny, nz after z; colors [V,3] (0..255): uchar red, green, blue after those (trimesh's order, what MeshLab and Blender read).
    extra {name: [V] array or tensor}: further scalar properties per vertex, after the colours, in the dict's order, typed by the
    array's dtype (int32 -> int, float32 -> float, uint8 -> uchar; anything else raises); read_ply(extra=names) reads them back."""
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
    extras = []
    for name, a in (extra or {}).items():
        a = _host_array(a)
        if str(a.dtype) not in _PLY_EXTRA_TYPES or a.reshape(-1).shape[0] != len(v) or not name.isidentifier():
            raise ValueError(f'write_ply: extra[{name!r}] must be {len(v)} values of {sorted(_PLY_EXTRA_TYPES)}, got {a.dtype} {a.shape}')
        ply_type, np_type = _PLY_EXTRA_TYPES[str(a.dtype)]
        fields.append(('x_' + name, np_type))
        props += f'property {ply_type} {name}\n'
        extras.append(('x_' + name, a.reshape(-1)))
    rows = np.empty(len(v), dtype=fields)                                   # packed: 12 (+ 12) (+ 3) bytes per vertex (+ the extras)
    rows['p'] = v
    for field, a in extras:
        rows[field] = a
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


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _ply_header(f, path):
    """-> (binary?, [(element, count, [(property, type) or (property, count type, item type)])])"""
    if f.readline().strip() != b'ply':
        raise _C.VqnError(f'read_ply: {path} is not a PLY file')
    fmt, elements = None, []
    for _ in range(1 << 16):                                               # (a header is tens of lines)
        raw = f.readline()
        if not raw:
            raise _C.VqnError(f'read_ply: {path}: the header does not end')
        w = raw.decode('ascii', 'replace').split()
        if not w or w[0] in ('comment', 'obj_info'):
            continue
        if w[0] == 'end_header':
            break
        if w[0] == 'format' and len(w) >= 2:
            fmt = w[1]
        elif w[0] == 'element' and len(w) == 3 and w[2].isdigit():
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property' and elements and len(w) == 5 and w[1] == 'list' and w[2] in _PLY_TYPES and w[3] in _PLY_TYPES:
            elements[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
        elif w[0] == 'property' and elements and len(w) == 3 and w[1] in _PLY_TYPES:
            elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
        else:
            raise _C.VqnError(f'read_ply: {path}: header line not understood: {raw!r}')
    else:
        raise _C.VqnError(f'read_ply: {path}: the header does not end')
    if fmt not in ('ascii', 'binary_little_endian'):
        raise _C.VqnError(f'read_ply: {path}: format {fmt} is not read (ascii and binary_little_endian are)')
    return fmt != 'ascii', elements


def _ply_rows(f, path, binary, name, count, props):
    """the rows of one element as {property: array [count] or, for a list of a fixed length, [count, length]}"""
    lists = [p for p in props if len(p) == 3]
    if lists and (len(props) != 1 or name != 'face'):
        raise _C.VqnError(f'read_ply: {path}: element {name}: a list property is read only as the single property of `face`')
    if binary:
        if lists:
            _, ct, it = props[0]
            dt = np.dtype([('n', '<' + ct), ('v', '<' + it, (3,))])
        else:
            dt = np.dtype([(p, '<' + t) for p, t in props])
        buf = f.read(dt.itemsize * count)
        rows = np.frombuffer(buf, dt, len(buf) // dt.itemsize)
        if lists and (rows['n'] != 3).any():                               # (read as rows of three: the first other face shows here)
            raise _C.VqnError(f'read_ply: {path}: only triangle faces are read')
        if len(rows) != count:
            raise _C.VqnError(f'read_ply: {path}: element {name} is cut short')
        if lists:
            return {props[0][0]: rows['v']}
        return {p: rows[p] for p, _ in props}
    width = 4 if lists else len(props)
    vals = []
    for _ in range(count):
        w = f.readline().split()
        if lists and w and w[0] != b'3':
            raise _C.VqnError(f'read_ply: {path}: only triangle faces are read')
        if len(w) != width:
            raise _C.VqnError(f'read_ply: {path}: element {name}: a row of {len(w)} values, expected {width}')
        vals.append(w)
    a = np.array(vals, dtype=np.float64).reshape(count, width)
    if lists:
        return {props[0][0]: a[:, 1:]}
    return {p: a[:, i] for i, (p, _) in enumerate(props)}


def read_ply(path, device='cuda', extra=None):
    """-> (vertices f32 [V,3], triangles int32 [T,3] or None, normals f32 [V,3] or None), tensors on `device`.  Reads ASCII and binary
    little-endian files whose `vertex` element has x y z and perhaps nx ny nz (colours and other scalar properties are skipped) and
    whose `face` element, if any, is one list `vertex_indices` / `vertex_index` of three: what write_ply writes, and point clouds
    without faces (DTU's scans).  Anything else -- big-endian data, faces that are not triangles -- raises VqnError.
    extra: names of scalar vertex properties (write_ply's `extra`, or red / green / blue) -> a fourth value, {name: tensor [V]} in the
    file's type (an ASCII file's values as float64); a name the file does not have raises VqnError."""
    with open(path, 'rb') as f:
        binary, elements = _ply_header(f, path)
        vert = tri = None
        for name, count, props in elements:
            rows = _ply_rows(f, path, binary, name, count, props)
            if name == 'vertex':
                vert = rows
            elif name == 'face':
                key = next((k for k in ('vertex_indices', 'vertex_index') if k in rows), None)
                if key is None:
                    raise _C.VqnError(f'read_ply: {path}: element face has no vertex_indices / vertex_index list')
                tri = rows[key]
    if vert is None or not all(k in vert for k in 'xyz'):
        raise _C.VqnError(f'read_ply: {path}: no vertex element with x, y and z')
    xyz = np.stack([vert[k] for k in 'xyz'], 1).astype(np.float32)
    nrm = np.stack([vert[k] for k in ('nx', 'ny', 'nz')], 1).astype(np.float32) if all(k in vert for k in ('nx', 'ny', 'nz')) else None
    if tri is not None:
        if len(tri) and (tri.min() < 0 or tri.max() >= len(xyz)):
            raise _C.VqnError(f'read_ply: {path}: a face names a vertex outside 0 .. {len(xyz) - 1}')
        tri = torch.as_tensor(np.array(tri, dtype=np.int32).reshape(-1, 3), device=device)        # (a copy: the file's bytes are read-only)
    out = (torch.as_tensor(np.ascontiguousarray(xyz), device=device), tri,
           None if nrm is None else torch.as_tensor(np.ascontiguousarray(nrm), device=device))
    if extra is None:
        return out
    missing = [k for k in extra if k not in vert]
    if missing:
        raise _C.VqnError(f'read_ply: {path}: the vertex element has no property {missing}')
    return out + ({k: torch.as_tensor(np.array(vert[k]), device=device) for k in extra},)


def sample_surface(vertices, triangles, n, generator=None, u=None):
    """n points of the surface, uniform by area (csrc/geometry_eval.hip: the face by binary search of the area prefix sum, the point
    (1 - sqrt(u1)) v0 + sqrt(u1) (1 - u2) v1 + sqrt(u1) u2 v2) -> (points f32 [n,3], unit face normals f32 [n,3], face int32 [n]).
    The randomness is an input: u f32 [n,3] in [0,1), or drawn from `generator` (a device generator; None: torch's global one)."""
    _C.require_device(vertices, 'sample_surface')
    vertices = vertices.detach().to(torch.float32).contiguous()
    triangles = triangles.to(torch.int32).contiguous()
    if u is None:
        u = torch.rand((int(n), 3), dtype=torch.float32, device=vertices.device, generator=generator)
    elif tuple(u.shape) != (int(n), 3):
        raise _C.VqnError(f'sample_surface: u must be [{int(n)}, 3], got {tuple(u.shape)}')
    cum = torch.cumsum(_C.geom_tri_areas(vertices, triangles), 0)
    return _C.geom_sample_surface(vertices, triangles, cum, u.contiguous())


# ---- material codes on the mesh: clean-up, face codes, split by code (csrc/mesh_materials.hip) ----------------
def _label_inputs(triangles, codes, what):
    _C.require_device(triangles, what)
    _C.require_device(codes, what)
    return triangles.detach().to(torch.int32).contiguous(), codes.detach().reshape(-1).to(torch.int32).contiguous()


def smooth_labels(triangles, codes, n_codes, iters=2, self_weight=1):
    """`iters` rounds of majority vote of the per-vertex codes [V] (int, 0 .. n_codes - 1) over the device mesh -> (codes, changed).
    One round: vertex v receives, for every triangle corner it is, one vote for the code of each of the triangle's two other corners,
    and self_weight votes for its own; it keeps its code if that holds the maximum, else takes the smallest code that does.  Every
    round reads the codes of the round before; a vertex no triangle uses keeps its code.  changed int32 [iters] (device): the
    vertices each round changed.  iters = 0 returns the same codes object and launches nothing.  No host read."""
    if int(iters) == 0:
        return codes, torch.empty((0,), dtype=torch.int32, device=codes.device)
    triangles, codes = _label_inputs(triangles, codes, 'smooth_labels')
    return _C.mesh_label_mode(triangles, codes, n_codes, iters, self_weight)


def _split_count(triangles, codes, n_codes):
    triangles, codes = _label_inputs(triangles, codes, 'split_by_label')
    return (triangles, codes) + _C.mesh_split_count(triangles, codes, n_codes)


def face_labels(triangles, codes, n_codes=_C.MESHMAT_MAX_CODES):
    """One code per face, int32 [T] (device): with a, b, c the codes of its vertices, a if a == b or a == c, else b if b == c, else
    min(a, b, c); -1 for a triangle with an index outside the vertices or a code outside [0, n_codes).  No host read."""
    return _split_count(triangles, codes, n_codes)[2]


def split_by_label(triangles, codes, n_codes):
    """The device mesh cut into one sub-mesh per code -> dict of
      face_code int32 [T] (face_labels); face_count [K] and face_offset [K + 1] (Python lists: the faces of each code and their
      exclusive prefix sum); face_src int32 [F]: the original indices of the faces with a code, ordered by (code, original index);
      vert_src int32 [S] with vert_offset [K + 1] (a list): for each code in turn the original ids of the vertices its faces use,
      ascending (a vertex on a border appears once in every group that uses it); vert_count [K];
      tris_local int32 [F, 3]: row j is face face_src[j], every vertex id replaced by its rank inside its group's slice of vert_src;
      n_faces = F, n_slots = S, dropped = T - F.
    Two kernels, two prefix sums between them, ONE host read (both offset lists, in one copy), as filter_components."""
    K = int(n_codes)
    triangles, codes, face_code, block_count, bitmap, word_count = _split_count(triangles, codes, K)
    T, V = triangles.shape[0], codes.shape[0]
    dev = triangles.device
    if V == 0 or T == 0:
        e = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
        return dict(face_code=face_code, face_count=[0] * K, face_offset=[0] * (K + 1), face_src=e(0), vert_src=e(0), vert_count=[0] * K,
                    vert_offset=[0] * (K + 1), tris_local=e(0, 3), n_faces=0, n_slots=0, dropped=T)
    B, W = block_count.shape[1], word_count.shape[1]
    binc = torch.cumsum(block_count.reshape(-1), 0, dtype=torch.int32)      # (totals <= T and <= 3 T: inside int32)
    winc = torch.cumsum(word_count.reshape(-1), 0, dtype=torch.int32)
    ends = torch.cat([binc[B - 1::B], winc[W - 1::W]]).tolist()             # the one host read
    face_offset, vert_offset = [0] + ends[:K], [0] + ends[K:]
    F, S = face_offset[K], vert_offset[K]
    block_offset = binc.sub_(block_count.reshape(-1))                       # exclusive prefix sums
    word_offset = winc.sub_(word_count.reshape(-1))
    face_src, tris_local, vert_src = _C.mesh_split_emit(triangles, V, K, face_code, block_offset, bitmap.reshape(-1), word_offset, F, S)
    return dict(face_code=face_code, face_count=[b - a for a, b in zip(face_offset, face_offset[1:])], face_offset=face_offset,
                face_src=face_src, vert_src=vert_src, vert_count=[b - a for a, b in zip(vert_offset, vert_offset[1:])],
                vert_offset=vert_offset, tris_local=tris_local, n_faces=F, n_slots=S, dropped=T - F)


def write_mtl(path, names, rows):
    """Wavefront MTL: one `newmtl <name>` per entry of names with the lines of rows[i], a dict of Kd [3], Ks [3], Pr, Ns and illum
    (decomp/material_mesh.py states how they follow from a material row).  Floats are written with nine significant digits: a
    float32 read back from the text is the float32 that was written."""
    with open(path, 'w') as f:
        f.write('# materials of the VQ codes\n')
        for name, row in zip(names, rows):
            f.write(f'\nnewmtl {name}\n')
            f.write('Kd %.9g %.9g %.9g\n' % tuple(float(x) for x in row['Kd']))
            f.write('Ks %.9g %.9g %.9g\n' % tuple(float(x) for x in row['Ks']))
            f.write('Pr %.9g\nNs %.9g\nillum %d\n' % (float(row['Pr']), float(row['Ns']), int(row['illum'])))


def write_obj(path, vertices, triangles_sorted, face_offset, names, normals=None, mtllib=None):
    """Wavefront OBJ of a mesh whose faces are sorted by material: `mtllib` (default: the path's own name with .mtl), every vertex as
    `v x y z` (and `vn` with normals [V,3]), then for every group k with face_offset[k] < face_offset[k + 1] one `usemtl names[k]`
    followed by its faces `f a b c` (`f a//a b//b c//c` with normals), 1-based.  triangles_sorted [F,3]: the faces in group order
    (tris[face_src] of split_by_label).  Floats with nine significant digits."""
    import os
    v = _host_array(vertices).reshape(-1, 3)
    t = _host_array(triangles_sorted).reshape(-1, 3).astype(np.int64) + 1
    n = None if normals is None else _host_array(normals).reshape(-1, 3)
    if len(face_offset) != len(names) + 1 or face_offset[0] != 0 or face_offset[-1] != len(t):
        raise ValueError(f'write_obj: face_offset must run from 0 to {len(t)} over {len(names)} groups, got {list(face_offset)[:4]} ...')
    if n is not None and len(n) != len(v):
        raise ValueError(f'write_obj: {len(n)} normals for {len(v)} vertices')
    if mtllib is None:
        mtllib = os.path.splitext(os.path.basename(path))[0] + '.mtl'
    with open(path, 'w') as f:
        f.write(f'mtllib {mtllib}\n')
        f.write(''.join('v %.9g %.9g %.9g\n' % tuple(r) for r in v.tolist()))
        if n is not None:
            f.write(''.join('vn %.9g %.9g %.9g\n' % tuple(r) for r in n.tolist()))
        fmt = 'f %d//%d %d//%d %d//%d\n' if n is not None else 'f %d %d %d\n'
        for k, name in enumerate(names):
            a, b = int(face_offset[k]), int(face_offset[k + 1])
            if a == b:
                continue
            f.write(f'usemtl {name}\n')
            rows = t[a:b].tolist()
            f.write(''.join(fmt % (tuple(x for i in r for x in (i, i)) if n is not None else tuple(r)) for r in rows))
