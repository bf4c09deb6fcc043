"""Mesh export of the NeuS surface on the device: the field on a regular grid through the fused SDF kernel, marching cubes through
csrc/marching_cubes.hip, a binary PLY writer.  Stands in for the reference's `mcubes.marching_cubes` + `trimesh` export
(geo/NeuS-ours2/models/renderer.py:10-36, nerf_runner.py:381-395); conventions: csrc/mc_table.h, DESIGN.md.

An extraction reads the host once (the vertex and triangle totals, to size the outputs); the field never leaves the device.
"""
import numpy as np
import torch

from vqnerf_release_amd import _C

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


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: `element vertex` with float x, y, z and `element face` with `property list uchar int vertex_indices`
    (the layout trimesh writes for a bare triangle mesh).  vertices [V,3], triangles [T,3]: arrays or tensors."""
    v = vertices.detach().cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)
    t = triangles.detach().cpu().numpy() if torch.is_tensor(triangles) else np.asarray(triangles)
    v = np.ascontiguousarray(v.reshape(-1, 3), dtype='<f4')
    t = t.reshape(-1, 3)
    faces = np.empty(len(t), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    faces['n'] = 3
    faces['v'] = t
    header = ('ply\nformat binary_little_endian 1.0\n'
              f'element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n'
              f'element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n')
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(v.tobytes())
        f.write(faces.tobytes())
