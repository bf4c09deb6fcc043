"""Ray queries against a triangle mesh on the device (csrc/mesh_rays.hip through _C.rays_*; include/vqn_mesh_rays.h states what a hit
is): the nearest hit of a ray, whether a segment is occluded, and the light visibility of surface points -- the
mesh route of `GeoExtractor.compute_vis_mesh` (geo/gen_geo.py), which asks of the exported mesh what `compute_vis` asks of the
network.  No counterpart in the reference, which computes visibility volumetrically only.
"""
import math

import numpy as np
import torch

from vqnerf_release_amd import _C

# The default bias of light_visibility, in grid cells.  The surface points of a view come from the volumetric render and lie a little
# off the mesh; the ray to a light must start clear of the mesh's own faces under the point.  Chosen on an UNTRAINED geometric-init
# sphere, the only network there was (scripts/probe_mesh_rays.py): there the render's surface points lie within a fraction of an
# extraction cell of the mesh, the default grid cell is about one extraction cell, and one cell clears every point while staying
# far below the size of anything that casts a shadow.  A trained scene may want another value: pass `bias`.
DEFAULT_BIAS_CELLS = 1.0


def _f32(t, dev, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _C.VqnError(f'{what}: expected a device tensor; the mesh ray caster runs on the HIP kernels only (there is no CPU fallback)')
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


class MeshRays:
    """MeshRays(vertices f32 [V, 3], triangles int32 [T, 3], cell=None): the grid over the mesh, built once -- the mesh's bounding box (read
    to the host: the planner is host code), plan, count, prefix sum, ONE read of the host (the total of the lists and the counters of
    dropped triangles), bin.  `stats`: {cause: dropped triangles,
    'pairs': (triangle, cell) pairs}; `grid`: the _C.GeomGrid; `cell`: its cell size."""

    def __init__(self, vertices, triangles, cell=None):
        if not torch.is_tensor(vertices) or not vertices.is_cuda or not torch.is_tensor(triangles) or not triangles.is_cuda:
            raise _C.VqnError('MeshRays: vertices and triangles must be device tensors (there is no CPU fallback)')
        self.vertices = vertices.detach().float().reshape(-1, 3).contiguous()
        self.triangles = triangles.detach().to(torch.int32).reshape(-1, 3).contiguous()
        dev = self.device = self.vertices.device
        T = self.triangles.shape[0]
        finite = self.vertices[torch.isfinite(self.vertices).all(1)]
        if finite.shape[0]:
            box = torch.stack([finite.min(0).values, finite.max(0).values]).cpu().numpy()      # (the mesh's own box: before the build)
        else:
            box = np.zeros((2, 3), np.float32)
        self.grid = _C.rays_grid_plan(box[0], box[1], T, cell)
        self.cell = float(self.grid.h)
        cell_count, stats = _C.rays_count(self.vertices, self.triangles, self.grid)
        ends = torch.cumsum(cell_count, 0, dtype=torch.int64)
        head = torch.cat([ends[-1:], stats.long()]).cpu().tolist()
        self.n_pairs = int(head[0])
        self.stats = dict(zip(_C.RAYS_STAT_NAMES, head[1:]), pairs=self.n_pairs)
        self.cell_offset = (ends - cell_count).to(torch.int32)
        self.bin, self.packed = _C.rays_bin(self.vertices, self.triangles, self.grid, self.cell_offset, self.n_pairs)

    def _scene(self):
        return self.packed, self.grid, self.cell_offset, self.n_pairs, self.bin

    def _rays(self, o, d, tmin, tmax, what):
        o, d = _f32(o, self.device, what).reshape(-1, 3), _f32(d, self.device, what).reshape(-1, 3)
        n = o.shape[0]
        if d.shape[0] != n:
            raise _C.VqnError(f'{what}: o and d are [n, 3] both, got {tuple(o.shape)} and {tuple(d.shape)}')
        lim = [torch.as_tensor(x, dtype=torch.float32, device=self.device).expand(n).contiguous() for x in (tmin, tmax)]
        return o, d, lim[0], lim[1], n

    @torch.no_grad()
    def cast(self, o, d, tmin=0.0, tmax=math.inf):
        """o, d [n, 3]; tmin, tmax scalars or [n] -> dict(face int32 [n] (-1: miss), t f32 [n] (+inf), uv f32 [n, 2] (0))"""
        o, d, tmin, tmax, n = self._rays(o, d, tmin, tmax, 'MeshRays.cast')
        if n == 0:
            return dict(face=torch.empty((0,), dtype=torch.int32, device=self.device), t=torch.empty((0,), device=self.device),
                        uv=torch.empty((0, 2), device=self.device))
        face, t, uv = _C.rays_cast(*self._scene(), o, d, tmin, tmax)
        return dict(face=face, t=t, uv=uv)

    @torch.no_grad()
    def occluded(self, o, d, tmin=0.0, tmax=math.inf):
        """-> bool [n]: some triangle is hit with tmin < t < tmax"""
        o, d, tmin, tmax, n = self._rays(o, d, tmin, tmax, 'MeshRays.occluded')
        if n == 0:
            return torch.empty((0,), dtype=torch.bool, device=self.device)
        return _C.rays_occluded(*self._scene(), o, d, tmin, tmax).bool()

    def default_bias(self):
        return DEFAULT_BIAS_CELLS * self.cell

    @torch.no_grad()
    def light_visibility(self, points, normals, lights, bias=None, lanes='points'):
        """points, normals [n, 3], lights [L, 3] -> f32 [n, L]: 1 where the light is in front of the point (by its normal) and the
        segment from p + bias n to the light meets no triangle, else 0.  bias None: DEFAULT_BIAS_CELLS grid cells.  lanes: 'points' or
        'lights', how the kernel lays the rays over a wave (the result is the same)."""
        what = 'MeshRays.light_visibility'
        p, nrm, l = (_f32(x, self.device, what).reshape(-1, 3) for x in (points, normals, lights))
        if p.shape != nrm.shape:
            raise _C.VqnError(f'{what}: points and normals are [n, 3] both, got {tuple(p.shape)} and {tuple(nrm.shape)}')
        if lanes not in ('points', 'lights'):
            raise _C.VqnError(f"{what}: lanes is 'points' or 'lights', got {lanes!r}")
        if p.shape[0] == 0 or l.shape[0] == 0:
            return torch.zeros((p.shape[0], l.shape[0]), device=self.device)
        return _C.rays_light_visibility(*self._scene(), p, nrm, l, self.default_bias() if bias is None else float(bias),
                                        _C.RAYS_LANES_POINTS if lanes == 'points' else _C.RAYS_LANES_LIGHTS)


def as_mesh_rays(mesh, device):
    """a MeshRays, a (vertices, triangles) pair or the path of a PLY (geo/mesh.read_ply) -> MeshRays"""
    if isinstance(mesh, MeshRays):
        return mesh
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, '__fspath__'):
        from vqnerf_release_amd.geo.mesh import read_ply
        vertices, triangles, _ = read_ply(mesh, device=device)
        if triangles is None:
            raise _C.VqnError(f'{mesh}: a point cloud has no faces to cast rays at')
        return MeshRays(vertices, triangles)
    vertices, triangles = mesh
    return MeshRays(torch.as_tensor(vertices).to(device), torch.as_tensor(triangles).to(device))
