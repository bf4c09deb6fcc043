/* vqn_mesh_rays.h -- ray queries against an indexed triangle mesh, from libvqnerf_hip.so (csrc/mesh_rays.hip; sizes, the grid rule,
 * limits and refusals by csrc/mesh_rays_plan.h; the plain statement is tests/mesh_rays_model.py): the nearest
 * hit of a ray, whether a segment is occluded, and the fused light visibility of surface points (geo/mesh_rays.py).  Same conventions
 * as vqn_mesh_raster.h and vqn_geometry_eval.h (device pointers owned by the caller, `stream` a hipStream_t, negative return = error
 * with vqn_last_error(), a refused call launches nothing, the library allocates nothing, no memory outside the stated extents is
 * touched).  Results are minima and booleans, no atomic forms one: the outputs are the same from run to run.
 *
 * THE STATEMENT OF A HIT.  verts [n_verts][3] f32, tris [n_tris][3] int32; a ray is (o, d, tmin, tmax).  All f32, every product and
 * sum rounded on its own (no FMA); a x b for vectors has the components fl(fl(a.y b.z) - fl(a.z b.y)), fl(fl(a.z b.x) - fl(a.x b.z)),
 * fl(fl(a.x b.y) - fl(a.y b.x)):
 *   e1 = v1 - v0, e2 = v2 - v0;  p = d x e2;  det = (e1.x p.x + e1.y p.y) + e1.z p.z;  inv = 1 / det;  s = o - v0;
 *   u = ((s.x p.x + s.y p.y) + s.z p.z) inv;  q = s x e1;  v = ((d.x q.x + d.y q.y) + d.z q.z) inv;
 *   t = ((e2.x q.x + e2.y q.y) + e2.z q.z) inv.
 * The ray hits the triangle iff det != 0, u >= 0, v >= 0, fl(u + v) <= 1 and tmin < t < tmax.  Both sides of a triangle count (the
 * exported mesh promises no winding); a NaN anywhere is a miss.  This is NOT watertight: a ray can pass between two triangles at an
 * edge they share, where u, v of the two are rounded apart (DESIGN section 18 counts it on a closed icosphere).
 * A triangle is kept unless -- counted in stats [VQN_RAYS_STATS] int32 in this order of causes -- it has an index outside
 * [0, n_verts) (stats[0]), a vertex that is not finite (stats[1]), or e1 x e2 == (0, 0, 0) exactly (stats[2]).  Only kept triangles
 * are tested.
 * A ray is cast iff every component of o and d and tmin are finite, tmax is not a NaN, 0 <= tmin < tmax and the largest |d| component
 * is at least VQN_RAYS_MIN_DIR = 2^-60; every other ray is a miss.
 * Nearest hit: the minimum over all hit triangles of (uint64)float_bits(t) << 32 | face -- the nearest face, ties to the lowest index,
 * whatever the traversal.  Any hit: a boolean.
 *
 * THE GRID.  A uniform grid (struct VqnGeomGrid of vqn_geometry_eval.h) holds per cell the list of the triangles that may meet it; a
 * ray walks its cells by a 3-D DDA of at most dims[0] + dims[1] + dims[2] + 3 steps.  vqn_rays_grid_plan places the grid half a cell
 * beyond the mesh's bounding box on every side; queries find the triangles that lie inside the grid's box shrunk by h / 2 -- all of
 * them, for a planned grid -- for ray origins and a mesh within 8 box diagonals of the world origin (DESIGN section 18 argues it; the
 * walk is bounded and in range for any input).  No result depends on the cell size. */
#ifndef VQN_MESH_RAYS_H_
#define VQN_MESH_RAYS_H_
#include <stdint.h>

#include "vqn_geometry_eval.h"
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_RAYS_MAX_AXIS 1024       /* cells per axis at most */
#define VQN_RAYS_MAX_CELLS 16777216  /* cells at most: 2^24, a cell table of 64 MB */
#define VQN_RAYS_STATS 3             /* counters of dropped triangles: bad index, non-finite vertex, zero area */
#define VQN_RAYS_MARGIN_INV 16       /* a triangle's box is widened by 1 / 16 cell on every side before it is binned */
#define VQN_RAYS_PACKED_FLOATS 12    /* floats of a packed triangle: v0, e1, e2, three of padding (48 bytes, 16-byte aligned) */
#define VQN_RAYS_MAX_LIGHTS 65536    /* lights of vqn_rays_light_visibility at most */
#define VQN_RAYS_TILE 64             /* points x lights of the tile that the visibility kernel stages and writes as whole rows */
#define VQN_RAYS_MIN_DIR_LOG2 -60    /* a ray is cast only if max |d component| >= 2^-60 */
#define VQN_RAYS_LANES_POINTS 0      /* vqn_rays_light_visibility: the 64 lanes of a wave hold 64 neighbouring points of one light */
#define VQN_RAYS_LANES_LIGHTS 1      /* ... or 64 lights of one point */

/* ---- the grid (host only, no device) ---------------------------------------------------------------------------------------------------
 * lo, hi = the bounding box of the mesh's finite vertices (three host floats each), n_tris >= 0 its triangle count.  cell > 0 is the
 * cell size h; cell <= 0 asks for the default h = sqrt(2 S / max(n_tris, 1)), S = the box's surface area (a box without area:
 * 2 L / max(n_tris, 1) with L its longest side, 1 for a point) -- marching-cubes triangles then span about one cell -- raised as far
 * as VQN_RAYS_MAX_AXIS and VQN_RAYS_MAX_CELLS require.  origin = fl(lo - fl(h / 2)), dims = floor((hi - lo) / h) + 2 per axis, so the
 * grid's box reaches at least h / 2 beyond the mesh on every side.  -1: a null pointer, a box that is not finite or has lo > hi, a
 * negative n_tris; -2: n_tris >= 2^31 / 3, an override that is not finite or needs more than the caps. */
int vqn_rays_grid_plan(const float* lo, const float* hi, int64_t n_tris, float cell, struct VqnGeomGrid* grid);

/* ---- count / bin; the caller takes the exclusive prefix sum between the two, as with vqn_raster_count / _resolve -----------------------
 * `grid` is a HOST pointer, handed to the kernels by value.  With g_a(x) = fl(fl(x - origin[a]) / h) and m = 1 / 16, a kept triangle
 * is listed in the cells [c0_a, c1_a] per axis a: c0_a = floor(fl(g_a(min_a) - m)), c1_a = floor(fl(g_a(max_a) + m)), min_a / max_a
 * over its three vertices, each clamped into [0, dims[a] - 1].
 *
 * vqn_rays_count zeroes and fills stats, and zeroes and fills cell_count [cells] int32: the kept triangles listed in each cell.
 * vqn_rays_bin takes cell_offset [cells] int32, the EXCLUSIVE prefix sum of cell_count, and its total n_pairs; zeroes cursor [cells]
 * (scratch); fills bin [n_pairs] int32 with each cell's triangles at cell_offset[cell] .. (in no particular order: results are minima
 * and booleans), and packed [n_tris][12] f32 (16-byte aligned): (v0, e1, e2, 0, 0, 0) of a kept triangle, e1 and e2 as the statement
 * rounds them, NaN throughout for a dropped one.  Entries of bin outside [0, n_pairs) are never written; offsets that do not belong
 * to these counts lose triangles and touch nothing else.
 * -1: a null pointer (where the array it names is not empty), a negative size, a grid that is not one (h, origin, dims, cells);
 * -2: n_verts >= 2^31, 3 n_tris >= 2^31, n_pairs >= 2^31, a grid over the caps. */
int vqn_rays_count(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const struct VqnGeomGrid* grid,
                   int32_t* cell_count, int32_t* stats, void* stream);
int vqn_rays_bin(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const struct VqnGeomGrid* grid,
                 const int32_t* cell_offset, int64_t n_pairs, int32_t* cursor, int32_t* bin, float* packed, void* stream);

/* ---- queries ----------------------------------------------------------------------------------------------------------------------------
 * packed, cell_offset, n_pairs and bin as vqn_rays_bin took and left them.  o, d f32 [n][3]; tmin, tmax f32 [n].  n = 0: a no-op.
 * vqn_rays_cast: face int32 [n] (-1 for a miss), t f32 [n] (+inf), uv f32 [n][2] (0): the nearest hit and its u, v.
 * vqn_rays_occluded: occ uint8 [n]: 1 iff any triangle is hit.
 * An entry of bin outside [0, n_tris) and a cell whose offsets are not 0 <= first <= end <= n_pairs are skipped. */
int vqn_rays_cast(const float* packed, int64_t n_tris, const struct VqnGeomGrid* grid, const int32_t* cell_offset, int64_t n_pairs,
                  const int32_t* bin, const float* o, const float* d, const float* tmin, const float* tmax, int64_t n, int32_t* face,
                  float* t, float* uv, void* stream);
int vqn_rays_occluded(const float* packed, int64_t n_tris, const struct VqnGeomGrid* grid, const int32_t* cell_offset, int64_t n_pairs,
                      const int32_t* bin, const float* o, const float* d, const float* tmin, const float* tmax, int64_t n, uint8_t* occ,
                      void* stream);

/* ---- light visibility: fused, no ray is ever stored ---------------------------------------------------------------------------------------
 * points, normals f32 [n][3]; lights f32 [n_lights][3], 1 <= n_lights <= VQN_RAYS_MAX_LIGHTS; bias finite.  Per (point i, light l),
 * f32, every operation rounded on its own, in this order:
 *   o = p + fl(bias n) per component;  dl = l - o;  dist = sqrt((dl.x^2 + dl.y^2) + dl.z^2);  d = dl / dist per component;
 *   front = ((d.x n.x + d.y n.y) + d.z n.z) > 0.
 * out [n][n_lights] f32: 1.0f iff front holds and the ray (o, d, tmin = 0, tmax = dist) hits no triangle, else 0.0f.  lanes:
 * VQN_RAYS_LANES_POINTS (a 64 x 64 tile of `out` is staged in LDS and written as whole rows) or VQN_RAYS_LANES_LIGHTS; the result
 * is the same.  -1 also for a bias that is not finite or another value of lanes; -2 also for n_lights outside its range and
 * n * n_lights >= 2^40. */
int vqn_rays_light_visibility(const float* packed, int64_t n_tris, const struct VqnGeomGrid* grid, const int32_t* cell_offset,
                              int64_t n_pairs, const int32_t* bin, const float* points, const float* normals, int64_t n,
                              const float* lights, int n_lights, float bias, int lanes, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_MESH_RAYS_H_ */
