/* vqn_geometry_eval.h -- surface scores of geometry that is on the device, from libvqnerf_hip.so: triangle areas and surface
 * sampling, a uniform grid over a reference cloud, the exact nearest neighbour of every query point, and the directed sums that
 * accuracy / completeness / Chamfer, precision / recall / F-score and normal consistency are made of (csrc/geometry_eval.hip; the
 * statement is tests/geometry_eval_model.py).  Same conventions as vqnerf_hip.h (device pointers owned by the
 * caller, host descriptors, `stream` a hipStream_t, negative return = error with vqn_last_error()).  The library allocates nothing.
 * Return codes of every call: -2 for a refused shape (no points, a count >= 2^31, more than 8 thresholds, a grid over the caps);
 * nothing is launched.  -1 for null pointers, a bad value or a scratch that is too small.  A call with zero queries / samples is a
 * no-op. */
#ifndef VQN_GEOMETRY_EVAL_H_
#define VQN_GEOMETRY_EVAL_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_GEOM_MAX_CELLS 16777216   /* cells of a grid at most: 2^24 */
#define VQN_GEOM_MAX_AXIS 1024        /* cells per axis at most */
#define VQN_GEOM_MAX_THRESHOLDS 8     /* distance thresholds of one reduction at most */
#define VQN_GEOM_OUT_WORDS 16         /* 8-byte words of the reduction's `out` */
#define VQN_GEOM_THREADS 256          /* threads of every workgroup: one point, query or triangle per thread */
#define VQN_GEOM_REDUCE_GRID_CAP 1024 /* workgroups of the reduction's first launch at most */

/* A uniform grid: cell (i, j, k) covers origin + (i, j, k) * h .. + h; its id is (k * dims[1] + j) * dims[0] + i (x fastest).
 * cells = dims[0] * dims[1] * dims[2]. */
struct VqnGeomGrid {
  float origin[3];
  float h;
  int32_t dims[3];
  int32_t cells;
};

/* ---- surface sampling -----------------------------------------------------------------------------------------------------------------
 * vertices f32 [n_verts][3], triangles int32 [n_tris][3].
 * _tri_areas: areas[t] (float64) = 0.5 |(v1 - v0) x (v2 - v0)|, in double from the float32 coordinates; 0 for a triangle with an
 * index outside [0, n_verts).
 * _sample_surface: cum float64 [n_tris] = the inclusive prefix sum of the areas (the caller's), u f32 [n][3] in [0, 1).  Sample i:
 * x = (double)u0 * cum[n_tris - 1]; face = the first t with cum[t] > x (binary search: a zero-area triangle is never chosen);
 * s = sqrt((double)u1), a = 1 - s, b = s (1 - u2), c = s u2; point = (a v0 + b v1) + c v2 in double, rounded once to f32; normal =
 * the unit face normal (v1 - v0) x (v2 - v0) / |.| in double, rounded once, (0, 0, 0) for a degenerate face.  No FMA contraction.
 * points, normals f32 [n][3], face int32 [n]. */
int vqn_geom_tri_areas(const float* vertices, int64_t n_verts, const int32_t* triangles, int64_t n_tris, double* areas, void* stream);
int vqn_geom_sample_surface(const float* vertices, int64_t n_verts, const int32_t* triangles, int64_t n_tris, const double* cum,
                            const float* u, int64_t n, float* points, float* normals, int32_t* face, void* stream);

/* ---- the grid over the reference cloud --------------------------------------------------------------------------------------------------
 * _grid_plan (host only, no device): lo, hi = the bounding box of the n reference points (three host floats each).  cell > 0 is the
 * cell size; cell <= 0 asks for the default h = sqrt(8 S / n), S = the box's surface area (for a box without area: 8 L / n with L its
 * longest side, 1 for a single point), raised as far as VQN_GEOM_MAX_AXIS and VQN_GEOM_MAX_CELLS require.  origin = lo,
 * dims = floor((hi - lo) / h) + 1 per axis.  An override that needs more than the caps, or is not finite, is refused with -2.
 * No result of _nearest depends on h.
 * _cell_ids: ids[i] = the id of the cell of point i: per axis floor((p - origin) / h) in f32, clamped into [0, dims - 1].
 * _pack_sorted: order int64 [n] = the permutation that sorts the ids (stable); packed [n] 16-byte records (x, y, z, the bits of the
 * original index as int32), record j = point order[j].  16-byte aligned. */
int vqn_geom_grid_plan(const float* lo, const float* hi, int64_t n, float cell, struct VqnGeomGrid* grid);
int vqn_geom_cell_ids(const float* points, int64_t n, const struct VqnGeomGrid* grid, int32_t* ids, void* stream);
int vqn_geom_pack_sorted(const float* points, int64_t n, const int64_t* order, void* packed, void* stream);

/* ---- nearest neighbour ------------------------------------------------------------------------------------------------------------------
 * query f32 [n_q][3]; packed the n_ref sorted records; cell_start int32 [cells + 1]: the records of cell c are
 * cell_start[c] .. cell_start[c + 1] - 1.  d2(q, p) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) in f32 with dx = fl(px - qx) ...: every
 * product and sum rounded on its own, no FMA.  Per query the record with the least (d2, original index), compared lexicographically:
 * ties go to the lowest original index whatever the traversal.  The search walks rings of cells around the query's (clamped) cell
 * and stops only when the best d2 is at most a lower bound of d2 to any point outside the rings done; the number
 * of rings is bounded by max(dims).  max_d2 (f32, +inf for none): the search also stops once that bound exceeds max_d2, and a query
 * whose best d2 > max_d2 gets idx -1 and d2 +inf.  q_order (may be NULL) int32 [n_q]: thread i serves query q_order[i] (queries
 * sorted by cell walk the same cells in a wave); results are written at the query's own row either way.  d2 f32 [n_q], idx int32
 * [n_q] = the original index.  One launch. */
int vqn_geom_nearest(const float* query, int64_t n_q, const int32_t* q_order, const void* packed, const int32_t* cell_start, int64_t n_ref,
                     const struct VqnGeomGrid* grid, float max_d2, float* d2, int32_t* idx, void* stream);

/* ---- directed reduction -----------------------------------------------------------------------------------------------------------------
 * d2, idx [n] as _nearest wrote them, n >= 1 (a sum over nothing is refused like any other empty shape); q_normals f32 [n][3] and ref_normals f32 [n_ref][3] (either may be NULL: no normal terms);
 * thresholds: n_thresholds <= 8 HOST doubles.  Over the valid queries (0 <= idx < n_ref), d = sqrt((double)d2):
 * out, 16 8-byte words: 0 int64 n; 1 int64 n_valid; 2..9 int64 count(d < threshold_k) (0 past n_thresholds); 10 float64 sum d;
 * 11 float64 sum (double)d2; 12 float64 max d (0 for none); 13 float64 sum |n_q . n_ref[idx]|, the dot product in double, over the
 * pairs whose two normals are both non-zero; 14 int64 their number; 15 zero.
 * scratch: vqn_geom_reduce_scratch_bytes(n) bytes (16 words per workgroup of the first launch; 0 for an n the call refuses).  Two
 * launches, per-workgroup partial sums added in a fixed order, no atomics: equal inputs give equal bits. */
int64_t vqn_geom_reduce_scratch_bytes(int64_t n);
int vqn_geom_reduce(const float* d2, const int32_t* idx, int64_t n, const float* q_normals, const float* ref_normals, int64_t n_ref,
                    const double* thresholds, int n_thresholds, void* scratch, int64_t scratch_bytes, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_GEOMETRY_EVAL_H_ */
