/* vqn_mesh_raster.h -- an indexed triangle mesh drawn from a pin-hole camera, from libvqnerf_hip.so (csrc/mesh_raster.hip; sizes, tile
 * grid and refusals by csrc/mesh_raster_plan.h; the plain statement is tests/mesh_raster_model.py): per pixel the visible face, its
 * depth and its perspective-correct barycentrics, and the gather of per-vertex attributes over them.  Same conventions as vqn_mesh.h
 * (device pointers owned by the caller, `stream` a hipStream_t, negative return = error with vqn_last_error(), a refused call launches
 * nothing, no memory outside the stated extents is touched).  Coverage is integer arithmetic, the winner of a pixel is a minimum, and
 * no result is formed by an atomic: the outputs are the same from run to run.
 *
 * Inputs: verts [n_verts][3] f32; tris [n_tris][3] int32; the camera P [3][4] f32, row-major, read from a HOST pointer and handed to
 * the kernels by value: P (x, y, z, 1)^T = (u w, v w, w) with w > 0 in front of the camera and P's third row scaled so that w is the
 * distance along the optical axis; 1 <= H, W <= VQN_RASTER_MAX_SIDE; near > 0; cull in {0, +1, -1}.  Pixel (i, j) is sampled at the
 * screen point (u, v) = (j, i) exactly.
 *
 * Vertex, f32, every operation rounded on its own: h_r = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3]; w = h_2, sx = h_0 / w,
 * sy = h_1 / w; X = rint(256 sx), Y = rint(256 sy) (half to even).  A vertex is usable iff w is finite, w >= near and |256 sx|,
 * |256 sy| < VQN_RASTER_COORD_LIMIT.
 * Triangle, int64: it is dropped -- and counted in stats [VQN_RASTER_STATS] int32, in this order of causes -- for an index outside
 * [0, n_verts) (stats[0]), an unusable vertex (stats[1]; there is NO clipping: a triangle that reaches behind `near` is not drawn),
 * area2 = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) == 0 (stats[2]), sign(area2) == cull (stats[3]).  With s = sign(area2) and the
 * sample p = (256 j, 256 i): E0 = s [(X2 - X1)(p.y - Y1) - (Y2 - Y1)(p.x - X1)], E1 and E2 the same for the edges v2 -> v0 and
 * v0 -> v1, so E0 + E1 + E2 = |area2|.  The sample is covered iff for every k E_k > 0, or E_k == 0 and edge k owns its boundary: with
 * d = s (end - start), d.y > 0 or (d.y == 0 and d.x < 0).
 * Depth and barycentrics, f64: q_k = 1.0 / (double)w_k; S = ((double)E0 q0 + (double)E1 q1) + (double)E2 q2; depth = (float)((double)
 * |area2| / S); bary_k = (float)(((double)E_k q_k) / S).
 * Visibility: the pixel keeps the minimum of (uint64)float_bits(depth) << 32 | face -- the nearest face, ties to the lowest index.
 * Outputs: face [H][W] int32 (-1: background), depth [H][W] f32 (+inf), bary [H][W][3] f32 (0).
 *
 * Every call returns
 *   -1 for a null pointer (where the array it names is not empty), a negative size, near <= 0 or not finite, cull outside {0, +1, -1},
 *      a total that contradicts the sizes;
 *   -2 for H or W outside 1 .. VQN_RASTER_MAX_SIDE, n_verts >= 2^31, 3 n_tris >= 2^31, n_pairs >= 2^31, n_channels outside 1 .. 16. */
#ifndef VQN_MESH_RASTER_H_
#define VQN_MESH_RASTER_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_RASTER_TILE 16                 /* pixels per side of a tile: one workgroup of 256 threads resolves one tile */
#define VQN_RASTER_SUBPIXEL_BITS 8         /* screen coordinates are snapped to 1 / 256 pixel */
#define VQN_RASTER_MAX_SIDE 8192           /* H and W at most */
#define VQN_RASTER_COORD_LIMIT (1 << 23)   /* |snapped coordinate| below this, in sub-pixel units */
#define VQN_RASTER_CHUNK 256               /* triangles of a tile's list staged in LDS at a time */
#define VQN_RASTER_STATS 4                 /* counters of dropped triangles: bad index, unusable vertex, zero area, culled */
#define VQN_RASTER_MAX_CHANNELS 16         /* attribute channels of vqn_raster_interpolate at most */

/* ---- count / resolve; the caller does the prefix sum between the two calls, as with vqn_mc_classify / _emit ------------------------
 * With TX = ceil(W / 16), TY = ceil(H / 16) and tile (ty, tx) at entry ty TX + tx:
 *
 * vqn_raster_count projects the vertices into pverts [n_verts][3] int32 (X, Y, the bits of w; w = 0 marks an unusable vertex), zeroes
 * and fills stats, and zeroes and fills tile_count [TY TX] int32: the kept triangles whose pixel bounding box -- the pixels (i, j)
 * with min X <= 256 j <= max X and min Y <= 256 i <= max Y, inside the image -- meets the tile.  n_tris = 0 or n_verts = 0: nothing
 * is read, the counts are zero.
 *
 * vqn_raster_resolve takes tile_offset [TY TX], the EXCLUSIVE prefix sum of tile_count, and its total n_pairs; zeroes cursor [TY TX]
 * (scratch); fills bin [n_pairs] int32 with each tile's triangles at tile_offset[tile] .. (in no particular order: the winner of a
 * pixel is a minimum), and writes face, depth and bary.  Entries of bin outside [0, n_pairs) are never written, and an entry that
 * does not name a kept triangle is skipped, so offsets that do not belong to these counts lose triangles and touch nothing else. */
int vqn_raster_count(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const float* P, int H, int W, float near,
                     int cull, int32_t* pverts, int32_t* tile_count, int32_t* stats, void* stream);
int vqn_raster_resolve(const int32_t* tris, int64_t n_tris, const int32_t* pverts, int64_t n_verts, int H, int W, int cull,
                       const int32_t* tile_offset, int64_t n_pairs, int32_t* cursor, int32_t* bin, int32_t* face, float* depth,
                       float* bary, void* stream);

/* ---- per-vertex attributes over the raster ------------------------------------------------------------------------------------------
 * attr [n_verts][n_channels] f32, 1 <= n_channels <= VQN_RASTER_MAX_CHANNELS -> out [H][W][n_channels]: with (v0, v1, v2) the
 * vertices of the pixel's face and b its bary, out = (b0 a0 + b1 a1) + b2 a2 in f32, every operation rounded on its own; nearest != 0:
 * the attribute of the corner with the largest b, ties to the lowest corner (integer labels held as f32).  A pixel whose face is
 * outside [0, n_tris), or whose face has an index outside [0, n_verts), gets the row background [n_channels] (device). */
int vqn_raster_interpolate(const int32_t* face, const float* bary, int H, int W, const int32_t* tris, int64_t n_tris, const float* attr,
                           int64_t n_verts, int n_channels, const float* background, int nearest, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_MESH_RASTER_H_ */
