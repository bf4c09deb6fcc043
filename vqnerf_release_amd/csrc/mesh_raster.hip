// A tiled triangle rasteriser for gfx950 (include/vqn_mesh_raster.h; the host side is csrc/mesh_raster_plan.h, the plain statement
// tests/mesh_raster_model.py; geo/mesh_render.py): per pixel the visible face of an indexed mesh, its depth and its barycentrics, and
// the gather of per-vertex attributes over them.  DESIGN.md section 17.
//
// Coverage is integer work on vertices snapped to 1 / 256 pixel, so a sample on an edge that two triangles share belongs to exactly
// one of them; depth and barycentrics are doubles formed from those exact integers; the winner of a pixel is the minimum of a 64-bit
// key held in the registers of the one thread that owns the pixel.  Atomics are used only where the result is an integer sum (the
// counters of dropped triangles, the triangles per tile) or where the order does not reach the output (the slot a triangle takes in
// its tile's list: the winner is a minimum).  Every array an atomic wrote is read by a LATER launch only.
//
//   project: one thread per vertex -> (X, Y, bits of w), w = 0 for a vertex that is not usable.
//   count:   one thread per triangle: classify it (rs_classify, the one statement of what is kept), count the dropped ones by cause,
//            add 1 to every tile its pixel bounding box meets.
//   bin:     the same walk again, now with the caller's prefix sum: triangle t goes to bin[tile_offset[tile] + cursor[tile]++].
//   resolve: one workgroup of 256 threads per 16 x 16 tile, one pixel per thread.  The tile's list is staged through LDS kRasterChunk
//            triangles at a time: every thread sets one triangle up (the three edge functions at the tile's first sample as int64,
//            their steps per pixel as int32, 1 / w per corner, the ownership bits), then all threads walk the chunk, every read an
//            LDS broadcast.  A thread tests its own sample with three 64-bit multiply-adds per edge pair and forms a depth only
//            where the sample is covered.  The barycentrics are formed once, for the winner, after the walk.
//
// fp contraction is off in the whole file: every product and sum below rounds on its own, as the model's numpy scalars do.  They are
// written with the plain operators: HIP's __fmul_rn / __dadd_rn and their kin are inline functions of a header compiled with
// contraction on, and a product and a sum that both come from there fuse after inlining (common.h).
#include "common.h"
#include "launch.h"
#include "wave.h"
#include "mesh_raster_plan.h"
#include "vqn_mesh_raster.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = kRasterThreads;
constexpr int kPerCu = 8;                 // grid-stride above this many workgroups per CU
constexpr unsigned long long kBackgroundKey = (0x7f800000ull << 32) | 0xffffffffull;      // depth +inf, face -1

struct RsCamera {
  float p[12];
};

__device__ __forceinline__ bool in_range(const int x, const int n) { return (unsigned)x < (unsigned)n; }

// ---- vertices -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void rs_project_kernel(const float* __restrict__ verts, const long V, const RsCamera cam, const float near_plane,
                                                              int* __restrict__ pverts) {
  for (long v = (long)blockIdx.x * kThreads + threadIdx.x; v < V; v += (long)gridDim.x * kThreads) {
    const float x = verts[3 * v], y = verts[3 * v + 1], z = verts[3 * v + 2];
    float h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float* p = cam.p + 4 * r;
      h[r] = ((p[0] * x + p[1] * y) + p[2] * z) + p[3];
    }
    const float w = h[2];
    const float fx = (h[0] / w) * (float)kRasterSubpixel, fy = (h[1] / w) * (float)kRasterSubpixel;
    // (a NaN fails every comparison: not usable)
    const bool usable = isfinite(w) && w >= near_plane && fabsf(fx) < (float)kRasterCoordLimit && fabsf(fy) < (float)kRasterCoordLimit;
    pverts[3 * v] = usable ? (int)rintf(fx) : 0;
    pverts[3 * v + 1] = usable ? (int)rintf(fy) : 0;
    pverts[3 * v + 2] = usable ? __float_as_int(w) : 0;
  }
}

// ---- the one statement of which triangles are kept ----------------------------------------------------------------------------------
struct RsTri {
  long long X[3], Y[3];
  float w[3];
  long long area_abs;
  int s;                  // sign(area2)
};

// -> 0 kept, else 1 + the slot of stats that counts the cause
__device__ __forceinline__ int rs_classify(const int* __restrict__ tris, const long t, const int V, const int* __restrict__ pverts, const int cull,
                                           RsTri* g) {
  const int idx[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
  if (!(in_range(idx[0], V) && in_range(idx[1], V) && in_range(idx[2], V))) return 1;
  bool usable = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g->X[k] = pverts[3 * (long)idx[k]];
    g->Y[k] = pverts[3 * (long)idx[k] + 1];
    g->w[k] = __int_as_float(pverts[3 * (long)idx[k] + 2]);
    usable = usable && g->w[k] > 0.0f;
  }
  if (!usable) return 2;
  const long long area2 = (g->X[1] - g->X[0]) * (g->Y[2] - g->Y[0]) - (g->X[2] - g->X[0]) * (g->Y[1] - g->Y[0]);
  if (area2 == 0) return 3;
  g->s = area2 > 0 ? 1 : -1;
  if (g->s == cull) return 4;
  g->area_abs = area2 > 0 ? area2 : -area2;
  return 0;
}

// the tiles the pixel bounding box of a kept triangle meets: [tx0, tx1] x [ty0, ty1]; false: none
__device__ __forceinline__ bool rs_tile_rect(const RsTri& g, const int H, const int W, int* tx0, int* tx1, int* ty0, int* ty1) {
  const long long min_x = min(g.X[0], min(g.X[1], g.X[2])), max_x = max(g.X[0], max(g.X[1], g.X[2]));
  const long long min_y = min(g.Y[0], min(g.Y[1], g.Y[2])), max_y = max(g.Y[0], max(g.Y[1], g.Y[2]));
  // the pixels j with min_x <= 256 j <= max_x: ceil and floor by arithmetic shifts, which round towards -inf
  const long long j0 = max((min_x + kRasterSubpixel - 1) >> kRasterSubpixelBits, 0ll), j1 = min(max_x >> kRasterSubpixelBits, (long long)W - 1);
  const long long i0 = max((min_y + kRasterSubpixel - 1) >> kRasterSubpixelBits, 0ll), i1 = min(max_y >> kRasterSubpixelBits, (long long)H - 1);
  if (j0 > j1 || i0 > i1) return false;
  *tx0 = (int)(j0 / kRasterTile), *tx1 = (int)(j1 / kRasterTile), *ty0 = (int)(i0 / kRasterTile), *ty1 = (int)(i1 / kRasterTile);
  return true;
}

// edge k runs from corner (k + 1) % 3 to corner (k + 2) % 3 and weighs corner k.  E_k(p) = a p.x + b p.y + c; *e_at: its value at
// the sample (px, py), in sub-pixel units; -> whether the edge owns its boundary
__device__ __forceinline__ bool rs_edge(const RsTri& g, const int k, const long long px, const long long py, int* a, int* b, long long* e_at) {
  const int i0 = k == 2 ? 0 : k + 1, i1 = k == 0 ? 2 : k - 1;
  const long long dx = g.s * (g.X[i1] - g.X[i0]), dy = g.s * (g.Y[i1] - g.Y[i0]);
  *a = (int)-dy, *b = (int)dx;
  *e_at = dx * (py - g.Y[i0]) - dy * (px - g.X[i0]);
  return dy > 0 || (dy == 0 && dx < 0);
}

__device__ __forceinline__ double rs_s(const long long e0, const long long e1, const long long e2, const double q0, const double q1, const double q2) {
  return ((double)e0 * q0 + (double)e1 * q1) + (double)e2 * q2;
}

__global__ __launch_bounds__(kThreads) void rs_count_kernel(const int* __restrict__ tris, const long T, const int V, const int* __restrict__ pverts,
                                                            const int H, const int W, const int cull, const int tiles_x, int* __restrict__ tile_count,
                                                            int* __restrict__ stats) {
  int dropped[kRasterStats] = {0, 0, 0, 0};
  for (long t0 = (long)blockIdx.x * kThreads; t0 < T; t0 += (long)gridDim.x * kThreads) {
    const long t = t0 + threadIdx.x;
    if (t >= T) continue;
    RsTri g;
    const int cause = rs_classify(tris, t, V, pverts, cull, &g);
#pragma unroll
    for (int c = 0; c < kRasterStats; ++c) dropped[c] += cause == c + 1;
    int tx0, tx1, ty0, ty1;
    if (cause || !rs_tile_rect(g, H, W, &tx0, &tx1, &ty0, &ty1)) continue;
    for (int ty = ty0; ty <= ty1; ++ty)
      for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(tile_count + ty * tiles_x + tx, 1);
  }
#pragma unroll
  for (int c = 0; c < kRasterStats; ++c) {
    const int n = wave_sum(dropped[c]);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(stats + c, n);
  }
}

__global__ __launch_bounds__(kThreads) void rs_bin_kernel(const int* __restrict__ tris, const long T, const int V, const int* __restrict__ pverts,
                                                          const int H, const int W, const int cull, const int tiles_x, const long tiles,
                                                          const int* __restrict__ tile_offset, const long n_pairs, int* __restrict__ cursor,
                                                          int* __restrict__ bin) {
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long)gridDim.x * kThreads) {
    RsTri g;
    int tx0, tx1, ty0, ty1;
    if (rs_classify(tris, t, V, pverts, cull, &g) || !rs_tile_rect(g, H, W, &tx0, &tx1, &ty0, &ty1)) continue;
    for (int ty = ty0; ty <= ty1; ++ty)
      for (int tx = tx0; tx <= tx1; ++tx) {
        const long tile = (long)ty * tiles_x + tx;
        const long first = tile_offset[tile], end = tile + 1 < tiles ? (long)tile_offset[tile + 1] : n_pairs;
        const long pos = first + atomicAdd(cursor + tile, 1);
        if (pos >= first && pos >= 0 && pos < end && pos < n_pairs) bin[pos] = (int)t;     // (always, for offsets that belong to these counts)
      }
  }
}

// ---- resolve ------------------------------------------------------------------------------------------------------------------------
struct alignas(16) RsEdges {
  long long f[3];         // E_k - (edge k owns its boundary ? 0 : 1) at the tile's first sample
  int a[3], b[3];         // its steps per sub-pixel unit in x and y
};
static_assert(sizeof(RsEdges) == 48, "three 16-byte reads");

__global__ __launch_bounds__(kThreads) void rs_resolve_kernel(const int* __restrict__ tris, const long T, const int V, const int* __restrict__ pverts,
                                                              const int H, const int W, const int cull, const int tiles_x, const long tiles,
                                                              const int* __restrict__ tile_offset, const long n_pairs, const int* __restrict__ bin,
                                                              int* __restrict__ face, float* __restrict__ depth, float* __restrict__ bary) {
  // the staged chunk; f = E - (the edge owns its boundary ? 0 : 1) at the tile's first sample, so covered <=> every f >= 0
  // (the part every sample reads is one 48-byte row, three 16-byte LDS reads; the rest is read where a sample is covered)
  __shared__ RsEdges s_edges[kRasterChunk];
  __shared__ double s_q[3][kRasterChunk];
  __shared__ long long s_area[kRasterChunk];
  __shared__ int s_face[kRasterChunk], s_notown[kRasterChunk];
  static_assert(sizeof(s_edges) + sizeof(s_q) + sizeof(s_area) + sizeof(s_face) + sizeof(s_notown) == kRasterLdsBytes,
                "the plan states the LDS of this kernel");
  const int lx = threadIdx.x % kRasterTile, ly = threadIdx.x / kRasterTile;
  const int step_x = lx * kRasterSubpixel, step_y = ly * kRasterSubpixel;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long)ty * tiles_x);
    const int i = ty * kRasterTile + ly, j = tx * kRasterTile + lx;
    const long long ox = (long long)tx * kRasterTile * kRasterSubpixel, oy = (long long)ty * kRasterTile * kRasterSubpixel;
    long first = tile_offset[tile], end = tile + 1 < tiles ? (long)tile_offset[tile + 1] : n_pairs;
    if (first < 0 || end > n_pairs || end < first) first = end = 0;             // (never, for offsets that belong to these counts)
    unsigned long long best = kBackgroundKey;
    for (long c0 = first; c0 < end; c0 += kRasterChunk) {                        // workgroup-uniform
      const int n = (int)min((long)kRasterChunk, end - c0);
      __syncthreads();                                                           // the walk before is over
      for (int m = threadIdx.x; m < n; m += kThreads) {
        const int t = bin[c0 + m];
        RsTri g;
        const bool kept = (unsigned long long)t < (unsigned long long)T && rs_classify(tris, t, V, pverts, cull, &g) == 0;
        int notown = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          int a = 0, b = 0;
          long long e = -1;
          bool owns = true;
          if (kept) owns = rs_edge(g, k, ox, oy, &a, &b, &e);
          notown |= (owns ? 0 : 1) << k;
          s_edges[m].a[k] = a, s_edges[m].b[k] = b;
          s_edges[m].f[k] = e - (owns ? 0 : 1);                                  // (not kept: -1, never covered)
          s_q[k][m] = kept ? 1.0 / (double)g.w[k] : 0.0;
        }
        s_area[m] = kept ? g.area_abs : 0;
        s_face[m] = kept ? t : -1;
        s_notown[m] = notown;
      }
      __syncthreads();
      for (int m = 0; m < n; ++m) {
        const RsEdges r = s_edges[m];
        const long long f0 = r.f[0] + (long long)r.a[0] * step_x + (long long)r.b[0] * step_y;
        const long long f1 = r.f[1] + (long long)r.a[1] * step_x + (long long)r.b[1] * step_y;
        const long long f2 = r.f[2] + (long long)r.a[2] * step_x + (long long)r.b[2] * step_y;
        if ((f0 | f1 | f2) < 0) continue;
        const int notown = s_notown[m];
        const double s = rs_s(f0 + (notown & 1), f1 + ((notown >> 1) & 1), f2 + ((notown >> 2) & 1), s_q[0][m], s_q[1][m], s_q[2][m]);
        const float d = (float)((double)s_area[m] / s);
        const unsigned long long key = ((unsigned long long)(unsigned)__float_as_int(d) << 32) | (unsigned)s_face[m];
        best = min(best, key);
      }
    }
    if (i >= H || j >= W) continue;
    const long pix = (long)i * W + j;
    const int winner = (int)(unsigned)(best & 0xffffffffull);
    float out_b[3] = {0.0f, 0.0f, 0.0f};
    RsTri g;
    if (winner >= 0 && rs_classify(tris, winner, V, pverts, cull, &g) == 0) {    // (a winner was kept when it was staged)
      long long e[3];
      double q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        int a, b;
        rs_edge(g, k, (long long)j * kRasterSubpixel, (long long)i * kRasterSubpixel, &a, &b, &e[k]);
        q[k] = 1.0 / (double)g.w[k];
      }
      const double s = rs_s(e[0], e[1], e[2], q[0], q[1], q[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) out_b[k] = (float)(((double)e[k] * q[k]) / s);
    }
    face[pix] = winner;
    depth[pix] = __int_as_float((int)(unsigned)(best >> 32));
    bary[3 * pix] = out_b[0], bary[3 * pix + 1] = out_b[1], bary[3 * pix + 2] = out_b[2];
  }
}

// ---- attributes ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void rs_interpolate_kernel(const int* __restrict__ face, const float* __restrict__ bary, const long pixels,
                                                                  const int* __restrict__ tris, const long T, const float* __restrict__ attr, const int V,
                                                                  const int C, const float* __restrict__ background, const int nearest,
                                                                  float* __restrict__ out) {
  const long n = pixels * C;
  for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long)gridDim.x * kThreads) {
    const long pix = e / C;
    const int c = (int)(e - pix * C);
    const int f = face[pix];
    float r = background[c];
    if ((unsigned long long)f < (unsigned long long)T) {
      const int v0 = tris[3 * (long)f], v1 = tris[3 * (long)f + 1], v2 = tris[3 * (long)f + 2];
      if (in_range(v0, V) && in_range(v1, V) && in_range(v2, V)) {
        const float b0 = bary[3 * pix], b1 = bary[3 * pix + 1], b2 = bary[3 * pix + 2];
        const float a0 = attr[(long)v0 * C + c], a1 = attr[(long)v1 * C + c], a2 = attr[(long)v2 * C + c];
        if (nearest)
          r = (b0 >= b1 && b0 >= b2) ? a0 : (b1 >= b2 ? a1 : a2);
        else
          r = (b0 * a0 + b1 * a1) + b2 * a2;
      }
    }
    out[e] = r;
  }
}

dim3 rs_grid(const int64_t n) { return dim3((unsigned)vqn_grid1((long)((n + kThreads - 1) / kThreads), kPerCu)); }

}  // namespace

extern "C" int vqn_raster_count(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const float* P, int H, int W, float near,
                                int cull, int32_t* pverts, int32_t* tile_count, int32_t* stats, void* stream) {
  RasterPlan g;
  char msg[200];
  if (const int rc = raster_count_plan(verts, n_verts, tris, n_tris, P, H, W, near, cull, pverts, tile_count, stats, &g, msg, sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  const hipStream_t s = (hipStream_t)stream;
  VQN_HIP(hipMemsetAsync(tile_count, 0, sizeof(int32_t) * (size_t)g.tiles, s));
  VQN_HIP(hipMemsetAsync(stats, 0, sizeof(int32_t) * kRasterStats, s));
  if (n_verts > 0) {
    RsCamera cam;
    memcpy(cam.p, P, sizeof(cam.p));
    if (int e = vqn_launch(__func__, rs_project_kernel, rs_grid(n_verts), kThreads, 0, stream, verts, (long)n_verts, cam, near, pverts)) return e;
  }
  if (n_tris > 0)
    if (int e = vqn_launch(__func__, rs_count_kernel, rs_grid(n_tris), kThreads, 0, stream, tris, (long)n_tris, (int)n_verts, (const int*)pverts, H, W,
                           cull, g.tiles_x, tile_count, stats))
      return e;
  return VQN_OK;
}

extern "C" int vqn_raster_resolve(const int32_t* tris, int64_t n_tris, const int32_t* pverts, int64_t n_verts, int H, int W, int cull,
                                  const int32_t* tile_offset, int64_t n_pairs, int32_t* cursor, int32_t* bin, int32_t* face, float* depth,
                                  float* bary, void* stream) {
  RasterPlan g;
  char msg[200];
  if (const int rc = raster_resolve_plan(tris, n_tris, pverts, n_verts, H, W, cull, tile_offset, n_pairs, cursor, bin, face, depth, bary, &g, msg,
                                         sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  const hipStream_t s = (hipStream_t)stream;
  VQN_HIP(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)g.tiles, s));
  if (n_pairs > 0)
    if (int e = vqn_launch(__func__, rs_bin_kernel, rs_grid(n_tris), kThreads, 0, stream, tris, (long)n_tris, (int)n_verts, pverts, H, W, cull,
                           g.tiles_x, (long)g.tiles, tile_offset, (long)n_pairs, cursor, bin))
      return e;
  return vqn_launch(__func__, rs_resolve_kernel, dim3((unsigned)vqn_grid1((long)g.tiles, kPerCu)), kThreads, 0, stream, tris, (long)n_tris,
                    (int)n_verts, pverts, H, W, cull, g.tiles_x, (long)g.tiles, tile_offset, (long)n_pairs, (const int*)bin, face, depth, bary);
}

extern "C" int vqn_raster_interpolate(const int32_t* face, const float* bary, int H, int W, const int32_t* tris, int64_t n_tris, const float* attr,
                                      int64_t n_verts, int n_channels, const float* background, int nearest, float* out, void* stream) {
  RasterPlan g;
  char msg[200];
  if (const int rc = raster_interpolate_plan(face, bary, H, W, tris, n_tris, attr, n_verts, n_channels, background, out, &g, msg, sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  return vqn_launch(__func__, rs_interpolate_kernel, rs_grid(g.pixels * n_channels), kThreads, 0, stream, face, bary, (long)g.pixels, tris,
                    (long)n_tris, attr, (int)n_verts, n_channels, background, nearest, out);
}
