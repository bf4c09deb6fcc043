// Ray queries against a triangle mesh for gfx950 (include/vqn_mesh_rays.h; the host side is csrc/mesh_rays_plan.h, the plain
// statement tests/mesh_rays_model.py; geo/mesh_rays.py): the nearest hit of a ray, whether a segment is occluded, and the fused light
// visibility of surface points.  DESIGN.md section 18.
//
// A uniform grid holds per cell the list of the triangles whose box, widened by 1 / 16 cell, meets it; one lane walks one ray
// through the cells by a 3-D DDA and tests the triangles of every cell it visits with the header's statement of a hit.  A hit is
// taken wherever along the ray it lies, not only inside the visited cell: the nearest hit is the minimum of a 64-bit key and "any
// hit" is a boolean, so neither depends on the order or on how often a triangle is met.  Atomics are used only where the result is
// an integer sum (the counters of dropped triangles, the triangles per cell) or where the order does not reach the output (the slot
// a triangle takes in its cell's list).  Every array an atomic wrote is read by a LATER launch only.
//
//   count:  one thread per triangle: classify it (rays_classify, the one statement of what is kept), count the dropped ones by
//           cause, add 1 to every cell of its widened box.
//   bin:    the same walk again with the caller's prefix sum: triangle t goes to bin[cell_offset[cell] + cursor[cell]++]; and the
//           packed record (v0, e1, e2) of every triangle, NaN for a dropped one -- a NaN misses, so the queries check no index.
//   walk:   rays_walk.  The crossing parameter of a cell plane is recomputed from the integer plane index at every step, so the
//           DDA accumulates no error; the walk ends when the entry parameter of the next cell exceeds what can still matter, when
//           it leaves the grid, or after dims[0] + dims[1] + dims[2] + 3 steps whatever the inputs.
//   light visibility: lanes = 64 neighbouring points of one light (coherent rays; a 64 x 64 tile of `out` is staged in LDS and
//           written as whole 256-byte rows), or lanes = 64 lights of one point (a fan of rays; the wave writes 256 contiguous bytes).
//
// fp contraction is off in the whole file: every product and sum below rounds on its own, as the model's numpy scalars do (written
// with the plain operators, see mesh_raster.hip).
#include "common.h"
#include "launch.h"
#include "wave.h"
#include "mesh_rays_plan.h"
#include "vqn_mesh_rays.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = kRaysThreads;
constexpr int kPerCu = 8;                                      // grid-stride above this many workgroups per CU
constexpr unsigned long long kMissKey = (0x7f800000ull << 32) | 0xffffffffull;      // t +inf, face -1
constexpr float kMinDir = 8.673617379884035e-19f;              // 2^-60
constexpr float kWalkedRatio = 9.313225746154785e-10f;         // 2^-30: an axis is walked iff |d_a| >= 2^-30 max |d|
static_assert(VQN_RAYS_MIN_DIR_LOG2 == -60, "kMinDir restates the header");

struct RaysGrid {                                              // struct VqnGeomGrid by value, with the flat strides
  float o[3], h;
  int dims[3], cells;
};

struct RaysScene {
  const float4* packed;
  long T;
  RaysGrid g;
  const int* cell_offset;
  long n_pairs;
  const int* bin;
};

RaysGrid rays_grid(const VqnGeomGrid* g) {
  RaysGrid r;
  for (int a = 0; a < 3; ++a) r.o[a] = g->origin[a], r.dims[a] = g->dims[a];
  r.h = g->h, r.cells = g->cells;
  return r;
}

__device__ __forceinline__ bool in_range(const int x, const int n) { return (unsigned)x < (unsigned)n; }
__device__ __forceinline__ float cross_c(const float a, const float b, const float c, const float d) { return a * b - c * d; }

// floor(x) clamped into [0, n - 1], the clamp in float: an infinity lands on an end, a NaN on 0
__device__ __forceinline__ int cell_clamp(const float x, const int n) { return (int)fminf(fmaxf(floorf(x), 0.0f), (float)(n - 1)); }

// ---- the one statement of which triangles are kept -------------------------------------------------------------------------------------
struct RaysTri {
  float v0[3], e1[3], e2[3], lo[3], hi[3];
};

// -> 0 kept, else 1 + the slot of stats that counts the cause
__device__ __forceinline__ int rays_classify(const int* __restrict__ tris, const long t, const int V, const float* __restrict__ verts, RaysTri* g) {
  const int idx[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
  if (!(in_range(idx[0], V) && in_range(idx[1], V) && in_range(idx[2], V))) return 1;
  float v[3][3];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[k][a] = verts[3 * (long)idx[k] + a];
      finite = finite && isfinite(v[k][a]);
    }
  if (!finite) return 2;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g->v0[a] = v[0][a], g->e1[a] = v[1][a] - v[0][a], g->e2[a] = v[2][a] - v[0][a];
    g->lo[a] = fminf(v[0][a], fminf(v[1][a], v[2][a])), g->hi[a] = fmaxf(v[0][a], fmaxf(v[1][a], v[2][a]));
  }
  const float nx = cross_c(g->e1[1], g->e2[2], g->e1[2], g->e2[1]), ny = cross_c(g->e1[2], g->e2[0], g->e1[0], g->e2[2]),
              nz = cross_c(g->e1[0], g->e2[1], g->e1[1], g->e2[0]);
  if (nx == 0.0f && ny == 0.0f && nz == 0.0f) return 3;
  return 0;
}

// the cells a kept triangle is listed in: [c0[a], c1[a]] per axis (never empty: both ends are clamped into the grid)
__device__ __forceinline__ void rays_cell_box(const RaysTri& g, const RaysGrid& grid, int c0[3], int c1[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c0[a] = cell_clamp((g.lo[a] - grid.o[a]) / grid.h - kRaysMargin, grid.dims[a]);
    c1[a] = cell_clamp((g.hi[a] - grid.o[a]) / grid.h + kRaysMargin, grid.dims[a]);
  }
}

__global__ __launch_bounds__(kThreads) void rays_count_kernel(const float* __restrict__ verts, const int V, const int* __restrict__ tris, const long T,
                                                              const RaysGrid grid, int* __restrict__ cell_count, int* __restrict__ stats) {
  int dropped[kRaysStats] = {0, 0, 0};
  for (long t0 = (long)blockIdx.x * kThreads; t0 < T; t0 += (long)gridDim.x * kThreads) {
    const long t = t0 + threadIdx.x;
    if (t >= T) continue;
    RaysTri g;
    const int cause = rays_classify(tris, t, V, verts, &g);
#pragma unroll
    for (int c = 0; c < kRaysStats; ++c) dropped[c] += cause == c + 1;
    if (cause) continue;
    int c0[3], c1[3];
    rays_cell_box(g, grid, c0, c1);
    for (int k = c0[2]; k <= c1[2]; ++k)
      for (int j = c0[1]; j <= c1[1]; ++j)
        for (int i = c0[0]; i <= c1[0]; ++i) atomicAdd(cell_count + ((long)k * grid.dims[1] + j) * grid.dims[0] + i, 1);
  }
#pragma unroll
  for (int c = 0; c < kRaysStats; ++c) {
    const int n = wave_sum(dropped[c]);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(stats + c, n);
  }
}

__global__ __launch_bounds__(kThreads) void rays_bin_kernel(const float* __restrict__ verts, const int V, const int* __restrict__ tris, const long T,
                                                            const RaysGrid grid, const int* __restrict__ cell_offset, const long n_pairs,
                                                            int* __restrict__ cursor, int* __restrict__ bin, float4* __restrict__ packed) {
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long)gridDim.x * kThreads) {
    RaysTri g;
    const bool kept = rays_classify(tris, t, V, verts, &g) == 0;
    const float nan = __int_as_float(0x7fc00000);
    packed[3 * t] = kept ? make_float4(g.v0[0], g.v0[1], g.v0[2], g.e1[0]) : make_float4(nan, nan, nan, nan);
    packed[3 * t + 1] = kept ? make_float4(g.e1[1], g.e1[2], g.e2[0], g.e2[1]) : make_float4(nan, nan, nan, nan);
    packed[3 * t + 2] = kept ? make_float4(g.e2[2], 0.0f, 0.0f, 0.0f) : make_float4(nan, nan, nan, nan);
    if (!kept) continue;
    int c0[3], c1[3];
    rays_cell_box(g, grid, c0, c1);
    for (int k = c0[2]; k <= c1[2]; ++k)
      for (int j = c0[1]; j <= c1[1]; ++j)
        for (int i = c0[0]; i <= c1[0]; ++i) {
          const long cell = ((long)k * grid.dims[1] + j) * grid.dims[0] + i;
          const long first = cell_offset[cell], end = cell + 1 < grid.cells ? (long)cell_offset[cell + 1] : n_pairs;
          const long pos = first + atomicAdd(cursor + cell, 1);
          if (pos >= first && pos >= 0 && pos < end && pos < n_pairs) bin[pos] = (int)t;     // (always, for offsets that belong to these counts)
        }
  }
}

// ---- the statement of a hit ------------------------------------------------------------------------------------------------------------
struct RaysRay {
  float o[3], d[3], tmin, tmax;
};

__device__ __forceinline__ bool rays_hit(const float4 r0, const float4 r1, const float4 r2, const RaysRay& r, float* t, float* u, float* v) {
  const float v0x = r0.x, v0y = r0.y, v0z = r0.z, e1x = r0.w, e1y = r1.x, e1z = r1.y, e2x = r1.z, e2y = r1.w, e2z = r2.x;
  const float px = cross_c(r.d[1], e2z, r.d[2], e2y), py = cross_c(r.d[2], e2x, r.d[0], e2z), pz = cross_c(r.d[0], e2y, r.d[1], e2x);
  const float det = (e1x * px + e1y * py) + e1z * pz;
  const float inv = 1.0f / det;
  const float sx = r.o[0] - v0x, sy = r.o[1] - v0y, sz = r.o[2] - v0z;
  *u = ((sx * px + sy * py) + sz * pz) * inv;
  const float qx = cross_c(sy, e1z, sz, e1y), qy = cross_c(sz, e1x, sx, e1z), qz = cross_c(sx, e1y, sy, e1x);
  *v = ((r.d[0] * qx + r.d[1] * qy) + r.d[2] * qz) * inv;
  *t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
  // (every comparison with a NaN is false, and det != 0 alone lets none through: u of a NaN det is a NaN)
  return det != 0.0f && *u >= 0.0f && *v >= 0.0f && (*u + *v) <= 1.0f && *t > r.tmin && *t < r.tmax;
}

// whether the ray is cast at all (the header's statement of a ray)
__device__ __forceinline__ bool rays_valid(const RaysRay& r) {
  const float dmax = fmaxf(fabsf(r.d[0]), fmaxf(fabsf(r.d[1]), fabsf(r.d[2])));
  return isfinite(r.o[0]) && isfinite(r.o[1]) && isfinite(r.o[2]) && isfinite(r.d[0]) && isfinite(r.d[1]) && isfinite(r.d[2]) &&
         isfinite(r.tmin) && r.tmin >= 0.0f && r.tmin < r.tmax && dmax >= kMinDir;
}

struct RaysBest {
  unsigned long long key;
  float u, v;
};

// One ray through the grid.  kAny: -> whether any triangle is hit.  Else *best takes the least key and its (u, v); -> key != miss.
template <bool kAny>
__device__ __forceinline__ bool rays_walk(const RaysScene& sc, const RaysRay& r, RaysBest* best) {
  best->key = kMissKey, best->u = 0.0f, best->v = 0.0f;
  if (!rays_valid(r)) return false;
  const RaysGrid& g = sc.g;
  const float dmax = fmaxf(fabsf(r.d[0]), fmaxf(fabsf(r.d[1]), fabsf(r.d[2])));
  const float walked_min = dmax * kWalkedRatio;                // (exact: a power of two, and dmax >= 2^-60)
  float inv[3], tn[3], t_enter = r.tmin, t_exit = r.tmax;
  int step[3], c[3];
  // the slab test against the grid's own box: the mesh lies h / 2 inside it, far more than the rounding of these products
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = g.o[a], hi = g.o[a] + (float)g.dims[a] * g.h;
    const bool walked = fabsf(r.d[a]) >= walked_min;
    inv[a] = walked ? 1.0f / r.d[a] : 0.0f;
    step[a] = walked ? (r.d[a] > 0.0f ? 1 : -1) : 0;
    if (walked) {
      const float ta = (lo - r.o[a]) * inv[a], tb = (hi - r.o[a]) * inv[a];
      t_enter = fmaxf(t_enter, fminf(ta, tb)), t_exit = fminf(t_exit, fmaxf(ta, tb));
    } else if (r.o[a] < lo || r.o[a] > hi) {
      return false;
    }
  }
  if (!(t_enter <= t_exit)) return false;
  // the cell of the entry point, clamped, and per walked axis the parameter at which the ray leaves that cell
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = step[a] ? r.o[a] + t_enter * r.d[a] : r.o[a];
    c[a] = cell_clamp((p - g.o[a]) / g.h, g.dims[a]);
    tn[a] = step[a] ? ((g.o[a] + (float)(c[a] + (step[a] > 0 ? 1 : 0)) * g.h) - r.o[a]) * inv[a] : INFINITY;
  }
  const float slack = (kRaysMargin * g.h) / dmax;
  const int max_steps = g.dims[0] + g.dims[1] + g.dims[2] + 3;
  for (int it = 0; it < max_steps; ++it) {
    const long cell = ((long)c[2] * g.dims[1] + c[1]) * g.dims[0] + c[0];
    long first = sc.cell_offset[cell], end = cell + 1 < g.cells ? (long)sc.cell_offset[cell + 1] : sc.n_pairs;
    if (first < 0 || end > sc.n_pairs || end < first) first = end = 0;           // (never, for offsets that belong to the counts)
    for (long j = first; j < end; ++j) {
      const int t = sc.bin[j];
      if ((unsigned long long)t >= (unsigned long long)sc.T) continue;
      const float4 r0 = sc.packed[3 * (long)t], r1 = sc.packed[3 * (long)t + 1], r2 = sc.packed[3 * (long)t + 2];
      float ht, hu, hv;
      if (!rays_hit(r0, r1, r2, r, &ht, &hu, &hv)) continue;
      if (kAny) return true;
      const unsigned long long key = ((unsigned long long)(unsigned)__float_as_int(ht) << 32) | (unsigned)t;
      if (key < best->key) best->key = key, best->u = hu, best->v = hv;
    }
    // the next cell is entered at the least of the three crossings; stop once nothing at or beyond it can matter
    const float t_next = fminf(tn[0], fminf(tn[1], tn[2]));
    const float t_best = __int_as_float((int)(unsigned)(best->key >> 32));     // (+inf while nothing is hit)
    const float limit = kAny ? t_exit : fminf(t_exit, t_best + slack);
    if (!(t_next <= limit)) break;
    // (selects, not an index that the lane computes: the three axes stay in registers)
    const bool sx = tn[0] <= tn[1] && tn[0] <= tn[2], sy = !sx && tn[1] <= tn[2], sz = !sx && !sy;
    c[0] += sx ? step[0] : 0, c[1] += sy ? step[1] : 0, c[2] += sz ? step[2] : 0;
    if (!in_range(c[0], g.dims[0]) || !in_range(c[1], g.dims[1]) || !in_range(c[2], g.dims[2])) break;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const bool stepped = a == 0 ? sx : (a == 1 ? sy : sz);
      if (stepped) tn[a] = ((g.o[a] + (float)(c[a] + (step[a] > 0 ? 1 : 0)) * g.h) - r.o[a]) * inv[a];
    }
  }
  return best->key != kMissKey;
}

// ---- cast / occluded -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ RaysRay rays_load(const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ tmin,
                                             const float* __restrict__ tmax, const long i) {
  RaysRay r;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.o[a] = o[3 * i + a], r.d[a] = d[3 * i + a];
  r.tmin = tmin[i], r.tmax = tmax[i];
  return r;
}

__global__ __launch_bounds__(kThreads) void rays_cast_kernel(const RaysScene sc, const float* __restrict__ o, const float* __restrict__ d,
                                                             const float* __restrict__ tmin, const float* __restrict__ tmax, const long n,
                                                             int* __restrict__ face, float* __restrict__ t, float* __restrict__ uv) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const RaysRay r = rays_load(o, d, tmin, tmax, i);
    RaysBest best;
    rays_walk<false>(sc, r, &best);
    face[i] = (int)(unsigned)(best.key & 0xffffffffull);
    t[i] = __int_as_float((int)(unsigned)(best.key >> 32));
    uv[2 * i] = best.u, uv[2 * i + 1] = best.v;
  }
}

__global__ __launch_bounds__(kThreads) void rays_occluded_kernel(const RaysScene sc, const float* __restrict__ o, const float* __restrict__ d,
                                                                 const float* __restrict__ tmin, const float* __restrict__ tmax, const long n,
                                                                 unsigned char* __restrict__ occ) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const RaysRay r = rays_load(o, d, tmin, tmax, i);
    RaysBest best;
    occ[i] = rays_walk<true>(sc, r, &best) ? 1 : 0;
  }
}

// ---- light visibility ------------------------------------------------------------------------------------------------------------------
// the header's statement per (point, light): -> 1.0f visible, 0.0f not
__device__ __forceinline__ float rays_light(const RaysScene& sc, const float p[3], const float nrm[3], const float bias, const float lx, const float ly,
                                            const float lz) {
  RaysRay r;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.o[a] = p[a] + bias * nrm[a];
  const float dlx = lx - r.o[0], dly = ly - r.o[1], dlz = lz - r.o[2];
  const float dist = sqrtf((dlx * dlx + dly * dly) + dlz * dlz);
  r.d[0] = dlx / dist, r.d[1] = dly / dist, r.d[2] = dlz / dist;
  r.tmin = 0.0f, r.tmax = dist;
  const bool front = ((r.d[0] * nrm[0] + r.d[1] * nrm[1]) + r.d[2] * nrm[2]) > 0.0f;
  if (!front) return 0.0f;
  RaysBest best;
  return rays_walk<true>(sc, r, &best) ? 0.0f : 1.0f;
}

// lanes = points: a workgroup owns 64 points; per chunk of 64 lights, wave w casts lights w, w + 4, ... of the chunk for the 64
// points (one point per lane) into the LDS tile, then the 256 threads write the tile as rows of 64 lights (256 contiguous bytes)
__global__ __launch_bounds__(kThreads) void rays_light_points_kernel(const RaysScene sc, const float* __restrict__ points,
                                                                     const float* __restrict__ normals, const long n, const float* __restrict__ lights,
                                                                     const int L, const float bias, float* __restrict__ out) {
  __shared__ float s_vis[kRaysTile][kRaysTile + 1];            // [light of the chunk][point of the tile]; + 1: the row-wise read below
  static_assert(sizeof(s_vis) == kRaysLdsBytes, "the plan states the LDS of this kernel");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kWaves = kThreads / 64;
  const long tiles = (n + kRaysTile - 1) / kRaysTile;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long i = tile * kRaysTile + lane;
    float p[3] = {0.0f, 0.0f, 0.0f}, nrm[3] = {0.0f, 0.0f, 0.0f};
    if (i < n) {
#pragma unroll
      for (int a = 0; a < 3; ++a) p[a] = points[3 * i + a], nrm[a] = normals[3 * i + a];
    }
    for (int l0 = 0; l0 < L; l0 += kRaysTile) {                                  // workgroup-uniform
      const int nl = min(kRaysTile, L - l0);
      __syncthreads();                                                           // the rows of the chunk before are written
      for (int k = wave; k < nl; k += kWaves) {                                  // wave-uniform
        const float* l = lights + 3 * (long)(l0 + k);
        s_vis[k][lane] = i < n ? rays_light(sc, p, nrm, bias, l[0], l[1], l[2]) : 0.0f;
      }
      __syncthreads();
      for (int row = wave; row < kRaysTile; row += kWaves) {
        const long pi = tile * kRaysTile + row;
        if (pi < n && lane < nl) out[pi * L + l0 + lane] = s_vis[lane][row];
      }
    }
  }
}

// lanes = lights: a wave owns one point and 64 consecutive lights
__global__ __launch_bounds__(kThreads) void rays_light_lights_kernel(const RaysScene sc, const float* __restrict__ points,
                                                                     const float* __restrict__ normals, const long n, const float* __restrict__ lights,
                                                                     const int L, const float bias, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kWaves = kThreads / 64;
  const long chunks = (L + kRaysTile - 1) / kRaysTile, units = n * chunks;
  for (long unit = (long)blockIdx.x * kWaves + wave; unit < units; unit += (long)gridDim.x * kWaves) {
    const long i = unit / chunks;
    const int l = (int)(unit - i * chunks) * kRaysTile + lane;
    if (l >= L) continue;
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const float nrm[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
    out[i * L + l] = rays_light(sc, p, nrm, bias, lights[3 * (long)l], lights[3 * (long)l + 1], lights[3 * (long)l + 2]);
  }
}

dim3 rays_launch_grid(const int64_t n) { return dim3((unsigned)vqn_grid1((long)((n + kThreads - 1) / kThreads), kPerCu)); }

RaysScene rays_scene(const float* packed, int64_t T, const VqnGeomGrid* grid, const int32_t* cell_offset, int64_t n_pairs, const int32_t* bin) {
  return RaysScene{(const float4*)packed, (long)T, rays_grid(grid), cell_offset, (long)n_pairs, bin};
}

}  // namespace

extern "C" int vqn_rays_grid_plan(const float* lo, const float* hi, int64_t n_tris, float cell, struct VqnGeomGrid* grid) {
  char msg[200];
  if (const int rc = rays_grid_plan(lo, hi, n_tris, cell, grid, msg, sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  return VQN_OK;
}

extern "C" int vqn_rays_count(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const struct VqnGeomGrid* grid,
                              int32_t* cell_count, int32_t* stats, void* stream) {
  char msg[200];
  if (const int rc = rays_count_plan(verts, n_verts, tris, n_tris, grid, cell_count, stats, msg, sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  const hipStream_t s = (hipStream_t)stream;
  VQN_HIP(hipMemsetAsync(cell_count, 0, sizeof(int32_t) * (size_t)grid->cells, s));
  VQN_HIP(hipMemsetAsync(stats, 0, sizeof(int32_t) * kRaysStats, s));
  if (n_tris > 0)
    if (int e = vqn_launch(__func__, rays_count_kernel, rays_launch_grid(n_tris), kThreads, 0, stream, verts, (int)n_verts, tris, (long)n_tris,
                           rays_grid(grid), cell_count, stats))
      return e;
  return VQN_OK;
}

extern "C" int vqn_rays_bin(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const struct VqnGeomGrid* grid,
                            const int32_t* cell_offset, int64_t n_pairs, int32_t* cursor, int32_t* bin, float* packed, void* stream) {
  char msg[200];
  if (const int rc = rays_bin_plan(verts, n_verts, tris, n_tris, grid, cell_offset, n_pairs, cursor, bin, packed, msg, sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  VQN_HIP(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)grid->cells, (hipStream_t)stream));
  if (n_tris > 0)
    if (int e = vqn_launch(__func__, rays_bin_kernel, rays_launch_grid(n_tris), kThreads, 0, stream, verts, (int)n_verts, tris, (long)n_tris,
                           rays_grid(grid), cell_offset, (long)n_pairs, cursor, bin, (float4*)packed))
      return e;
  return VQN_OK;
}

extern "C" int vqn_rays_cast(const float* packed, int64_t n_tris, const struct VqnGeomGrid* grid, const int32_t* cell_offset, int64_t n_pairs,
                             const int32_t* bin, const float* o, const float* d, const float* tmin, const float* tmax, int64_t n, int32_t* face,
                             float* t, float* uv, void* stream) {
  char msg[200];
  if (const int rc = rays_cast_plan(packed, n_tris, grid, cell_offset, n_pairs, bin, o, d, tmin, tmax, n, face && t && uv, msg, sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  if (n == 0) return VQN_OK;
  return vqn_launch(__func__, rays_cast_kernel, rays_launch_grid(n), kThreads, 0, stream, rays_scene(packed, n_tris, grid, cell_offset, n_pairs, bin),
                    o, d, tmin, tmax, (long)n, face, t, uv);
}

extern "C" int vqn_rays_occluded(const float* packed, int64_t n_tris, const struct VqnGeomGrid* grid, const int32_t* cell_offset, int64_t n_pairs,
                                 const int32_t* bin, const float* o, const float* d, const float* tmin, const float* tmax, int64_t n, uint8_t* occ,
                                 void* stream) {
  char msg[200];
  if (const int rc = rays_cast_plan(packed, n_tris, grid, cell_offset, n_pairs, bin, o, d, tmin, tmax, n, occ != nullptr, msg, sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  if (n == 0) return VQN_OK;
  return vqn_launch(__func__, rays_occluded_kernel, rays_launch_grid(n), kThreads, 0, stream,
                    rays_scene(packed, n_tris, grid, cell_offset, n_pairs, bin), o, d, tmin, tmax, (long)n, occ);
}

extern "C" int vqn_rays_light_visibility(const float* packed, int64_t n_tris, const struct VqnGeomGrid* grid, const int32_t* cell_offset,
                                         int64_t n_pairs, const int32_t* bin, const float* points, const float* normals, int64_t n,
                                         const float* lights, int n_lights, float bias, int lanes, float* out, void* stream) {
  char msg[200];
  if (const int rc = rays_light_plan(packed, n_tris, grid, cell_offset, n_pairs, bin, points, normals, n, lights, n_lights, bias, lanes, out, msg,
                                     sizeof(msg))) {
    vqn_set_error("%s: %s", __func__, msg);
    return rc;
  }
  if (n == 0) return VQN_OK;
  const RaysScene sc = rays_scene(packed, n_tris, grid, cell_offset, n_pairs, bin);
  const dim3 g((unsigned)vqn_grid1((long)rays_light_units(n, n_lights, lanes), kPerCu));
  if (lanes == VQN_RAYS_LANES_POINTS)
    return vqn_launch(__func__, rays_light_points_kernel, g, kThreads, 0, stream, sc, points, normals, (long)n, lights, n_lights, bias, out);
  return vqn_launch(__func__, rays_light_lights_kernel, g, kThreads, 0, stream, sc, points, normals, (long)n, lights, n_lights, bias, out);
}
