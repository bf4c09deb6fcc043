// Geometry scores on the device: how far a predicted surface is from a reference one.  Accuracy / completeness / Chamfer, precision /
// recall / F-score at distance thresholds and normal consistency are sums over the exact nearest neighbour of every point of one
// surface among the points of the other (geo/geometry_eval.py; the NumPy statement is tests/geometry_eval_model.py, DESIGN section
// 14).  The reference ships no geometry evaluator; DTU's own is a k-d tree on the host.
//
//  * tri_areas_kernel, sample_surface_kernel: a triangle per thread (area in double), a sample per thread (binary search of the
//    caller's inclusive area prefix, the point a v0 + b v1 + c v2 and the unit face normal in double, each rounded once).
//  * cell_ids_kernel, pack_sorted_kernel: the cell of every point in a uniform grid (floor((p - origin) / h) per axis in f32,
//    clamped), and the reference points in cell order as 16-byte records (x, y, z, original index): a candidate is one vector load.
//  * nearest_kernel (the hot one): a query per thread.  Rings r = 0, 1, 2 ... of cells around the query's cell c: the shell of the
//    box of cells [c - r, c + r], clipped to the grid, walked row by row; cells that are neighbours along x are neighbours in the
//    record array, so a row of the shell is ONE run of records.  The best (d2, original index) is kept lexicographically, so the
//    traversal order cannot show.  After ring r the search stops when best d2 <= bound(r), a strict lower bound of the f32 d2 of
//    every point OUTSIDE the box:
//      a point outside the box has, on some axis, a cell index >= K = c + r + 1 (an upper face) or <= K - 1 with K = c - r (a lower
//      face).  Its cell index is floor(t), t = fl(fl(p - o) / h) = (p - o) / h (1 + e1)(1 + e2), |e| <= 2^-24 (the difference of two
//      floats has a RELATIVE error; clamping moves indices only towards the grid).  Hence p >= o + K h (1 - 2^-22) beyond an upper
//      face and p < o + K h (1 + 2^-22) beyond a lower one.  The kernel places the faces in double with the margin 2^-20 and takes off
//      2^-48 (|o| + |q| + K h) for its own three double roundings; gap = the least such distance over the faces that are inside the
//      grid (a face on or past the grid's boundary has no point behind it: +inf; a negative gap counts as 0).  The f32 d2 of a point
//      behind a face is >= fl(dx dx) with |dx| >= gap (1 - 2^-24), so >= gap^2 (1 - 2^-22) (sums of non-negative terms round
//      monotonically); bound = gap^2 (1 - 2^-18) is strictly below it, and 0 where gap^2 is small enough for a product to underflow.
//    Stopping late costs time, stopping early would change bits: every margin errs towards late.  The ring loop is bounded by a host
//    value (max(dims), fewer with a distance cap) and a row's record loop by n_ref, whatever cell_start holds.
//  * reduce_kernel, reduce_final_kernel: per-thread strided sums, a fixed LDS tree per workgroup, the workgroups' words added in
//    slot order by one workgroup.  No atomics: equal inputs give equal bits.
#include "common.h"
#include "geometry_eval_plan.h"
#include "vqn_geometry_eval.h"

// every product, sum and quotient below is rounded on its own, as the statement's are
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = VQN_GEOM_THREADS;
constexpr int kMaxThr = VQN_GEOM_MAX_THRESHOLDS;
constexpr int kOutWords = VQN_GEOM_OUT_WORDS;
constexpr int kReduceGridCap = VQN_GEOM_REDUCE_GRID_CAP;
constexpr int kWordN = 0, kWordValid = 1, kWordCount = 2, kWordSumD = 10, kWordSumD2 = 11, kWordMaxD = 12, kWordSumDot = 13, kWordPairs = 14;
static_assert(kWordCount + kMaxThr == kWordSumD && kWordPairs + 2 == kOutWords, "the layout of `out`");
constexpr double kFaceMargin = 0x1p-20, kOwnRounding = 0x1p-48, kD2Margin = 0x1p-18, kUnderflow = 1e-30;

struct Thresholds {
  double tau[kMaxThr];
  int n;
};

__device__ __forceinline__ bool tri_ok(const int32_t* __restrict__ tris, const int64_t t, const int64_t n_verts, int (&v)[3]) {
  v[0] = tris[3 * t], v[1] = tris[3 * t + 1], v[2] = tris[3 * t + 2];
  return (uint64_t)v[0] < (uint64_t)n_verts && (uint64_t)v[1] < (uint64_t)n_verts && (uint64_t)v[2] < (uint64_t)n_verts;
}

// (v1 - v0) x (v2 - v0) in double; the corners as doubles in p
__device__ __forceinline__ void tri_cross(const float* __restrict__ verts, const int (&v)[3], double (&p)[3][3], double (&c)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) p[k][a] = (double)verts[3 * (int64_t)v[k] + a];
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) e1[a] = p[1][a] - p[0][a], e2[a] = p[2][a] - p[0][a];
  c[0] = e1[1] * e2[2] - e1[2] * e2[1];
  c[1] = e1[2] * e2[0] - e1[0] * e2[2];
  c[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

__global__ __launch_bounds__(kThreads) void tri_areas_kernel(const float* __restrict__ verts, const int64_t n_verts,
                                                             const int32_t* __restrict__ tris, const int64_t n_tris,
                                                             double* __restrict__ areas) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= n_tris) return;
  int v[3];
  double p[3][3], c[3], area = 0.0;
  if (tri_ok(tris, t, n_verts, v)) {
    tri_cross(verts, v, p, c);
    area = 0.5 * sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  }
  areas[t] = area;
}

__global__ __launch_bounds__(kThreads) void sample_surface_kernel(const float* __restrict__ verts, const int64_t n_verts,
                                                                  const int32_t* __restrict__ tris, const int64_t n_tris,
                                                                  const double* __restrict__ cum, const float* __restrict__ u,
                                                                  const int64_t n, float* __restrict__ points,
                                                                  float* __restrict__ normals, int32_t* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double x = (double)u[3 * i] * cum[n_tris - 1];
  int64_t lo = 0, hi = n_tris - 1;                           // the first t with cum[t] > x (the last triangle for an x past the total)
  for (int it = 0; it < 32 && lo < hi; ++it) {               // n_tris < 2^31: 31 halvings at most
    const int64_t mid = (lo + hi) >> 1;
    if (cum[mid] > x)
      hi = mid;
    else
      lo = mid + 1;
  }
  int v[3];
  double p[3][3], c[3];
  float out_p[3] = {0.f, 0.f, 0.f}, out_n[3] = {0.f, 0.f, 0.f};
  if (tri_ok(tris, lo, n_verts, v)) {
    tri_cross(verts, v, p, c);
    const double s = sqrt((double)u[3 * i + 1]), u2 = (double)u[3 * i + 2];
    const double a = 1.0 - s, b = s * (1.0 - u2), w = s * u2;
    const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      out_p[k] = (float)((a * p[0][k] + b * p[1][k]) + w * p[2][k]);
      out_n[k] = len > 0.0 ? (float)(c[k] / len) : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) points[3 * i + k] = out_p[k], normals[3 * i + k] = out_n[k];
  face[i] = (int32_t)lo;
}

// floor((p - o) / h) in f32, clamped into [0, n - 1] (as a float first: the quotient of a far point does not fit an int; NaN -> 0)
__device__ __forceinline__ int cell_axis(const float p, const float o, const float h, const int n) {
  const float t = floorf((p - o) / h);
  return (int)fminf(fmaxf(t, 0.f), (float)(n - 1));
}

__global__ __launch_bounds__(kThreads) void cell_ids_kernel(const float* __restrict__ pts, const int64_t n, const VqnGeomGrid g,
                                                            int32_t* __restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int cx = cell_axis(pts[3 * i], g.origin[0], g.h, g.dims[0]);
  const int cy = cell_axis(pts[3 * i + 1], g.origin[1], g.h, g.dims[1]);
  const int cz = cell_axis(pts[3 * i + 2], g.origin[2], g.h, g.dims[2]);
  ids[i] = (cz * g.dims[1] + cy) * g.dims[0] + cx;
}

__global__ __launch_bounds__(kThreads) void pack_sorted_kernel(const float* __restrict__ pts, const int64_t n,
                                                               const int64_t* __restrict__ order, f32x4* __restrict__ packed) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const int64_t i = order[j];
  f32x4 r;
  if ((uint64_t)i < (uint64_t)n) {
    r = f32x4{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float((int)i)};
  } else {                                                   // not a permutation: a record that no query can choose (its d2 is NaN)
    const float nan = __int_as_float(0x7fc00000);
    r = f32x4{nan, nan, nan, __int_as_float(0x7fffffff)};
  }
  packed[j] = r;
}

struct Best {
  float d2;
  int idx;
};

constexpr int kBatch = 4;

// Plain operators under this file's contract(off): the __fmul_rn / __fadd_rn of the HIP headers are `x * y` and `x + y` compiled under
// the headers' own contraction setting, and fuse once they are inlined.
__device__ __forceinline__ void candidate(const f32x4 p, const float qx, const float qy, const float qz, Best& best) {
  const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float d2 = (xx + yy) + zz;
  const int id = __float_as_int(p.w);
  const bool better = d2 < best.d2 || (d2 == best.d2 && id < best.idx);
  best.d2 = better ? d2 : best.d2;
  best.idx = better ? id : best.idx;
}

// records [cell_start[c0], cell_start[c1 + 1]) against q; the loop cannot leave [0, n_ref) whatever cell_start holds
__device__ __forceinline__ void scan_cells(const f32x4* __restrict__ packed, const int32_t* __restrict__ cell_start, const int c0, const int c1,
                                           const int n_ref, const float qx, const float qy, const float qz, Best& best) {
  int a = cell_start[c0], b = cell_start[c1 + 1];
  a = a < 0 ? 0 : a;
  b = b > n_ref ? n_ref : (b < 0 ? 0 : b);
  int j = a;
  for (; j <= b - kBatch; j += kBatch) {                     // kBatch loads in flight, then kBatch updates without a branch
    f32x4 p[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) p[k] = packed[j + k];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) candidate(p[k], qx, qy, qz, best);
  }
  for (; j < b; ++j) candidate(packed[j], qx, qy, qz, best);
}

// the distance from q to the faces K_lo (lower) and K_hi (upper) of one axis that are inside the grid, each placed so that it is a
// lower bound of the distance to any point whose cell lies beyond it (see the head of the file); +inf for a face on the boundary
__device__ __forceinline__ double axis_gap(const double q, const double o, const double h, const int k_lo, const int k_hi, const int n) {
  double gap = __builtin_inf();
  if (k_lo >= 1) {
    const double kh = (double)k_lo * h, face = o + kh * (1.0 + kFaceMargin);
    gap = (q - face) - kOwnRounding * ((fabs(o) + fabs(q)) + kh);
  }
  if (k_hi <= n - 1) {
    const double kh = (double)k_hi * h, face = o + kh * (1.0 - kFaceMargin);
    const double g2 = (face - q) - kOwnRounding * ((fabs(o) + fabs(q)) + kh);
    gap = g2 < gap ? g2 : gap;
  }
  return gap;
}

__global__ __launch_bounds__(kThreads) void nearest_kernel(const float* __restrict__ query, const int64_t n_q, const int32_t* __restrict__ q_order,
                                                           const f32x4* __restrict__ packed, const int32_t* __restrict__ cell_start,
                                                           const int n_ref, const VqnGeomGrid g, const int max_rings, const float max_d2,
                                                           float* __restrict__ out_d2, int32_t* __restrict__ out_idx) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_q) return;
  const int64_t q = q_order ? (int64_t)q_order[i] : i;
  if ((uint64_t)q >= (uint64_t)n_q) return;
  const float qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
  const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  const int cx = cell_axis(qx, g.origin[0], g.h, nx), cy = cell_axis(qy, g.origin[1], g.h, ny), cz = cell_axis(qz, g.origin[2], g.h, nz);
  const double h = (double)g.h;
  Best best = {__builtin_inff(), 0x7fffffff};
  for (int r = 0; r < max_rings; ++r) {
    const int x0 = cx - r < 0 ? 0 : cx - r, x1 = cx + r > nx - 1 ? nx - 1 : cx + r;
    const int y0 = cy - r < 0 ? 0 : cy - r, y1 = cy + r > ny - 1 ? ny - 1 : cy + r;
    const int z0 = cz - r < 0 ? 0 : cz - r, z1 = cz + r > nz - 1 ? nz - 1 : cz + r;
    for (int z = z0; z <= z1; ++z) {
      const bool z_shell = z == cz - r || z == cz + r;
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * ny + y) * nx;
        if (z_shell || y == cy - r || y == cy + r) {         // a row of the shell's z or y faces: one run of records
          scan_cells(packed, cell_start, row + x0, row + x1, n_ref, qx, qy, qz, best);
        } else {                                             // an inner row: the two cells of the x faces (r >= 1 here)
          if (cx - r >= 0) scan_cells(packed, cell_start, row + cx - r, row + cx - r, n_ref, qx, qy, qz, best);
          if (cx + r <= nx - 1) scan_cells(packed, cell_start, row + cx + r, row + cx + r, n_ref, qx, qy, qz, best);
        }
      }
    }
    double gap = axis_gap((double)qx, (double)g.origin[0], h, cx - r, cx + r + 1, nx);
    const double gy = axis_gap((double)qy, (double)g.origin[1], h, cy - r, cy + r + 1, ny);
    const double gz = axis_gap((double)qz, (double)g.origin[2], h, cz - r, cz + r + 1, nz);
    gap = gy < gap ? gy : gap;
    gap = gz < gap ? gz : gap;
    double bound = 0.0;                                      // (also for a NaN gap: never an early stop)
    if (gap > 0.0) {
      bound = (gap * gap) * (1.0 - kD2Margin);
      if (bound < kUnderflow) bound = 0.0;
    }
    if ((double)best.d2 <= bound || bound > (double)max_d2) break;
  }
  const bool found = best.idx != 0x7fffffff && best.d2 <= max_d2;
  out_d2[q] = found ? best.d2 : __builtin_inff();
  out_idx[q] = found ? best.idx : -1;
}

// ---- directed reduction ----
struct Sums {
  int64_t valid, count[kMaxThr], pairs;
  double sum_d, sum_d2, max_d, sum_dot;
};

__device__ __forceinline__ void add(Sums& a, const Sums& b) {
  a.valid += b.valid;
#pragma unroll
  for (int k = 0; k < kMaxThr; ++k) a.count[k] += b.count[k];
  a.pairs += b.pairs;
  a.sum_d = a.sum_d + b.sum_d;
  a.sum_d2 = a.sum_d2 + b.sum_d2;
  a.max_d = b.max_d > a.max_d ? b.max_d : a.max_d;
  a.sum_dot = a.sum_dot + b.sum_dot;
}

__device__ __forceinline__ Sums zero_sums() {
  Sums s;
  s.valid = s.pairs = 0;
#pragma unroll
  for (int k = 0; k < kMaxThr; ++k) s.count[k] = 0;
  s.sum_d = s.sum_d2 = s.max_d = s.sum_dot = 0.0;
  return s;
}

// the workgroup's sum in thread 0: a tree with a fixed shape (thread t takes t + 128, then t + 64 ...)
__device__ __forceinline__ void block_sum(Sums& s, Sums* __restrict__ lds) {
  const int tid = threadIdx.x;
  lds[tid] = s;
  __syncthreads();
  for (int step = kThreads / 2; step >= 1; step >>= 1) {
    if (tid < step) {
      add(s, lds[tid + step]);
      lds[tid] = s;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void store_words(const Sums& s, int64_t* __restrict__ w) {
  w[kWordValid] = s.valid;
#pragma unroll
  for (int k = 0; k < kMaxThr; ++k) w[kWordCount + k] = s.count[k];
  w[kWordSumD] = __double_as_longlong(s.sum_d);
  w[kWordSumD2] = __double_as_longlong(s.sum_d2);
  w[kWordMaxD] = __double_as_longlong(s.max_d);
  w[kWordSumDot] = __double_as_longlong(s.sum_dot);
  w[kWordPairs] = s.pairs;
  w[kWordN] = 0, w[kOutWords - 1] = 0;
}

__device__ __forceinline__ Sums load_words(const int64_t* __restrict__ w) {
  Sums s;
  s.valid = w[kWordValid];
#pragma unroll
  for (int k = 0; k < kMaxThr; ++k) s.count[k] = w[kWordCount + k];
  s.sum_d = __longlong_as_double(w[kWordSumD]);
  s.sum_d2 = __longlong_as_double(w[kWordSumD2]);
  s.max_d = __longlong_as_double(w[kWordMaxD]);
  s.sum_dot = __longlong_as_double(w[kWordSumDot]);
  s.pairs = w[kWordPairs];
  return s;
}

__global__ __launch_bounds__(kThreads) void reduce_kernel(const float* __restrict__ d2, const int32_t* __restrict__ idx, const int64_t n,
                                                          const float* __restrict__ qn, const float* __restrict__ rn, const int64_t n_ref,
                                                          const Thresholds thr, int64_t* __restrict__ slots) {
  __shared__ Sums lds[kThreads];
  Sums s = zero_sums();
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t id = idx[i];
    if (id < 0 || id >= n_ref) continue;
    const double dd = (double)d2[i], d = sqrt(dd);
    s.valid += 1;
#pragma unroll
    for (int k = 0; k < kMaxThr; ++k) s.count[k] += (k < thr.n && d < thr.tau[k]) ? 1 : 0;
    s.sum_d = s.sum_d + d;
    s.sum_d2 = s.sum_d2 + dd;
    s.max_d = d > s.max_d ? d : s.max_d;
    if (qn && rn) {
      const float a0 = qn[3 * i], a1 = qn[3 * i + 1], a2 = qn[3 * i + 2];
      const float b0 = rn[3 * id], b1 = rn[3 * id + 1], b2 = rn[3 * id + 2];
      const bool a_nz = a0 != 0.f || a1 != 0.f || a2 != 0.f, b_nz = b0 != 0.f || b1 != 0.f || b2 != 0.f;
      if (a_nz && b_nz) {
        const double dot = ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
        s.sum_dot = s.sum_dot + fabs(dot);
        s.pairs += 1;
      }
    }
  }
  block_sum(s, lds);
  if (threadIdx.x == 0) store_words(s, slots + (int64_t)blockIdx.x * kOutWords);
}

__global__ __launch_bounds__(kThreads) void reduce_final_kernel(const int64_t* __restrict__ slots, const int n_slots, const int64_t n,
                                                                int64_t* __restrict__ out) {
  __shared__ Sums lds[kThreads];
  Sums s = zero_sums();
  for (int j = threadIdx.x; j < n_slots; j += kThreads) add(s, load_words(slots + (int64_t)j * kOutWords));
  block_sum(s, lds);
  if (threadIdx.x == 0) {
    store_words(s, out);
    out[kWordN] = n;
  }
}

unsigned blocks_of(const int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

bool count_ok(const char* fn, const char* what, const int64_t n) {
  if (n < 1 || n >= ((int64_t)1 << 31)) {
    vqn_set_error("%s: unsupported shape: 1 <= %s < 2^31, got %lld", fn, what, (long long)n);
    return false;
  }
  return true;
}

int64_t reduce_blocks(const int64_t n) {
  const int64_t b = (n + kThreads - 1) / kThreads;
  return b < kReduceGridCap ? b : kReduceGridCap;
}

}  // namespace

extern "C" int vqn_geom_tri_areas(const float* vertices, int64_t n_verts, const int32_t* triangles, int64_t n_tris, double* areas,
                                  void* stream) {
  if (!count_ok(__func__, "vertices", n_verts) || !count_ok(__func__, "triangles", n_tris)) return VQN_ESHAPE;
  VQN_CHECK_ARG(vertices && triangles && areas, "null pointer");
  hipLaunchKernelGGL(tri_areas_kernel, dim3(blocks_of(n_tris)), dim3(kThreads), 0, (hipStream_t)stream, vertices, n_verts, triangles, n_tris,
                     areas);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_geom_sample_surface(const float* vertices, int64_t n_verts, const int32_t* triangles, int64_t n_tris, const double* cum,
                                       const float* u, int64_t n, float* points, float* normals, int32_t* face, void* stream) {
  if (!count_ok(__func__, "vertices", n_verts) || !count_ok(__func__, "triangles", n_tris)) return VQN_ESHAPE;
  if (n == 0) return VQN_OK;
  if (!count_ok(__func__, "samples", n)) return VQN_ESHAPE;
  VQN_CHECK_ARG(vertices && triangles && cum && u && points && normals && face, "null pointer");
  hipLaunchKernelGGL(sample_surface_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, (hipStream_t)stream, vertices, n_verts, triangles, n_tris,
                     cum, u, n, points, normals, face);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_geom_grid_plan(const float* lo, const float* hi, int64_t n, float cell, struct VqnGeomGrid* grid) {
  const char* why = "";
  const int rc = vqn_geom_plan_grid(lo, hi, n, cell, grid, &why);
  if (rc != 0) vqn_set_error("%s: %s: %s", __func__, rc == VQN_ESHAPE ? "unsupported shape" : "bad argument", why);
  return rc;
}

extern "C" int vqn_geom_cell_ids(const float* points, int64_t n, const struct VqnGeomGrid* grid, int32_t* ids, void* stream) {
  if (n == 0) return VQN_OK;
  if (!count_ok(__func__, "points", n)) return VQN_ESHAPE;
  VQN_CHECK_ARG(points && grid && ids, "null pointer");
  VQN_CHECK_SHAPE(vqn_geom_grid_ok(grid), "a grid of h > 0, 1 .. 1024 cells per axis, at most 2^24 cells, cells = their product");
  hipLaunchKernelGGL(cell_ids_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, (hipStream_t)stream, points, n, *grid, ids);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_geom_pack_sorted(const float* points, int64_t n, const int64_t* order, void* packed, void* stream) {
  if (!count_ok(__func__, "points", n)) return VQN_ESHAPE;
  VQN_CHECK_ARG(points && order && packed, "null pointer");
  VQN_CHECK_ARG(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
  hipLaunchKernelGGL(pack_sorted_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, (hipStream_t)stream, points, n, order, (f32x4*)packed);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_geom_nearest(const float* query, int64_t n_q, const int32_t* q_order, const void* packed, const int32_t* cell_start,
                                int64_t n_ref, const struct VqnGeomGrid* grid, float max_d2, float* d2, int32_t* idx, void* stream) {
  if (!count_ok(__func__, "reference points", n_ref)) return VQN_ESHAPE;
  if (n_q == 0) return VQN_OK;
  if (!count_ok(__func__, "queries", n_q)) return VQN_ESHAPE;
  VQN_CHECK_ARG(query && packed && cell_start && grid && d2 && idx, "null pointer");
  VQN_CHECK_ARG(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
  VQN_CHECK_ARG(max_d2 >= 0.0f, "max_d2 >= 0 (+inf for none)");
  VQN_CHECK_SHAPE(vqn_geom_grid_ok(grid), "a grid of h > 0, 1 .. 1024 cells per axis, at most 2^24 cells, cells = their product");
  int rings = grid->dims[0] > grid->dims[1] ? grid->dims[0] : grid->dims[1];
  rings = rings > grid->dims[2] ? rings : grid->dims[2];
  // with a cap, ring r's bound is about (r h)^2: past sqrt(max_d2) / h + 1 rings it exceeds the cap
  const double capped = ceil(sqrt((double)max_d2) / (double)grid->h) + 2.0;
  if (capped < (double)rings) rings = (int)capped;
  hipLaunchKernelGGL(nearest_kernel, dim3(blocks_of(n_q)), dim3(kThreads), 0, (hipStream_t)stream, query, n_q, q_order, (const f32x4*)packed,
                     cell_start, (int)n_ref, *grid, rings, max_d2, d2, idx);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int64_t vqn_geom_reduce_scratch_bytes(int64_t n) {
  if (n < 1 || n >= ((int64_t)1 << 31)) return 0;
  return reduce_blocks(n) * kOutWords * 8;
}

extern "C" int vqn_geom_reduce(const float* d2, const int32_t* idx, int64_t n, const float* q_normals, const float* ref_normals, int64_t n_ref,
                               const double* thresholds, int n_thresholds, void* scratch, int64_t scratch_bytes, void* out, void* stream) {
  if (!count_ok(__func__, "queries", n) || !count_ok(__func__, "reference points", n_ref)) return VQN_ESHAPE;
  VQN_CHECK_SHAPE(n_thresholds >= 0 && n_thresholds <= kMaxThr, "0 .. 8 thresholds");
  const int64_t need = vqn_geom_reduce_scratch_bytes(n);
  VQN_CHECK_ARG(d2 && idx && out && scratch && (thresholds || n_thresholds == 0), "null pointer");
  VQN_CHECK_ARG(scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0, "scratch smaller than vqn_geom_reduce_scratch_bytes, or not 8-byte aligned");
  Thresholds thr;
  thr.n = n_thresholds;
  for (int k = 0; k < kMaxThr; ++k) thr.tau[k] = k < n_thresholds ? thresholds[k] : 0.0;
  const int blocks = (int)reduce_blocks(n);
  hipLaunchKernelGGL(reduce_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, d2, idx, n, q_normals, ref_normals, n_ref, thr,
                     (int64_t*)scratch);
  VQN_LAUNCH_CHECK();
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)scratch, blocks, n, (int64_t*)out);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}
