// Host side of the mesh ray caster (csrc/mesh_rays.hip): the grid rule, the limits, the sizes of every array and of the launches,
// with every refusal.  Plain C++, no HIP: tests/native/mesh_rays_host.cpp builds it into a stand-alone program under ASan / UBSan.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vqn_mesh_rays.h"  // (by path: the stand-alone build of this header names no include directory)

constexpr int kRaysMaxAxis = VQN_RAYS_MAX_AXIS;
constexpr int64_t kRaysMaxCells = VQN_RAYS_MAX_CELLS;
constexpr int kRaysStats = VQN_RAYS_STATS;
constexpr float kRaysMargin = 1.0f / VQN_RAYS_MARGIN_INV;      // in cells: the widening of a triangle's box, and the walk's slack
constexpr int kRaysPackedFloats = VQN_RAYS_PACKED_FLOATS;
constexpr int kRaysMaxLights = VQN_RAYS_MAX_LIGHTS;
constexpr int kRaysTile = VQN_RAYS_TILE;
constexpr int kRaysThreads = 256;
constexpr int64_t kRaysIndexLimit = (int64_t)1 << 31;          // every index and every flat offset of a list is an int32
constexpr int64_t kRaysPairLimit = (int64_t)1 << 40;           // n * n_lights below this
// the staged tile of the visibility kernel: kRaysTile lights x (kRaysTile + 1) points, one 4-byte word each
constexpr int kRaysLdsBytes = kRaysTile * (kRaysTile + 1) * 4;
static_assert(kRaysMaxCells * 4 <= 64ll << 20, "the cell table stays within 64 MB");
static_assert(kRaysTile == 64 && kRaysThreads % kRaysTile == 0, "a wave holds one row or one column of the tile");
static_assert(kRaysLdsBytes <= 64 * 1024, "the staged tile fits the LDS a kernel gets unasked");
static_assert(kRaysPackedFloats % 4 == 0, "a packed triangle is whole 16-byte reads");

#define RAYS_REFUSE(code, ...)           \
  do {                                   \
    snprintf(msg, msg_len, __VA_ARGS__); \
    return code;                         \
  } while (0)

// dims of a box of extents ext[3] at cell size h: floor(ext / h) + 2; false when they exceed the caps (or h is no number)
inline bool rays_dims(const double ext[3], const double h, int32_t dims[3]) {
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    const double d = floor(ext[a] / h) + 2.0;
    if (!(d <= (double)kRaysMaxAxis)) return false;            // (also a NaN quotient)
    dims[a] = (int32_t)d;
    cells *= dims[a];
  }
  return cells <= kRaysMaxCells;
}

// vqn_rays_grid_plan
inline int rays_grid_plan(const float* lo, const float* hi, const int64_t T, const float cell, VqnGeomGrid* grid, char* msg, size_t msg_len) {
  if (!lo || !hi || !grid) RAYS_REFUSE(-1, "bad argument: null pointer: lo, hi or grid");
  if (T < 0) RAYS_REFUSE(-1, "bad argument: negative size: n_tris = %lld", (long long)T);
  if (T >= (kRaysIndexLimit + 2) / 3) RAYS_REFUSE(-2, "unsupported shape: 3 n_tris must be < 2^31, n_tris = %lld", (long long)T);
  double ext[3];
  for (int a = 0; a < 3; ++a) {
    if (!isfinite(lo[a]) || !isfinite(hi[a]) || lo[a] > hi[a]) RAYS_REFUSE(-1, "bad argument: the bounding box must be finite with lo <= hi");
    ext[a] = (double)hi[a] - (double)lo[a];
    if (!isfinite((float)ext[a])) RAYS_REFUSE(-1, "bad argument: the bounding box must be finite with lo <= hi");
  }
  int32_t dims[3];
  float h;
  if (cell > 0.0f) {
    if (!isfinite(cell) || !rays_dims(ext, (double)cell, dims))
      RAYS_REFUSE(-2, "unsupported shape: the cell size %g is not finite or needs more than %d cells per axis or 2^24 cells", (double)cell,
                  kRaysMaxAxis);
    h = cell;
  } else {
    const double n = (double)(T > 0 ? T : 1);
    const double S = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]);
    const double L = fmax(ext[0], fmax(ext[1], ext[2]));
    double hd = S > 0.0 ? sqrt(2.0 * S / n) : (L > 0.0 ? 2.0 * L / n : 1.0);
    hd = fmax(hd, L / (kRaysMaxAxis - 2));                     // at most 1024 cells per axis (rounding: the loop below)
    hd = fmax(hd, 1e-30);                                      // (a normal float)
    h = (float)hd;
    bool ok = false;
    for (int it = 0; it < 64 && isfinite(h); ++it) {           // raise h until the caps hold: a few steps
      if ((ok = rays_dims(ext, (double)h, dims))) break;
      h *= 1.25f;
    }
    if (!ok) RAYS_REFUSE(-1, "bad argument: no float cell size fits the bounding box");
  }
  const float half = h / 2.0f;
  for (int a = 0; a < 3; ++a) {
    grid->origin[a] = lo[a] - half, grid->dims[a] = dims[a];
    if (!isfinite(grid->origin[a])) RAYS_REFUSE(-1, "bad argument: the bounding box must be finite with lo <= hi");
  }
  grid->h = h;
  grid->cells = dims[0] * dims[1] * dims[2];
  return 0;
}

// what the device calls require of a grid they are handed -> 0, -1 (not a grid) or -2 (over the caps)
inline int rays_grid_check(const VqnGeomGrid* g, char* msg, size_t msg_len) {
  if (!g) RAYS_REFUSE(-1, "bad argument: null pointer: grid");
  if (!(g->h > 0.0f) || !isfinite(g->h)) RAYS_REFUSE(-1, "bad argument: the grid's cell size must be positive and finite");
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (!isfinite(g->origin[a]) || g->dims[a] < 1) RAYS_REFUSE(-1, "bad argument: the grid's origin must be finite and its dims >= 1");
    if (g->dims[a] > kRaysMaxAxis) RAYS_REFUSE(-2, "unsupported shape: the grid has more than %d cells on an axis", kRaysMaxAxis);
    cells *= g->dims[a];
  }
  if (cells > kRaysMaxCells) RAYS_REFUSE(-2, "unsupported shape: the grid has more than 2^24 cells");
  if (cells != g->cells) RAYS_REFUSE(-1, "bad argument: the grid's cells = %d is not the product of its dims", g->cells);
  return 0;
}

// the mesh sizes every entry point takes
inline int rays_mesh_check(const int64_t T, const int64_t V, char* msg, size_t msg_len) {
  if (T < 0 || V < 0) RAYS_REFUSE(-1, "bad argument: negative size: n_tris = %lld, n_verts = %lld", (long long)T, (long long)V);
  if (V >= kRaysIndexLimit) RAYS_REFUSE(-2, "unsupported shape: n_verts = %lld must be < 2^31", (long long)V);
  if (T >= (kRaysIndexLimit + 2) / 3) RAYS_REFUSE(-2, "unsupported shape: 3 n_tris must be < 2^31, n_tris = %lld", (long long)T);
  return 0;
}

inline int rays_pairs_check(const int64_t n_pairs, const int64_t T, const VqnGeomGrid* g, char* msg, size_t msg_len) {
  if (n_pairs < 0) RAYS_REFUSE(-1, "bad argument: negative size: n_pairs = %lld", (long long)n_pairs);
  if (n_pairs >= kRaysIndexLimit) RAYS_REFUSE(-2, "unsupported shape: n_pairs = %lld must be < 2^31", (long long)n_pairs);
  if (n_pairs > T * (int64_t)g->cells)                         // (< 2^30 * 2^24)
    RAYS_REFUSE(-1, "bad argument: n_pairs = %lld contradicts the sizes: %lld triangles in %d cells", (long long)n_pairs, (long long)T, g->cells);
  return 0;
}

// vqn_rays_count
inline int rays_count_plan(const void* verts, int64_t V, const void* tris, int64_t T, const VqnGeomGrid* g, const void* cell_count, const void* stats,
                           char* msg, size_t msg_len) {
  if (const int rc = rays_mesh_check(T, V, msg, msg_len)) return rc;
  if (!cell_count || !stats) RAYS_REFUSE(-1, "bad argument: null pointer: cell_count or stats");
  if (!verts && V > 0) RAYS_REFUSE(-1, "bad argument: null pointer: verts");
  if (!tris && T > 0) RAYS_REFUSE(-1, "bad argument: null pointer: tris");
  return rays_grid_check(g, msg, msg_len);
}

// vqn_rays_bin
inline int rays_bin_plan(const void* verts, int64_t V, const void* tris, int64_t T, const VqnGeomGrid* g, const void* cell_offset, int64_t n_pairs,
                         const void* cursor, const void* bin, const void* packed, char* msg, size_t msg_len) {
  if (const int rc = rays_mesh_check(T, V, msg, msg_len)) return rc;
  if (!cell_offset || !cursor) RAYS_REFUSE(-1, "bad argument: null pointer: cell_offset or cursor");
  if (!verts && V > 0) RAYS_REFUSE(-1, "bad argument: null pointer: verts");
  if ((!tris || !packed) && T > 0) RAYS_REFUSE(-1, "bad argument: null pointer: tris or packed");
  if (((uintptr_t)packed & 15) != 0) RAYS_REFUSE(-1, "bad argument: packed must be 16-byte aligned");
  if (const int rc = rays_grid_check(g, msg, msg_len)) return rc;
  if (const int rc = rays_pairs_check(n_pairs, T, g, msg, msg_len)) return rc;
  if (!bin && n_pairs > 0) RAYS_REFUSE(-1, "bad argument: null pointer: bin");
  return 0;
}

// what every query takes: the built grid, then n rows
inline int rays_query_plan(const void* packed, int64_t T, const VqnGeomGrid* g, const void* cell_offset, int64_t n_pairs, const void* bin, int64_t n,
                           char* msg, size_t msg_len) {
  if (const int rc = rays_mesh_check(T, 0, msg, msg_len)) return rc;
  if (n < 0) RAYS_REFUSE(-1, "bad argument: negative size: n = %lld", (long long)n);
  if (!cell_offset) RAYS_REFUSE(-1, "bad argument: null pointer: cell_offset");
  if (!packed && T > 0) RAYS_REFUSE(-1, "bad argument: null pointer: packed");
  if (((uintptr_t)packed & 15) != 0) RAYS_REFUSE(-1, "bad argument: packed must be 16-byte aligned");
  if (const int rc = rays_grid_check(g, msg, msg_len)) return rc;
  if (const int rc = rays_pairs_check(n_pairs, T, g, msg, msg_len)) return rc;
  if (!bin && n_pairs > 0) RAYS_REFUSE(-1, "bad argument: null pointer: bin");
  return 0;
}

// vqn_rays_cast / vqn_rays_occluded: `outs` = whether every output pointer is there
inline int rays_cast_plan(const void* packed, int64_t T, const VqnGeomGrid* g, const void* cell_offset, int64_t n_pairs, const void* bin, const void* o,
                          const void* d, const void* tmin, const void* tmax, int64_t n, bool outs, char* msg, size_t msg_len) {
  if (const int rc = rays_query_plan(packed, T, g, cell_offset, n_pairs, bin, n, msg, msg_len)) return rc;
  if (n >= kRaysIndexLimit) RAYS_REFUSE(-2, "unsupported shape: n = %lld rays must be < 2^31", (long long)n);
  if (n > 0 && (!o || !d || !tmin || !tmax || !outs)) RAYS_REFUSE(-1, "bad argument: null pointer: o, d, tmin, tmax or an output");
  return 0;
}

// vqn_rays_light_visibility
inline int rays_light_plan(const void* packed, int64_t T, const VqnGeomGrid* g, const void* cell_offset, int64_t n_pairs, const void* bin,
                           const void* points, const void* normals, int64_t n, const void* lights, int L, float bias, int lanes, const void* out,
                           char* msg, size_t msg_len) {
  if (const int rc = rays_query_plan(packed, T, g, cell_offset, n_pairs, bin, n, msg, msg_len)) return rc;
  if (!isfinite(bias)) RAYS_REFUSE(-1, "bad argument: bias must be finite, got %g", (double)bias);
  if (lanes != VQN_RAYS_LANES_POINTS && lanes != VQN_RAYS_LANES_LIGHTS) RAYS_REFUSE(-1, "bad argument: lanes must be 0 or 1, got %d", lanes);
  if (L < 1 || L > kRaysMaxLights) RAYS_REFUSE(-2, "unsupported shape: 1 .. %d lights, got %d", kRaysMaxLights, L);
  if (n >= kRaysIndexLimit || n * (int64_t)L >= kRaysPairLimit)
    RAYS_REFUSE(-2, "unsupported shape: n = %lld points x %d lights must be < 2^40 with n < 2^31", (long long)n, L);
  if (!lights) RAYS_REFUSE(-1, "bad argument: null pointer: lights");
  if (n > 0 && (!points || !normals || !out)) RAYS_REFUSE(-1, "bad argument: null pointer: points, normals or out");
  return 0;
}

// workgroups of the visibility launch: one 64-point tile each (lanes = points), or 4 (point, 64-light chunk) waves each
inline int64_t rays_light_units(const int64_t n, const int L, const int lanes) {
  if (lanes == VQN_RAYS_LANES_POINTS) return (n + kRaysTile - 1) / kRaysTile;
  const int64_t chunks = (L + kRaysTile - 1) / kRaysTile;
  return (n * chunks + kRaysThreads / 64 - 1) / (kRaysThreads / 64);
}
