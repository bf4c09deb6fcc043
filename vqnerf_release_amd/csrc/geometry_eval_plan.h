// The grid planner of the geometry scores (host only, plain C++: csrc/geometry_eval.hip wraps it as vqn_geom_grid_plan, and
// tests/native/geometry_plan_host.cpp builds it without HIP).  Not a public header.
#pragma once
#include <math.h>
#include <stdint.h>

#include "vqn_geometry_eval.h"

// dims of a box of extents ext[3] at cell size h; false when they exceed the caps
static inline bool vqn_geom_dims(const double ext[3], const double h, int32_t dims[3]) {
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    const double d = floor(ext[a] / h) + 1.0;
    if (!(d <= (double)VQN_GEOM_MAX_AXIS)) return false;      // (also a NaN quotient)
    dims[a] = (int32_t)d;
    cells *= dims[a];
  }
  return cells <= VQN_GEOM_MAX_CELLS;
}

// 0, or -1 (null pointer, a box that is not finite or has lo > hi), or -2 (n outside [1, 2^31), an override over the caps); *why
// names the reason
static inline int vqn_geom_plan_grid(const float* lo, const float* hi, const int64_t n, const float cell, VqnGeomGrid* grid,
                                     const char** why) {
  if (!lo || !hi || !grid) return *why = "null pointer", -1;
  if (n < 1 || n >= ((int64_t)1 << 31)) return *why = "1 <= n < 2^31 reference points", -2;
  double ext[3];
  for (int a = 0; a < 3; ++a) {
    if (!isfinite(lo[a]) || !isfinite(hi[a]) || lo[a] > hi[a]) return *why = "the bounding box must be finite with lo <= hi", -1;
    ext[a] = (double)hi[a] - (double)lo[a];
  }
  int32_t dims[3];
  float h;
  if (cell > 0.0f) {
    if (!isfinite(cell) || !vqn_geom_dims(ext, (double)cell, dims))
      return *why = "the cell size is not finite or needs more than 1024 cells per axis or 2^24 cells", -2;
    h = cell;
  } else {
    const double S = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]);
    const double L = fmax(ext[0], fmax(ext[1], ext[2]));
    double hd = S > 0.0 ? sqrt(8.0 * S / (double)n) : (L > 0.0 ? 8.0 * L / (double)n : 1.0);
    hd = fmax(hd, L / (VQN_GEOM_MAX_AXIS - 1));                // at most 1024 cells per axis (rounding: the loop below)
    hd = fmax(hd, 1e-30);                                      // (a normal float)
    h = (float)hd;
    bool ok = false;
    for (int it = 0; it < 64 && isfinite(h); ++it) {           // raise h until the caps hold: a few steps (cells shrink by 1.25^3)
      if ((ok = vqn_geom_dims(ext, (double)h, dims))) break;
      h *= 1.25f;
    }
    if (!ok) return *why = "no float cell size fits the bounding box", -1;
  }
  for (int a = 0; a < 3; ++a) grid->origin[a] = lo[a], grid->dims[a] = dims[a];
  grid->h = h;
  grid->cells = dims[0] * dims[1] * dims[2];
  return 0;
}

// what the device calls require of a grid they are handed
static inline bool vqn_geom_grid_ok(const VqnGeomGrid* g) {
  if (!(g->h > 0.0f) || !isfinite(g->h)) return false;
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (!isfinite(g->origin[a]) || g->dims[a] < 1 || g->dims[a] > VQN_GEOM_MAX_AXIS) return false;
    cells *= g->dims[a];
  }
  return cells <= VQN_GEOM_MAX_CELLS && cells == g->cells;
}
