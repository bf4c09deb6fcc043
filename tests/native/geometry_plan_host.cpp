// AddressSanitizer / UBSan check of the host-only C++ of the geometry scores (csrc/geometry_eval_plan.h): the grid planner over point
// counts 1 .. 2^30 and boxes with zero extent on none, one, two or three axes -- the caps hold, the cell size is a positive finite
// float, the grid covers the box -- an override honoured or refused, and every refusal with its code.  Built and run by
// tests/test_geometry_eval_io.py:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ivqnerf_release_amd/csrc
//       tests/native/geometry_plan_host.cpp
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "geometry_eval_plan.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s\n", what);
    ++failures;
  }
}

static bool grid_holds(const VqnGeomGrid& g, const float* lo, const float* hi) {
  bool ok = g.h > 0.0f && isfinite(g.h) && vqn_geom_grid_ok(&g);
  for (int a = 0; a < 3; ++a) {
    ok = ok && g.origin[a] == lo[a] && g.dims[a] >= 1 && g.dims[a] <= VQN_GEOM_MAX_AXIS;
    ok = ok && (double)g.dims[a] == floor(((double)hi[a] - (double)lo[a]) / (double)g.h) + 1.0;     // the far corner has a cell
  }
  return ok && (int64_t)g.dims[0] * g.dims[1] * g.dims[2] == g.cells && g.cells <= VQN_GEOM_MAX_CELLS;
}

int main() {
  const float extents[][3] = {{1.f, 1.f, 1.f},   {2.f, 0.5f, 3.f}, {1e-3f, 1e3f, 1.f}, {0.f, 1.f, 1.f}, {1.f, 0.f, 2.f}, {1.f, 1.f, 0.f},
                              {0.f, 0.f, 1.f},   {0.f, 5.f, 0.f},  {7.f, 0.f, 0.f},    {0.f, 0.f, 0.f}, {1e30f, 1e30f, 1e30f},
                              {1e-30f, 0.f, 0.f}, {3e38f, 1.f, 0.f}};
  const float origins[] = {0.f, -1.5f, 1000.f};
  int plans = 0;
  const char* why = "";
  for (const auto& e : extents)
    for (const float o : origins) {
      const float lo[3] = {o, o, o}, hi[3] = {o + e[0], o + e[1], o + e[2]};
      if (!isfinite(hi[0])) continue;
      for (int64_t n = 1; n <= ((int64_t)1 << 30); n = n < 16 ? n + 1 : n * 2 - 3) {
        VqnGeomGrid g;
        const int rc = vqn_geom_plan_grid(lo, hi, n, 0.0f, &g, &why);
        expect(rc == 0 && grid_holds(g, lo, hi), "default plan");
        ++plans;
      }
    }
  // the default of a unit cube of 10^6 points: h = sqrt(8 * 6 / 10^6), about 8 points per cell of the surface
  const float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {1.f, 1.f, 1.f};
  VqnGeomGrid g;
  expect(vqn_geom_plan_grid(lo, hi, 1000000, 0.0f, &g, &why) == 0 && g.h == (float)sqrt(48.0 / 1e6) && g.dims[0] == 145 && g.cells == 145 * 145 * 145,
         "default cell size");
  // overrides: honoured, or refused with -2
  expect(vqn_geom_plan_grid(lo, hi, 10, 0.25f, &g, &why) == 0 && g.h == 0.25f && g.dims[0] == 5 && g.dims[2] == 5 && g.cells == 125, "override");
  expect(vqn_geom_plan_grid(lo, hi, 10, 100.0f, &g, &why) == 0 && g.cells == 1, "one cell");
  expect(vqn_geom_plan_grid(lo, hi, 10, 1.0f / 1023.5f, &g, &why) == -2, "an override over 1024 cells per axis");
  expect(vqn_geom_plan_grid(lo, hi, 10, 1.0f / 300.0f, &g, &why) == -2, "an override over 2^24 cells");
  expect(vqn_geom_plan_grid(lo, hi, 10, INFINITY, &g, &why) == -2, "an infinite override");
  expect(vqn_geom_plan_grid(lo, hi, 0, 0.0f, &g, &why) == -2 && vqn_geom_plan_grid(lo, hi, (int64_t)1 << 31, 0.0f, &g, &why) == -2, "point counts");
  expect(vqn_geom_plan_grid(nullptr, hi, 10, 0.0f, &g, &why) == -1 && vqn_geom_plan_grid(lo, hi, 10, 0.0f, nullptr, &why) == -1, "null pointers");
  expect(vqn_geom_plan_grid(hi, lo, 10, 0.0f, &g, &why) == -1, "lo > hi");
  const float bad[3] = {0.f, NAN, 0.f};
  expect(vqn_geom_plan_grid(bad, hi, 10, 0.0f, &g, &why) == -1, "a NaN corner");
  g.cells += 1;
  expect(!vqn_geom_grid_ok(&g), "a grid whose cells are not the product of its dims");
  if (failures) return 1;
  printf("geometry plan ok: %d default plans\n", plans);
  return 0;
}
