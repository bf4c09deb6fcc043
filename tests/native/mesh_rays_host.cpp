// Stand-alone check of the host side of the mesh ray caster (csrc/mesh_rays_plan.h) under ASan / UBSan: the limits, the grid rule over
// a sweep of boxes, triangle counts and cell sizes, the sizes of the launches, and every refusal of the entry points with its reason.
// Run by tests/test_mesh_rays_native.py.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mesh_rays_plan.h"

static int failures = 0;
static void check(bool ok, const char* file, int line, const char* what) {
  if (!ok) {
    printf("FAILED %s:%d: %s\n", file, line, what);
    ++failures;
  }
}
#define CHECK(cond) check((cond), __FILE__, __LINE__, #cond)

static int refusals = 0;
static void refused(int rc, const char* msg, int code, const char* word) {
  ++refusals;
  if (rc != code || !strstr(msg, word) || !strstr(msg, code == -2 ? "unsupported shape" : "bad argument")) {
    printf("FAILED refusal %d: rc %d (want %d), reason '%s' (want '%s')\n", refusals, rc, code, msg, word);
    ++failures;
  }
}

// a pointer that is never read: the plan only asks whether it is null (16-byte aligned, as `packed` must be)
alignas(16) static char some_bytes[16];
static const void* const some = some_bytes;

static VqnGeomGrid good_grid() {
  VqnGeomGrid g;
  g.origin[0] = g.origin[1] = g.origin[2] = -1.0f;
  g.h = 0.25f;
  g.dims[0] = 9, g.dims[1] = 10, g.dims[2] = 11;
  g.cells = 990;
  return g;
}

struct BinArgs {
  const void *verts = some, *tris = some, *cell_offset = some, *cursor = some, *bin = some, *packed = some;
  int64_t V = 100, T = 200, n_pairs = 300;
  VqnGeomGrid g = good_grid();
  bool no_grid = false;
};
static int bin(const BinArgs& a, char* msg, size_t n) {
  msg[0] = 0;
  return rays_bin_plan(a.verts, a.V, a.tris, a.T, a.no_grid ? nullptr : &a.g, a.cell_offset, a.n_pairs, a.cursor, a.bin, a.packed, msg, n);
}

struct CastArgs {
  const void *packed = some, *cell_offset = some, *bin = some, *o = some, *d = some, *tmin = some, *tmax = some;
  int64_t T = 200, n_pairs = 300, n = 1000;
  bool outs = true;
  VqnGeomGrid g = good_grid();
  bool no_grid = false;
};
static int cast(const CastArgs& a, char* msg, size_t n) {
  msg[0] = 0;
  return rays_cast_plan(a.packed, a.T, a.no_grid ? nullptr : &a.g, a.cell_offset, a.n_pairs, a.bin, a.o, a.d, a.tmin, a.tmax, a.n, a.outs, msg, n);
}

struct LightArgs {
  const void *packed = some, *cell_offset = some, *bin = some, *points = some, *normals = some, *lights = some, *out = some;
  int64_t T = 200, n_pairs = 300, n = 1000;
  int L = 512, lanes = 0;
  float bias = 0.01f;
  VqnGeomGrid g = good_grid();
  bool no_grid = false;
};
static int light(const LightArgs& a, char* msg, size_t n) {
  msg[0] = 0;
  return rays_light_plan(a.packed, a.T, a.no_grid ? nullptr : &a.g, a.cell_offset, a.n_pairs, a.bin, a.points, a.normals, a.n, a.lights, a.L, a.bias, a.lanes, a.out,
                         msg, n);
}

int main() {
  char msg[256];
  const int64_t two31 = (int64_t)1 << 31;
  const int64_t t_max = (two31 - 1) / 3;
  int shapes = 0;

  // ---- the limits as the header states them ----
  CHECK(kRaysMaxAxis == 1024 && kRaysMaxCells == (1 << 24) && kRaysStats == 3 && kRaysMargin == 0.0625f && kRaysPackedFloats == 12);
  CHECK(kRaysMaxLights == 65536 && kRaysTile == 64 && kRaysThreads == 256 && kRaysLdsBytes == 64 * 65 * 4);
  CHECK(VQN_RAYS_MIN_DIR_LOG2 == -60 && VQN_RAYS_LANES_POINTS == 0 && VQN_RAYS_LANES_LIGHTS == 1);

  // ---- the grid rule over a sweep: boxes flat, thin, a point, huge and tiny; triangle counts 0 .. 2^31 / 3; default and given cells ----
  const float sides[] = {0.0f, 1e-6f, 0.013f, 1.0f, 2.5f, 977.0f, 3e30f};
  const int64_t counts[] = {0, 1, 12, 320, 100000, 1500000, t_max};
  const float origins[] = {-3e30f, -1.5f, 0.0f, 7.25f};
  for (float sx : sides)
    for (float sy : sides)
      for (float sz : sides)
        for (int64_t T : counts)
          for (float at : origins) {
            const float lo[3] = {at, at, at}, hi[3] = {at + sx, at + sy, at + sz};
            if (!(isfinite(hi[0]) && isfinite(hi[1]) && isfinite(hi[2]))) continue;
            const double ext[3] = {(double)hi[0] - lo[0], (double)hi[1] - lo[1], (double)hi[2] - lo[2]};
            const double longest = fmax(ext[0], fmax(ext[1], ext[2]));
            for (int mode = 0; mode < 3; ++mode) {
              // the default; one cell for the whole box; 64 cells on the longest side
              const float cell = mode == 0 ? 0.0f : (mode == 1 ? (float)fmax(2.0 * longest, 1e-3) : (float)(longest / 64.0));
              if (mode == 2 && !(cell > 0.0f)) continue;
              VqnGeomGrid g;
              memset(&g, 0, sizeof(g));
              msg[0] = 0;
              const int rc = rays_grid_plan(lo, hi, T, cell, &g, msg, sizeof(msg));
              if (rc != 0) {
                // the only sizes of the sweep a plan may turn down: an origin that no float holds half a cell below lo
                CHECK(rc == -1 && at < -1e30f);
                continue;
              }
              ++shapes;
              int64_t cells = 1;
              for (int a = 0; a < 3; ++a) {
                CHECK(g.dims[a] >= 2 && g.dims[a] <= kRaysMaxAxis);
                CHECK(g.dims[a] == (int32_t)(floor(ext[a] / (double)g.h) + 2.0));
                cells *= g.dims[a];
                // the grid's box reaches beyond the mesh's on both sides
                CHECK(g.origin[a] <= lo[a] && (double)g.origin[a] + (double)g.dims[a] * (double)g.h >= (double)hi[a]);
                if (mode == 1) CHECK(g.dims[a] == 2);
              }
              CHECK(cells == g.cells && cells <= kRaysMaxCells && g.h > 0.0f && isfinite(g.h));
              if (cell > 0.0f) CHECK(g.h == cell);
              CHECK(rays_grid_check(&g, msg, sizeof(msg)) == 0);
            }
          }
  // the export-sized mesh: 1.5 M triangles in a unit box run into the cell cap, 256 cells a side and no more
  {
    const float lo[3] = {-0.5f, -0.5f, -0.5f}, hi[3] = {0.5f, 0.5f, 0.5f};
    VqnGeomGrid g;
    CHECK(rays_grid_plan(lo, hi, 1500000, 0.0f, &g, msg, sizeof(msg)) == 0);
    CHECK(g.cells <= kRaysMaxCells && g.dims[0] == g.dims[1] && g.dims[1] == g.dims[2] && g.dims[0] > 200 && g.dims[0] <= 256);
    CHECK(rays_grid_plan(lo, hi, 320, 0.0f, &g, msg, sizeof(msg)) == 0);
    CHECK(fabs((double)g.h - sqrt(2.0 * 6.0 / 320.0)) < 1e-6 && g.dims[0] == (int)floor(1.0 / g.h) + 2);
    ++shapes;
  }
  // the launches of the visibility kernel
  CHECK(rays_light_units(146779, 512, 0) == 2294 && rays_light_units(1, 1, 0) == 1 && rays_light_units(64, 7, 0) == 1 && rays_light_units(65, 7, 0) == 2);
  CHECK(rays_light_units(146779, 512, 1) == (146779ll * 8 + 3) / 4 && rays_light_units(1, 1, 1) == 1 && rays_light_units(5, 65, 1) == 3);

  // ---- refusals: the grid plan ----
  {
    const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1}, bad_hi[3] = {1, -1, 1}, inf_hi[3] = {1, INFINITY, 1}, nan_lo[3] = {0, NAN, 0};
    VqnGeomGrid g;
    refused(rays_grid_plan(nullptr, hi, 10, 0.0f, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    refused(rays_grid_plan(lo, nullptr, 10, 0.0f, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    refused(rays_grid_plan(lo, hi, 10, 0.0f, nullptr, msg, sizeof(msg)), msg, -1, "null pointer");
    refused(rays_grid_plan(lo, hi, -1, 0.0f, &g, msg, sizeof(msg)), msg, -1, "negative size");
    refused(rays_grid_plan(lo, hi, t_max + 1, 0.0f, &g, msg, sizeof(msg)), msg, -2, "3 n_tris");
    refused(rays_grid_plan(lo, bad_hi, 10, 0.0f, &g, msg, sizeof(msg)), msg, -1, "bounding box");
    refused(rays_grid_plan(lo, inf_hi, 10, 0.0f, &g, msg, sizeof(msg)), msg, -1, "bounding box");
    refused(rays_grid_plan(nan_lo, hi, 10, 0.0f, &g, msg, sizeof(msg)), msg, -1, "bounding box");
    refused(rays_grid_plan(lo, hi, 10, INFINITY, &g, msg, sizeof(msg)), msg, -2, "cell size");
    refused(rays_grid_plan(lo, hi, 10, 1.0f / 1030.0f, &g, msg, sizeof(msg)), msg, -2, "cell size");     // 1032 cells a side
    refused(rays_grid_plan(lo, hi, 10, 1.0f / 300.0f, &g, msg, sizeof(msg)), msg, -2, "cell size");      // 302^3 > 2^24
    CHECK(rays_grid_plan(lo, hi, 10, 1.0f / 254.5f, &g, msg, sizeof(msg)) == 0 && g.dims[0] == 256);
  }
  // ---- refusals: a grid handed to a device call ----
  {
    VqnGeomGrid g = good_grid();
    CHECK(rays_grid_check(&g, msg, sizeof(msg)) == 0);
    refused(rays_grid_check(nullptr, msg, sizeof(msg)), msg, -1, "null pointer");
    g = good_grid(), g.h = 0.0f;
    refused(rays_grid_check(&g, msg, sizeof(msg)), msg, -1, "cell size");
    g = good_grid(), g.h = NAN;
    refused(rays_grid_check(&g, msg, sizeof(msg)), msg, -1, "cell size");
    g = good_grid(), g.origin[1] = INFINITY;
    refused(rays_grid_check(&g, msg, sizeof(msg)), msg, -1, "origin");
    g = good_grid(), g.dims[2] = 0;
    refused(rays_grid_check(&g, msg, sizeof(msg)), msg, -1, "dims");
    g = good_grid(), g.dims[0] = 1025;
    refused(rays_grid_check(&g, msg, sizeof(msg)), msg, -2, "cells on an axis");
    g = good_grid(), g.dims[0] = g.dims[1] = g.dims[2] = 257, g.cells = 257 * 257 * 257;
    refused(rays_grid_check(&g, msg, sizeof(msg)), msg, -2, "2^24 cells");
    g = good_grid(), g.cells = 991;
    refused(rays_grid_check(&g, msg, sizeof(msg)), msg, -1, "product of its dims");
  }
  // ---- refusals: count ----
  {
    VqnGeomGrid g = good_grid();
    CHECK(rays_count_plan(some, 100, some, 200, &g, some, some, msg, sizeof(msg)) == 0);
    CHECK(rays_count_plan(nullptr, 0, nullptr, 0, &g, some, some, msg, sizeof(msg)) == 0);              // an empty mesh
    refused(rays_count_plan(some, -1, some, 200, &g, some, some, msg, sizeof(msg)), msg, -1, "negative size");
    refused(rays_count_plan(some, 100, some, -1, &g, some, some, msg, sizeof(msg)), msg, -1, "negative size");
    refused(rays_count_plan(some, two31, some, 200, &g, some, some, msg, sizeof(msg)), msg, -2, "n_verts");
    refused(rays_count_plan(some, 100, some, t_max + 1, &g, some, some, msg, sizeof(msg)), msg, -2, "3 n_tris");
    refused(rays_count_plan(nullptr, 100, some, 200, &g, some, some, msg, sizeof(msg)), msg, -1, "verts");
    refused(rays_count_plan(some, 100, nullptr, 200, &g, some, some, msg, sizeof(msg)), msg, -1, "tris");
    refused(rays_count_plan(some, 100, some, 200, &g, nullptr, some, msg, sizeof(msg)), msg, -1, "cell_count");
    refused(rays_count_plan(some, 100, some, 200, &g, some, nullptr, msg, sizeof(msg)), msg, -1, "stats");
    refused(rays_count_plan(some, 100, some, 200, nullptr, some, some, msg, sizeof(msg)), msg, -1, "grid");
    g.h = -1.0f;
    refused(rays_count_plan(some, 100, some, 200, &g, some, some, msg, sizeof(msg)), msg, -1, "cell size");
  }
  // ---- refusals: bin ----
  {
    BinArgs a;
    CHECK(bin(a, msg, sizeof(msg)) == 0);
    a = BinArgs(), a.n_pairs = 0, a.bin = nullptr;
    CHECK(bin(a, msg, sizeof(msg)) == 0);
    a = BinArgs(), a.T = 0, a.V = 0, a.n_pairs = 0, a.verts = a.tris = a.bin = a.packed = nullptr;
    CHECK(bin(a, msg, sizeof(msg)) == 0);
    a = BinArgs(), a.cell_offset = nullptr;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "cell_offset");
    a = BinArgs(), a.cursor = nullptr;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "cursor");
    a = BinArgs(), a.verts = nullptr;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "verts");
    a = BinArgs(), a.tris = nullptr;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "tris");
    a = BinArgs(), a.packed = nullptr;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "packed");
    a = BinArgs(), a.packed = some_bytes + 4;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "16-byte aligned");
    a = BinArgs(), a.bin = nullptr;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "bin");
    a = BinArgs(), a.n_pairs = -1;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "negative size");
    a = BinArgs(), a.n_pairs = two31, a.T = t_max;
    refused(bin(a, msg, sizeof(msg)), msg, -2, "n_pairs");
    a = BinArgs(), a.n_pairs = 200 * 990 + 1;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "contradicts");
    a = BinArgs(), a.no_grid = true;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "grid");
    a = BinArgs(), a.g.cells = 5;
    refused(bin(a, msg, sizeof(msg)), msg, -1, "product of its dims");
  }
  // ---- refusals: cast / occluded ----
  {
    CastArgs a;
    CHECK(cast(a, msg, sizeof(msg)) == 0);
    a = CastArgs(), a.n = 0, a.o = a.d = a.tmin = a.tmax = nullptr, a.outs = false;
    CHECK(cast(a, msg, sizeof(msg)) == 0);                                                            // zero rays
    a = CastArgs(), a.T = 0, a.n_pairs = 0, a.packed = a.bin = nullptr;
    CHECK(cast(a, msg, sizeof(msg)) == 0);                                                            // an empty mesh
    a = CastArgs(), a.n = -1;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "negative size");
    a = CastArgs(), a.n = two31;
    refused(cast(a, msg, sizeof(msg)), msg, -2, "rays");
    a = CastArgs(), a.T = -1;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "negative size");
    a = CastArgs(), a.packed = nullptr;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "packed");
    a = CastArgs(), a.packed = some_bytes + 8;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "16-byte aligned");
    a = CastArgs(), a.cell_offset = nullptr;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "cell_offset");
    a = CastArgs(), a.bin = nullptr;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "bin");
    a = CastArgs(), a.n_pairs = 200 * 990 + 1;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "contradicts");
    a = CastArgs(), a.o = nullptr;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "null pointer");
    a = CastArgs(), a.d = nullptr;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "null pointer");
    a = CastArgs(), a.tmin = nullptr;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "null pointer");
    a = CastArgs(), a.tmax = nullptr;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "null pointer");
    a = CastArgs(), a.outs = false;
    refused(cast(a, msg, sizeof(msg)), msg, -1, "an output");
    a = CastArgs(), a.g.dims[1] = 2000;
    refused(cast(a, msg, sizeof(msg)), msg, -2, "cells on an axis");
  }
  // ---- refusals: light visibility ----
  {
    LightArgs a;
    CHECK(light(a, msg, sizeof(msg)) == 0);
    a = LightArgs(), a.lanes = 1, a.L = 1;
    CHECK(light(a, msg, sizeof(msg)) == 0);
    a = LightArgs(), a.L = kRaysMaxLights;
    CHECK(light(a, msg, sizeof(msg)) == 0);
    a = LightArgs(), a.n = 0, a.points = a.normals = a.out = nullptr;
    CHECK(light(a, msg, sizeof(msg)) == 0);
    a = LightArgs(), a.L = 0;
    refused(light(a, msg, sizeof(msg)), msg, -2, "lights");
    a = LightArgs(), a.L = kRaysMaxLights + 1;
    refused(light(a, msg, sizeof(msg)), msg, -2, "lights");
    a = LightArgs(), a.n = two31;
    refused(light(a, msg, sizeof(msg)), msg, -2, "points");
    a = LightArgs(), a.n = (int64_t)1 << 24, a.L = kRaysMaxLights;
    refused(light(a, msg, sizeof(msg)), msg, -2, "2^40");
    a = LightArgs(), a.bias = NAN;
    refused(light(a, msg, sizeof(msg)), msg, -1, "bias");
    a = LightArgs(), a.bias = INFINITY;
    refused(light(a, msg, sizeof(msg)), msg, -1, "bias");
    a = LightArgs(), a.lanes = 2;
    refused(light(a, msg, sizeof(msg)), msg, -1, "lanes");
    a = LightArgs(), a.lanes = -1;
    refused(light(a, msg, sizeof(msg)), msg, -1, "lanes");
    a = LightArgs(), a.lights = nullptr;
    refused(light(a, msg, sizeof(msg)), msg, -1, "lights");
    a = LightArgs(), a.points = nullptr;
    refused(light(a, msg, sizeof(msg)), msg, -1, "points");
    a = LightArgs(), a.normals = nullptr;
    refused(light(a, msg, sizeof(msg)), msg, -1, "normals");
    a = LightArgs(), a.out = nullptr;
    refused(light(a, msg, sizeof(msg)), msg, -1, "out");
    a = LightArgs(), a.n = -1;
    refused(light(a, msg, sizeof(msg)), msg, -1, "negative size");
    a = LightArgs(), a.packed = nullptr;
    refused(light(a, msg, sizeof(msg)), msg, -1, "packed");
    a = LightArgs(), a.no_grid = true;
    refused(light(a, msg, sizeof(msg)), msg, -1, "grid");
  }

  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("mesh rays plan ok: %d shapes, %d refusals\n", shapes, refusals);
  return 0;
}
