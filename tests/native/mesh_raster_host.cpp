// Stand-alone check of the host side of the mesh rasteriser (csrc/mesh_raster_plan.h) under ASan / UBSan: the limits, the tile grid at
// its edges, the sizes of the scratch arrays and of the bin, the LDS of the staged chunk, and every refusal of the three entry points
// with its reason.  Run by tests/test_mesh_raster_native.py.
#include <initializer_list>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mesh_raster_plan.h"

static int failures = 0;
static void check(bool ok, const char* file, int line, const char* what) {
  if (!ok) {
    printf("FAILED %s:%d: %s\n", file, line, what);
    ++failures;
  }
}
#define CHECK(cond) check((cond), __FILE__, __LINE__, #cond)      // (an expression: it follows a comma below)

static int refusals = 0;
static void refused(int rc, const char* msg, int code, const char* word) {
  ++refusals;
  if (rc != code || !strstr(msg, word) || !strstr(msg, code == -2 ? "unsupported shape" : "bad argument")) {
    printf("FAILED refusal %d: rc %d (want %d), reason '%s' (want '%s')\n", refusals, rc, code, msg, word);
    ++failures;
  }
}

// a pointer that is never read: the plan only asks whether it is null
static const void* const some = &failures;

struct CountArgs {
  const void *verts = some, *tris = some, *P = some, *pverts = some, *tile_count = some, *stats = some;
  int64_t V = 100, T = 200;
  int H = 40, W = 24, cull = 0;
  float near_plane = 1e-3f;
};
static int count(const CountArgs& a, RasterPlan* g, char* msg, size_t n) {
  msg[0] = 0;
  return raster_count_plan(a.verts, a.V, a.tris, a.T, a.P, a.H, a.W, a.near_plane, a.cull, a.pverts, a.tile_count, a.stats, g, msg, n);
}

struct ResolveArgs {
  const void *tris = some, *pverts = some, *tile_offset = some, *cursor = some, *bin = some, *face = some, *depth = some, *bary = some;
  int64_t V = 100, T = 200, n_pairs = 300;
  int H = 40, W = 24, cull = 0;
};
static int resolve(const ResolveArgs& a, RasterPlan* g, char* msg, size_t n) {
  msg[0] = 0;
  return raster_resolve_plan(a.tris, a.T, a.pverts, a.V, a.H, a.W, a.cull, a.tile_offset, a.n_pairs, a.cursor, a.bin, a.face, a.depth, a.bary, g,
                             msg, n);
}

struct InterpArgs {
  const void *face = some, *bary = some, *tris = some, *attr = some, *background = some, *out = some;
  int64_t V = 100, T = 200;
  int H = 40, W = 24, C = 3;
};
static int interp(const InterpArgs& a, RasterPlan* g, char* msg, size_t n) {
  msg[0] = 0;
  return raster_interpolate_plan(a.face, a.bary, a.H, a.W, a.tris, a.T, a.attr, a.V, a.C, a.background, a.out, g, msg, n);
}

int main() {
  RasterPlan g;
  char msg[256];
  const int64_t two31 = (int64_t)1 << 31;
  const int64_t t_max = (two31 - 1) / 3;
  int shapes = 0;

  // ---- the limits as the header states them, and what the kernel's arithmetic rests on ----
  CHECK(kRasterTile == 16 && kRasterSubpixelBits == 8 && kRasterSubpixel == 256 && kRasterMaxSide == 8192 && kRasterCoordLimit == (1 << 23));
  CHECK(kRasterThreads == 256 && kRasterChunk >= 1 && kRasterChunk % kRasterThreads == 0 && kRasterStats == 4 && kRasterMaxChannels == 16);
  CHECK(kRasterStagedBytes == 88 && kRasterLdsBytes == kRasterChunk * 88 && kRasterLdsBytes <= 64 * 1024);
  // the largest edge function: |difference of two coordinates| * |sample - coordinate|, twice, stays exact in a double
  const int64_t span = 2 * (int64_t)kRasterCoordLimit, reach = (int64_t)kRasterCoordLimit + (int64_t)kRasterMaxSide * kRasterSubpixel;
  CHECK(2 * span * reach < ((int64_t)1 << 53) && span < two31);

  // ---- an export-sized mesh at 800 x 800 ----
  msg[0] = 0;
  CHECK(raster_plan(2000000, 1000000, 800, 800, &g, msg, sizeof(msg)) == 0 && msg[0] == 0);
  CHECK(g.tiles_x == 50 && g.tiles_y == 50 && g.tiles == 2500 && g.pvert_words == 3000000 && g.pixels == 640000);
  CHECK(g.pair_limit == two31 - 1);                              // (2 * 10^6 * 2500 pairs could not be held: the limit binds)

  // ---- the tile grid at its edges ----
  const int sides[] = {1, 15, 16, 17, 31, 32, 33, 800, 8191, 8192};
  const int64_t Ts[] = {0, 1, 255, 256, 257, 100000, t_max};
  const int64_t Vs[] = {0, 1, 3, 5000, two31 - 1};
  for (int H : sides)
    for (int W : sides)
      for (int64_t T : Ts)
        for (int64_t V : Vs) {
          msg[0] = 0;
          const int rc = raster_plan(T, V, H, W, &g, msg, sizeof(msg));
          ++shapes;
          CHECK(rc == 0 && msg[0] == 0);
          CHECK(g.tiles_x * 16 >= W && (g.tiles_x - 1) * 16 < W && g.tiles_y * 16 >= H && (g.tiles_y - 1) * 16 < H);
          CHECK(g.tiles == (int64_t)g.tiles_x * g.tiles_y && g.tiles >= 1 && g.tiles <= 512 * 512);
          CHECK(g.pvert_words == 3 * V && g.pixels == (int64_t)H * W && g.pixels * kRasterMaxChannels < ((int64_t)1 << 62));
          CHECK(g.pair_limit >= 0 && g.pair_limit < two31 && g.pair_limit <= T * g.tiles && (g.pair_limit == T * g.tiles || g.pair_limit == two31 - 1));
          // the three entry points take the same sizes
          CountArgs c;
          c.T = T, c.V = V, c.H = H, c.W = W;
          RasterPlan g2;
          CHECK(count(c, &g2, msg, sizeof(msg)) == 0 && memcmp(&g, &g2, sizeof(g)) == 0);
          ResolveArgs r;
          r.T = T, r.V = V, r.H = H, r.W = W, r.n_pairs = V ? g.pair_limit : 0;
          CHECK(resolve(r, &g2, msg, sizeof(msg)) == 0 && memcmp(&g, &g2, sizeof(g)) == 0);
          InterpArgs i;
          i.T = T, i.V = V, i.H = H, i.W = W;
          CHECK(interp(i, &g2, msg, sizeof(msg)) == 0 && memcmp(&g, &g2, sizeof(g)) == 0);
        }

  // ---- empty arrays may be null ----
  {
    CountArgs c;
    c.V = 0, c.T = 0, c.verts = c.pverts = c.tris = nullptr;
    CHECK(count(c, &g, msg, sizeof(msg)) == 0);
    ResolveArgs r;
    r.V = 0, r.T = 0, r.n_pairs = 0, r.tris = r.pverts = r.bin = nullptr;
    CHECK(resolve(r, &g, msg, sizeof(msg)) == 0);
    InterpArgs i;
    i.V = 0, i.T = 0, i.tris = i.attr = nullptr;
    CHECK(interp(i, &g, msg, sizeof(msg)) == 0);
  }

  // ---- refusals: vqn_raster_count ----
  {
    CountArgs c;
    c = CountArgs(), c.T = -1, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "negative size");
    c = CountArgs(), c.V = -1, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "negative size");
    c = CountArgs(), c.V = -1, c.H = 0, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "negative size");   // before any shape
    const float nears[] = {0.0f, -1.0f, INFINITY, NAN};
    for (float n : nears) c = CountArgs(), c.near_plane = n, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "near");
    for (int cull : {-2, 2, 100}) c = CountArgs(), c.cull = cull, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "cull");
    for (int cull : {-1, 0, 1}) c = CountArgs(), c.cull = cull, CHECK(count(c, &g, msg, sizeof(msg)) == 0);
    c = CountArgs(), c.P = nullptr, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    c = CountArgs(), c.tile_count = nullptr, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    c = CountArgs(), c.stats = nullptr, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    c = CountArgs(), c.verts = nullptr, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    c = CountArgs(), c.pverts = nullptr, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    c = CountArgs(), c.tris = nullptr, refused(count(c, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    for (int side : {0, -5, 8193, 1 << 30}) {
      c = CountArgs(), c.H = side, refused(count(c, &g, msg, sizeof(msg)), msg, -2, "H and W");
      c = CountArgs(), c.W = side, refused(count(c, &g, msg, sizeof(msg)), msg, -2, "H and W");
    }
    c = CountArgs(), c.V = two31, refused(count(c, &g, msg, sizeof(msg)), msg, -2, "n_verts");
    c = CountArgs(), c.T = t_max + 1, refused(count(c, &g, msg, sizeof(msg)), msg, -2, "3 n_tris");
    c = CountArgs(), c.T = two31, refused(count(c, &g, msg, sizeof(msg)), msg, -2, "3 n_tris");
    CHECK(3 * t_max < two31 && 3 * (t_max + 1) >= two31);
  }

  // ---- refusals: vqn_raster_resolve ----
  {
    ResolveArgs r;
    r = ResolveArgs(), r.T = -1, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "negative size");
    r = ResolveArgs(), r.V = -1, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "negative size");
    r = ResolveArgs(), r.n_pairs = -1, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "negative size");
    for (int cull : {-2, 2}) r = ResolveArgs(), r.cull = cull, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "cull");
    const void* ResolveArgs::*always[] = {&ResolveArgs::tile_offset, &ResolveArgs::cursor, &ResolveArgs::face, &ResolveArgs::depth, &ResolveArgs::bary,
                                          &ResolveArgs::tris, &ResolveArgs::pverts, &ResolveArgs::bin};
    for (auto member : always) r = ResolveArgs(), r.*member = nullptr, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    for (int side : {0, 8193}) {
      r = ResolveArgs(), r.H = side, refused(resolve(r, &g, msg, sizeof(msg)), msg, -2, "H and W");
      r = ResolveArgs(), r.W = side, refused(resolve(r, &g, msg, sizeof(msg)), msg, -2, "H and W");
    }
    r = ResolveArgs(), r.V = two31, refused(resolve(r, &g, msg, sizeof(msg)), msg, -2, "n_verts");
    r = ResolveArgs(), r.T = t_max + 1, refused(resolve(r, &g, msg, sizeof(msg)), msg, -2, "3 n_tris");
    // the pairs: 2^31 and more is a shape, more than the sizes can give is a contradiction
    r = ResolveArgs(), r.T = t_max, r.H = r.W = 8192, r.n_pairs = two31, refused(resolve(r, &g, msg, sizeof(msg)), msg, -2, "n_pairs");
    r = ResolveArgs(), r.T = t_max, r.H = r.W = 8192, r.n_pairs = two31 - 1, CHECK(resolve(r, &g, msg, sizeof(msg)) == 0);
    r = ResolveArgs(), r.n_pairs = 200 * 6 + 1, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "contradicts");      // 40 x 24: 3 x 2 tiles
    r = ResolveArgs(), r.n_pairs = 200 * 6, CHECK(resolve(r, &g, msg, sizeof(msg)) == 0);
    r = ResolveArgs(), r.T = 0, r.n_pairs = 1, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "contradicts");
    r = ResolveArgs(), r.V = 0, r.n_pairs = 1, refused(resolve(r, &g, msg, sizeof(msg)), msg, -1, "contradicts");
  }

  // ---- refusals: vqn_raster_interpolate ----
  {
    InterpArgs i;
    i = InterpArgs(), i.T = -1, refused(interp(i, &g, msg, sizeof(msg)), msg, -1, "negative size");
    i = InterpArgs(), i.V = -1, refused(interp(i, &g, msg, sizeof(msg)), msg, -1, "negative size");
    const void* InterpArgs::*always[] = {&InterpArgs::face, &InterpArgs::bary, &InterpArgs::background, &InterpArgs::out, &InterpArgs::tris,
                                         &InterpArgs::attr};
    for (auto member : always) i = InterpArgs(), i.*member = nullptr, refused(interp(i, &g, msg, sizeof(msg)), msg, -1, "null pointer");
    for (int C : {0, -1, 17, 1000}) i = InterpArgs(), i.C = C, refused(interp(i, &g, msg, sizeof(msg)), msg, -2, "channels");
    for (int C : {1, 3, 16}) i = InterpArgs(), i.C = C, CHECK(interp(i, &g, msg, sizeof(msg)) == 0);
    for (int side : {0, 8193}) {
      i = InterpArgs(), i.H = side, refused(interp(i, &g, msg, sizeof(msg)), msg, -2, "H and W");
      i = InterpArgs(), i.W = side, refused(interp(i, &g, msg, sizeof(msg)), msg, -2, "H and W");
    }
    i = InterpArgs(), i.V = two31, refused(interp(i, &g, msg, sizeof(msg)), msg, -2, "n_verts");
    i = InterpArgs(), i.T = t_max + 1, refused(interp(i, &g, msg, sizeof(msg)), msg, -2, "3 n_tris");
  }

  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("mesh raster plan ok: %d shapes, %d refusals\n", shapes, refusals);
  return 0;
}
