// Host side of the mesh rasteriser (csrc/mesh_raster.hip): the sizes as the caller states them -> the limits, the tile grid, the sizes
// of the scratch arrays and of the staged chunk, with every refusal.  Plain C++, no HIP: tests/native/mesh_raster_host.cpp builds it
// into a stand-alone program under ASan / UBSan.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vqn_mesh_raster.h"  // (by path: the stand-alone build of this header names no include directory)

constexpr int kRasterTile = VQN_RASTER_TILE;
constexpr int kRasterSubpixelBits = VQN_RASTER_SUBPIXEL_BITS;
constexpr int kRasterSubpixel = 1 << VQN_RASTER_SUBPIXEL_BITS;
constexpr int kRasterMaxSide = VQN_RASTER_MAX_SIDE;
constexpr int kRasterCoordLimit = VQN_RASTER_COORD_LIMIT;
constexpr int kRasterChunk = VQN_RASTER_CHUNK;
constexpr int kRasterStats = VQN_RASTER_STATS;
constexpr int kRasterMaxChannels = VQN_RASTER_MAX_CHANNELS;
constexpr int kRasterThreads = kRasterTile * kRasterTile;     // one pixel per thread
constexpr int64_t kRasterIndexLimit = (int64_t)1 << 31;       // every index and every flat offset is an int32
// a staged triangle: per edge the two int32 steps and the int64 value at the tile's first sample, per corner 1 / w as a double, then
// |area2| (int64), the face index and the ownership bits
constexpr int kRasterStagedBytes = 3 * (4 + 4 + 8) + 3 * 8 + 8 + 4 + 4;
constexpr int kRasterLdsBytes = kRasterChunk * kRasterStagedBytes;
static_assert(kRasterThreads == 256 && kRasterChunk % kRasterThreads == 0, "every thread stages whole triangles of a chunk");
static_assert(kRasterLdsBytes <= 64 * 1024, "the staged chunk fits the LDS a kernel gets unasked");
// every edge function is exact in int64 and in a double: coordinates and samples below 2^24 in magnitude, differences below 2^25,
// products below 2^50, their differences below 2^51
static_assert((int64_t)kRasterCoordLimit <= ((int64_t)1 << 24) && (int64_t)kRasterMaxSide * kRasterSubpixel <= ((int64_t)1 << 24),
              "edge functions stay below 2^53");

struct RasterPlan {
  int64_t T, V;
  int32_t H, W;
  int32_t tiles_x, tiles_y;
  int64_t tiles;          // tiles_x * tiles_y <= 512 * 512: entries of tile_count, tile_offset and cursor
  int64_t pvert_words;    // 3 V: int32 entries of pverts
  int64_t pixels;         // H * W
  int64_t pair_limit;     // the largest n_pairs these sizes can give: min(T * tiles, 2^31 - 1)
};

#define RASTER_REFUSE(code, ...)         \
  do {                                   \
    snprintf(msg, msg_len, __VA_ARGS__); \
    return code;                         \
  } while (0)

// the sizes every entry point takes -> 0, or -1 (bad argument) / -2 (unsupported shape) with the reason in msg
inline int raster_plan(int64_t T, int64_t V, int H, int W, RasterPlan* out, char* msg, size_t msg_len) {
  memset(out, 0, sizeof(*out));
  if (T < 0 || V < 0) RASTER_REFUSE(-1, "bad argument: negative size: n_tris = %lld, n_verts = %lld", (long long)T, (long long)V);
  if (H < 1 || W < 1 || H > kRasterMaxSide || W > kRasterMaxSide)
    RASTER_REFUSE(-2, "unsupported shape: H and W must be 1 .. %d, got %d x %d", kRasterMaxSide, H, W);
  if (V >= kRasterIndexLimit) RASTER_REFUSE(-2, "unsupported shape: n_verts = %lld must be < 2^31", (long long)V);
  if (T >= (kRasterIndexLimit + 2) / 3) RASTER_REFUSE(-2, "unsupported shape: 3 n_tris must be < 2^31, n_tris = %lld", (long long)T);
  out->T = T, out->V = V, out->H = H, out->W = W;
  out->tiles_x = (W + kRasterTile - 1) / kRasterTile;
  out->tiles_y = (H + kRasterTile - 1) / kRasterTile;
  out->tiles = (int64_t)out->tiles_x * out->tiles_y;
  out->pvert_words = 3 * V;
  out->pixels = (int64_t)H * W;
  const int64_t most = T * out->tiles;                       // (< 2^30 * 2^18)
  out->pair_limit = most < kRasterIndexLimit - 1 ? most : kRasterIndexLimit - 1;
  return 0;
}

// vqn_raster_count: the arguments beyond the sizes
inline int raster_count_plan(const void* verts, int64_t V, const void* tris, int64_t T, const void* P, int H, int W, float near_plane, int cull,
                             const void* pverts, const void* tile_count, const void* stats, RasterPlan* out, char* msg, size_t msg_len) {
  memset(out, 0, sizeof(*out));
  if (T < 0 || V < 0) RASTER_REFUSE(-1, "bad argument: negative size: n_tris = %lld, n_verts = %lld", (long long)T, (long long)V);
  if (!(near_plane > 0.0f) || !isfinite(near_plane)) RASTER_REFUSE(-1, "bad argument: near must be positive and finite, got %g", (double)near_plane);
  if (cull < -1 || cull > 1) RASTER_REFUSE(-1, "bad argument: cull must be 0, +1 or -1, got %d", cull);
  if (!P || !tile_count || !stats) RASTER_REFUSE(-1, "bad argument: null pointer: P, tile_count or stats");
  if ((!verts || !pverts) && V > 0) RASTER_REFUSE(-1, "bad argument: null pointer: verts or pverts");
  if (!tris && T > 0) RASTER_REFUSE(-1, "bad argument: null pointer: tris");
  return raster_plan(T, V, H, W, out, msg, msg_len);
}

// vqn_raster_resolve
inline int raster_resolve_plan(const void* tris, int64_t T, const void* pverts, int64_t V, int H, int W, int cull, const void* tile_offset,
                               int64_t n_pairs, const void* cursor, const void* bin, const void* face, const void* depth, const void* bary,
                               RasterPlan* out, char* msg, size_t msg_len) {
  memset(out, 0, sizeof(*out));
  if (T < 0 || V < 0 || n_pairs < 0)
    RASTER_REFUSE(-1, "bad argument: negative size: n_tris = %lld, n_verts = %lld, n_pairs = %lld", (long long)T, (long long)V, (long long)n_pairs);
  if (cull < -1 || cull > 1) RASTER_REFUSE(-1, "bad argument: cull must be 0, +1 or -1, got %d", cull);
  if (!tile_offset || !cursor || !face || !depth || !bary)
    RASTER_REFUSE(-1, "bad argument: null pointer: tile_offset, cursor, face, depth or bary");
  if (!tris && T > 0) RASTER_REFUSE(-1, "bad argument: null pointer: tris");
  if (!pverts && V > 0) RASTER_REFUSE(-1, "bad argument: null pointer: pverts");
  if (!bin && n_pairs > 0) RASTER_REFUSE(-1, "bad argument: null pointer: bin");
  const int rc = raster_plan(T, V, H, W, out, msg, msg_len);
  if (rc) return rc;
  if (n_pairs >= kRasterIndexLimit) RASTER_REFUSE(-2, "unsupported shape: n_pairs = %lld must be < 2^31", (long long)n_pairs);
  if (n_pairs > out->pair_limit || (V == 0 && n_pairs > 0))
    RASTER_REFUSE(-1, "bad argument: n_pairs = %lld contradicts the sizes: %lld triangles on %lld tiles", (long long)n_pairs, (long long)T,
                  (long long)out->tiles);
  return 0;
}

// vqn_raster_interpolate
inline int raster_interpolate_plan(const void* face, const void* bary, int H, int W, const void* tris, int64_t T, const void* attr, int64_t V,
                                   int C, const void* background, const void* outp, RasterPlan* out, char* msg, size_t msg_len) {
  memset(out, 0, sizeof(*out));
  if (T < 0 || V < 0) RASTER_REFUSE(-1, "bad argument: negative size: n_tris = %lld, n_verts = %lld", (long long)T, (long long)V);
  if (!face || !bary || !background || !outp) RASTER_REFUSE(-1, "bad argument: null pointer: face, bary, background or out");
  if (!tris && T > 0) RASTER_REFUSE(-1, "bad argument: null pointer: tris");
  if (!attr && V > 0) RASTER_REFUSE(-1, "bad argument: null pointer: attr");
  const int rc = raster_plan(T, V, H, W, out, msg, msg_len);
  if (rc) return rc;
  if (C < 1 || C > kRasterMaxChannels) RASTER_REFUSE(-2, "unsupported shape: 1 .. %d channels, got %d", kRasterMaxChannels, C);
  return 0;
}
