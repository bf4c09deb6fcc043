// Host side of the material-ball kernel (csrc/material_balls.hip): the call as the caller states it -> the sample grid, the sheet
// geometry, the sizes and the launch grid, with every refusal.  Plain C++, no HIP: tests/native/material_balls_host.cpp builds it into
// a stand-alone program under ASan / UBSan.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vqn_material_balls.h"  // (by path: the stand-alone build of this header names no include directory)

constexpr int kBallsMaxM = VQN_MATBALLS_MAX_MATERIALS;
constexpr int kBallsMaxP = VQN_MATBALLS_MAX_PROBES;
constexpr int kBallsLightStep = VQN_MATBALLS_LIGHT_STEP;
constexpr int kBallsMaxL = VQN_MATBALLS_MAX_LIGHTS;
constexpr int kBallsMaxIms = VQN_MATBALLS_MAX_IMS;
constexpr int kBallsMaxSps = VQN_MATBALLS_MAX_SPS;
constexpr int kBallsSumBlock = VQN_MATBALLS_SUM_BLOCK;
constexpr int64_t kBallsMaxBytes = VQN_MATBALLS_MAX_OUT_BYTES;
constexpr float kBallsCamDist = 10.f;               // the reference's cam_dist
constexpr int kBallsNoCell = 255;                   // BallsPlan::cell_of of a material the sheet does not show

// the probes of one launch: n_p from p0 on; the kernel variant `pairs` = accumulator pairs per lane, the smallest of kBallsPairs that
// holds 3 n_p values; the launch's probe table [L][2 * pairs] (the kernel reads whole rows) starts at float table_at of the scratch
struct BallsChunk {
  int32_t p0, n_p, pairs;
  int64_t table_at;
};

struct BallsPlan {
  int32_t M, P, L, ims, sps;
  int32_t n_chunks;                 // launches: all probes in one up to kBallsChunkMax, else the first kBallsChunkSplit and the rest
  BallsChunk chunk[2];
  float a, step, radius, r2, inv_spp;      // sample grid: u_i = (a + i * step) / ims
  float rot[9], cam[3];             // camera frame -> light frame, and the camera's position there
  float gamma[2];
  int32_t has_gamma, white_bg;
  int32_t rows, cols, n_order;      // the sheet (0 when there is none)
  uint8_t cell_of[kBallsMaxM];      // material -> the cell that shows it, or kBallsNoCell
  int64_t image_elems;              // ims * ims * 3
  int64_t out_elems;                // M * P * image_elems
  int64_t sheet_bytes;              // P * rows * ims * cols * ims * 3
  int64_t scratch_need;             // bytes of the probe tables
  int64_t grid;                     // workgroups: one 64-lane wave per pixel
  int64_t lds_bytes;                // a wave's list of front-lit lights: L x (4 floats + the light's index)
};

// accumulator pairs the kernel is compiled for: 3 n_p values in pairs, n_p = 1, <= 4, <= 8, <= 12, <= 17 (the model's light and 16
// probes).  Three accumulator sets of a lane (block sum, total, pixel) at 26 pairs are 156 registers; at the 36 pairs of 24 probes the
// kernel would spill, so more than 17 probes go in two launches
constexpr int kBallsPairs[5] = {2, 6, 12, 18, 26};
constexpr int kBallsChunkMax = 17, kBallsChunkSplit = 12;
static_assert(2 * kBallsPairs[4] >= 3 * kBallsChunkMax && 2 * kBallsPairs[3] >= 3 * kBallsChunkSplit &&
                  kBallsMaxP - kBallsChunkSplit <= kBallsChunkSplit,
              "every chunk has a kernel variant");
static_assert(2 * (2 * kBallsPairs[3]) * 4 <= VQN_MATBALLS_SCRATCH_PER_LIGHT && 2 * kBallsPairs[4] * 4 <= VQN_MATBALLS_SCRATCH_PER_LIGHT,
              "the stated scratch holds the tables");

#define BALLS_REFUSE(code, ...)          \
  do {                                   \
    snprintf(msg, msg_len, __VA_ARGS__); \
    return code;                         \
  } while (0)

// have_* : which pointers of the call are non-null.  -> 0, or -1 (bad argument) / -2 (unsupported shape) with the reason in msg.
inline int balls_plan(int M, int P, int L, int ims, int spp, float radius, const float* cam_rot, int white_bg, const float* gamma,
                      bool have_inputs, bool have_f32, bool have_u8, bool have_sheet, const int32_t* order, int n_order, int rows, int cols,
                      bool have_scratch, bool scratch_aligned, int64_t scratch_bytes, BallsPlan* out, char* msg, size_t msg_len) {
  memset(out, 0, sizeof(*out));
  if (M < 1 || M > kBallsMaxM) BALLS_REFUSE(-2, "unsupported shape: 1 .. %d materials, got %d", kBallsMaxM, M);
  if (P < 1 || P > kBallsMaxP) BALLS_REFUSE(-2, "unsupported shape: 1 .. %d probes, got %d", kBallsMaxP, P);
  if (L < kBallsLightStep || L > kBallsMaxL || L % kBallsLightStep != 0)
    BALLS_REFUSE(-2, "unsupported shape: the lights are a multiple of %d up to %d, got %d", kBallsLightStep, kBallsMaxL, L);
  if (ims < 1 || ims > kBallsMaxIms) BALLS_REFUSE(-2, "unsupported shape: ims is 1 .. %d, got %d", kBallsMaxIms, ims);
  int sps = 0;
  for (int s = 1; s <= kBallsMaxSps; ++s)
    if (s * s == spp) sps = s;
  if (!sps) BALLS_REFUSE(-2, "unsupported shape: spp is a square, 1 .. %d, got %d", kBallsMaxSps * kBallsMaxSps, spp);
  if (!have_inputs) BALLS_REFUSE(-1, "bad argument: null materials / lights / lxyz / areas");
  if (!have_f32 && !have_u8 && !have_sheet) BALLS_REFUSE(-1, "bad argument: no output: out_f32, out_u8 and sheet are all null");
  if (!(radius > 0.f && radius <= 0.5f)) BALLS_REFUSE(-1, "bad argument: sphere_radius must lie in (0, 0.5], got %g", (double)radius);
  out->M = M, out->P = P, out->L = L, out->ims = ims, out->sps = sps;
  out->n_chunks = P <= kBallsChunkMax ? 1 : 2;
  for (int c = 0; c < out->n_chunks; ++c) {
    BallsChunk& ch = out->chunk[c];
    ch.p0 = c * kBallsChunkSplit;
    ch.n_p = out->n_chunks == 1 ? P : (c == 0 ? kBallsChunkSplit : P - kBallsChunkSplit);
    for (int i = 4; i >= 0; --i)
      if (2 * kBallsPairs[i] >= 3 * ch.n_p) ch.pairs = kBallsPairs[i];
    ch.table_at = out->scratch_need / 4;
    out->scratch_need += (int64_t)L * 2 * ch.pairs * 4;
  }
  out->image_elems = (int64_t)ims * ims * 3;
  out->out_elems = (int64_t)M * P * out->image_elems;
  if ((have_f32 && out->out_elems * 4 > kBallsMaxBytes) || (have_u8 && out->out_elems > kBallsMaxBytes))
    BALLS_REFUSE(-2, "unsupported shape: %d x %d images of %d x %d pixels exceed the %lld bytes of an output buffer", M, P, ims, ims,
                 (long long)kBallsMaxBytes);
  if (have_sheet) {
    if (!order) n_order = M;
    if (n_order < 1 || n_order > M) BALLS_REFUSE(-1, "bad argument: a sheet shows 1 .. %d of the %d balls, got %d", M, M, n_order);
    if (rows < 1 || cols < 1 || (int64_t)rows * cols < n_order)
      BALLS_REFUSE(-1, "bad argument: a sheet of %d x %d cells does not hold %d balls", rows, cols, n_order);
    if (rows > kBallsMaxM || cols > kBallsMaxM) BALLS_REFUSE(-1, "bad argument: a sheet has at most %d rows and columns", kBallsMaxM);
    memset(out->cell_of, kBallsNoCell, sizeof(out->cell_of));
    for (int i = 0; i < n_order; ++i) {
      const int m = order ? order[i] : i;
      if (m < 0 || m >= M) BALLS_REFUSE(-1, "bad argument: order[%d] is %d, materials are 0 .. %d", i, m, M - 1);
      if (out->cell_of[m] != kBallsNoCell) BALLS_REFUSE(-1, "bad argument: order names material %d twice", m);
      out->cell_of[m] = (uint8_t)i;
    }
    out->rows = rows, out->cols = cols, out->n_order = n_order;
    out->sheet_bytes = (int64_t)P * rows * ims * cols * ims * 3;
    if (out->sheet_bytes > kBallsMaxBytes)
      BALLS_REFUSE(-2, "unsupported shape: a sheet of %d x %d cells of %d x %d pixels under %d probes exceeds %lld bytes", rows, cols, ims, ims,
                   P, (long long)kBallsMaxBytes);
  }
  if (!have_scratch || !scratch_aligned || scratch_bytes < out->scratch_need)
    BALLS_REFUSE(-1, "bad argument: scratch must be 16-byte aligned and hold %lld bytes, got %lld", (long long)out->scratch_need,
                 (long long)(have_scratch ? scratch_bytes : 0));
  // the sample grid, in f32 as the kernel and the model evaluate it
  const int n = ims * sps;
  out->a = 1.f / (float)(sps + 1);
  out->step = n > 1 ? ((float)ims - 2.f * out->a) / (float)(n - 1) : 0.f;
  out->radius = radius, out->r2 = radius * radius;
  out->inv_spp = 1.f / (float)(sps * sps);
  static const float kDefaultRot[9] = {1.f, 0.f, 0.f, 0.f, 0.f, -1.f, 0.f, 1.f, 0.f};
  memcpy(out->rot, cam_rot ? cam_rot : kDefaultRot, sizeof(out->rot));
  for (int r = 0; r < 3; ++r) out->cam[r] = out->rot[3 * r + 2] * kBallsCamDist;
  out->has_gamma = gamma != nullptr, out->white_bg = white_bg != 0;
  out->gamma[0] = gamma ? gamma[0] : 1.f, out->gamma[1] = gamma ? gamma[1] : 1.f;
  out->grid = (int64_t)ims * ims;
  out->lds_bytes = (int64_t)L * 20;
  return 0;
}

// where byte (pixel y, x, channel c) of material cell `cell` under probe p lies in the sheet
inline int64_t balls_sheet_index(const BallsPlan& g, int p, int cell, int y, int x, int c) {
  const int64_t W = (int64_t)g.cols * g.ims;
  return (((int64_t)p * g.rows * g.ims + (int64_t)(cell / g.cols) * g.ims + y) * W + (int64_t)(cell % g.cols) * g.ims + x) * 3 + c;
}
