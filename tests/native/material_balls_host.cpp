// Stand-alone check of the host side of the material-ball kernel (csrc/material_balls_plan.h) under ASan / UBSan: the grid, the probe
// chunks and their tables, the sheet geometry, the sizes, and every refusal with its reason.  Run by tests/test_material_balls_native.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "material_balls_plan.h"

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                \
    }                                                            \
  } while (0)

struct Call {
  int M = 64, P = 17, L = 512, ims = 128, spp = 4;
  float radius = 0.4f;
  bool inputs = true, f32 = true, u8 = false, sheet = false, scratch = true, aligned = true;
  const int32_t* order = nullptr;
  int n_order = 0, rows = 0, cols = 0;
  int64_t scratch_bytes = 288 * 1024;
  const float* rot = nullptr;
  const float* gamma = nullptr;
  int white_bg = 1;
};

static int plan(const Call& c, BallsPlan* g, char* msg, size_t len) {
  msg[0] = 0;
  return balls_plan(c.M, c.P, c.L, c.ims, c.spp, c.radius, c.rot, c.white_bg, c.gamma, c.inputs, c.f32, c.u8, c.sheet, c.order, c.n_order,
                    c.rows, c.cols, c.scratch, c.aligned, c.scratch_bytes, g, msg, len);
}

static int refusals = 0;
static void refused(const Call& c, int code, const char* word) {
  BallsPlan g;
  char msg[256];
  const int rc = plan(c, &g, msg, sizeof(msg));
  ++refusals;
  if (rc != code || !strstr(msg, word) || !strstr(msg, code == -2 ? "unsupported shape" : "bad argument")) {
    printf("FAILED refusal %d: rc %d (want %d), reason '%s' (want '%s')\n", refusals, rc, code, msg, word);
    ++failures;
  }
}

int main() {
  BallsPlan g;
  char msg[256];
  // ---- the flagship shape: 64 codes, the model's light and 16 probes, 512 lights, 128^2 at 4 spp ----
  Call c;
  CHECK(plan(c, &g, msg, sizeof(msg)) == 0 && msg[0] == 0);
  CHECK(g.sps == 2 && g.n_chunks == 1 && g.chunk[0].p0 == 0 && g.chunk[0].n_p == 17 && g.chunk[0].pairs == 26 && g.chunk[0].table_at == 0);
  CHECK(g.scratch_need == 512 * 52 * 4 && g.grid == 128 * 128 && g.lds_bytes == 512 * 20);
  CHECK(g.image_elems == 128 * 128 * 3 && g.out_elems == (int64_t)64 * 17 * 128 * 128 * 3);
  CHECK(g.a == 1.f / 3.f && g.step == (128.f - 2.f * (1.f / 3.f)) / 255.f && g.inv_spp == 0.25f && g.r2 == 0.4f * 0.4f);
  CHECK(g.cam[0] == 0.f && g.cam[1] == -10.f && g.cam[2] == 0.f);              // the default camera stands on -Y
  CHECK(g.has_gamma == 0 && g.white_bg == 1 && g.rows == 0);
  // ---- every probe count: the chunks cover the probes once, each has a kernel variant that holds it, the stated scratch suffices ----
  for (int P = 1; P <= kBallsMaxP; ++P)
    for (int L = 64; L <= kBallsMaxL; L += 64) {
      Call d;
      d.P = P, d.L = L, d.ims = 8, d.scratch_bytes = (int64_t)VQN_MATBALLS_SCRATCH_PER_LIGHT * L;
      CHECK(plan(d, &g, msg, sizeof(msg)) == 0);
      int covered = 0;
      int64_t at = 0;
      for (int i = 0; i < g.n_chunks; ++i) {
        const BallsChunk& ch = g.chunk[i];
        CHECK(ch.p0 == covered && ch.n_p >= 1 && 2 * ch.pairs >= 3 * ch.n_p && ch.table_at == at && ch.table_at % 4 == 0);
        bool compiled = false;
        for (int v = 0; v < 5; ++v) compiled = compiled || kBallsPairs[v] == ch.pairs;
        CHECK(compiled);
        covered += ch.n_p, at += (int64_t)L * 2 * ch.pairs;
      }
      CHECK(covered == P && at * 4 == g.scratch_need && g.scratch_need <= d.scratch_bytes);
      d.scratch_bytes = g.scratch_need;                                         // exactly enough passes, one byte less does not
      CHECK(plan(d, &g, msg, sizeof(msg)) == 0);
      d.scratch_bytes -= 1;
      CHECK(plan(d, &g, msg, sizeof(msg)) == -1);
    }
  // ---- the sample grid of the smallest and of an odd image ----
  {
    Call d;
    d.ims = 1, d.spp = 1;
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0 && g.a == 0.5f && g.step == 0.f && g.grid == 1);
    d.ims = 33, d.spp = 9;
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0 && g.sps == 3 && g.a == 0.25f && g.step == (33.f - 0.5f) / 98.f && g.grid == 33 * 33);
  }
  // ---- a sheet: every material's cell, and where its bytes lie ----
  {
    Call d;
    d.M = 5, d.ims = 4, d.sheet = true, d.f32 = false;
    const int32_t order[4] = {3, 0, 4, 1};
    d.order = order, d.n_order = 4, d.rows = 2, d.cols = 3, d.P = 2;
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0);
    CHECK(g.cell_of[3] == 0 && g.cell_of[0] == 1 && g.cell_of[4] == 2 && g.cell_of[1] == 3 && g.cell_of[2] == kBallsNoCell);
    CHECK(g.sheet_bytes == 2 * 8 * 12 * 3);
    std::vector<int> hit((size_t)g.sheet_bytes, 0);                             // every byte of a shown cell is addressed exactly once
    for (int p = 0; p < 2; ++p)
      for (int cell = 0; cell < 4; ++cell)
        for (int y = 0; y < 4; ++y)
          for (int x = 0; x < 4; ++x)
            for (int ch = 0; ch < 3; ++ch) {
              const int64_t i = balls_sheet_index(g, p, cell, y, x, ch);
              CHECK(i >= 0 && i < g.sheet_bytes);
              if (i >= 0 && i < g.sheet_bytes) ++hit[(size_t)i];
            }
    int once = 0;
    for (int v : hit) {
      CHECK(v <= 1);
      once += v;
    }
    CHECK(once == 2 * 4 * 4 * 4 * 3);
    CHECK(balls_sheet_index(g, 1, 3, 2, 1, 0) == ((int64_t)(8 + 4 + 2) * 12 + 1) * 3);      // cell 3 = row 1, column 0
    d.order = nullptr, d.n_order = 0, d.rows = 1, d.cols = 5;                   // no order: 0 .. M - 1
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0 && g.n_order == 5 && g.cell_of[4] == 4);
  }
  // ---- the largest outputs that pass, and the first that do not ----
  {
    Call d;
    d.M = 1, d.P = 1, d.ims = 1024, d.spp = 16;
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0 && g.sps == 4 && g.out_elems * 4 <= kBallsMaxBytes);
    d.M = 65, d.P = 24, d.ims = 338;                                           // 65 * 24 * 338^2 * 3 * 4 B = 2,138,660,160 <= 2^31 - 1
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0);
    d.ims = 339;
    refused(d, -2, "exceed");
    d.f32 = false, d.u8 = true;                                                // the byte image is a quarter of it
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0);
    Call s;
    s.M = 65, s.P = 24, s.ims = 1024, s.f32 = false, s.sheet = true, s.rows = 5, s.cols = 13;
    refused(s, -2, "sheet");
  }
  // ---- refusals ----
  { Call d; d.M = 0; refused(d, -2, "materials"); }
  { Call d; d.M = 66; refused(d, -2, "materials"); }
  { Call d; d.P = 0; refused(d, -2, "probes"); }
  { Call d; d.P = 25; refused(d, -2, "probes"); }
  { Call d; d.L = 96; refused(d, -2, "multiple of 64"); }
  { Call d; d.L = 0; refused(d, -2, "multiple of 64"); }
  { Call d; d.L = 1088; refused(d, -2, "up to 1024"); }
  { Call d; d.ims = 0; refused(d, -2, "ims"); }
  { Call d; d.ims = 1025; refused(d, -2, "ims"); }
  { Call d; d.spp = 2; refused(d, -2, "square"); }
  { Call d; d.spp = 25; refused(d, -2, "square"); }
  { Call d; d.spp = 0; refused(d, -2, "square"); }
  { Call d; d.inputs = false; refused(d, -1, "null"); }
  { Call d; d.f32 = false; refused(d, -1, "no output"); }
  { Call d; d.radius = 0.f; refused(d, -1, "sphere_radius"); }
  { Call d; d.radius = 0.6f; refused(d, -1, "sphere_radius"); }
  { Call d; d.radius = strtof("nan", nullptr); refused(d, -1, "sphere_radius"); }
  { Call d; d.sheet = true; d.rows = 7; d.cols = 9; refused(d, -1, "does not hold"); }       // 63 cells for 64 balls
  { Call d; d.sheet = true; d.rows = 0; d.cols = 64; refused(d, -1, "does not hold"); }
  { Call d; d.sheet = true; d.rows = 1; d.cols = 66; d.M = 65; refused(d, -1, "at most 65"); }
  { Call d; const int32_t o[2] = {0, 64}; d.sheet = true; d.order = o; d.n_order = 2; d.rows = d.cols = 2; refused(d, -1, "order[1]"); }
  { Call d; const int32_t o[2] = {-1, 3}; d.sheet = true; d.order = o; d.n_order = 2; d.rows = d.cols = 2; refused(d, -1, "order[0]"); }
  { Call d; const int32_t o[2] = {3, 3}; d.sheet = true; d.order = o; d.n_order = 2; d.rows = d.cols = 2; refused(d, -1, "twice"); }
  { Call d; const int32_t o[1] = {0}; d.sheet = true; d.order = o; d.n_order = 65; d.rows = d.cols = 9; refused(d, -1, "shows"); }
  { Call d; d.scratch = false; refused(d, -1, "scratch"); }
  { Call d; d.aligned = false; refused(d, -1, "scratch"); }
  { Call d; d.scratch_bytes = 512 * 52 * 4 - 1; refused(d, -1, "scratch"); }
  // ---- camera and gamma pass through ----
  {
    Call d;
    const float rot[9] = {0.f, 0.f, 1.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}, gam[2] = {2.f, 0.5f};
    d.rot = rot, d.gamma = gam, d.white_bg = 0;
    CHECK(plan(d, &g, msg, sizeof(msg)) == 0 && g.cam[0] == 10.f && g.cam[1] == 0.f && g.cam[2] == 0.f && g.rot[3] == 1.f);
    CHECK(g.has_gamma == 1 && g.gamma[0] == 2.f && g.gamma[1] == 0.5f && g.white_bg == 0);
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("material balls plan ok: 384 probe / light shapes, %d refusals\n", refusals + 384);
  return 0;
}
