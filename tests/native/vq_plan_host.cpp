// AddressSanitizer / UBSan check of the host-only C++ of the VQ host side (csrc/vq_plan.h): a table of shapes -> decisions for 256 CUs,
// written down from the expressions the entry points of csrc/vq.hip held before the plan existed -- every refusal once, both sides of
// every threshold.  Built and run by tests/test_vq_plan_native.py:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ivqnerf_release_amd/csrc
//       tests/native/vq_plan_host.cpp
#include <stdio.h>
#include <string.h>

#include "vq_plan.h"

static int failures = 0, rows = 0;
static void expect(bool ok, const char* what, int row) {
  ++rows;
  if (!ok) {
    fprintf(stderr, "FAIL: %s (row %d)\n", what, row);
    ++failures;
  }
}

constexpr int CUS = 256;
static const char* const kTooManyCodes = "K <= 128";
static const char* const kNoFit = "codebook does not fit in 160 KB of LDS";

struct AssignRow {
  long N;
  int D, K;
  bool sel, dist, split_on;
  const char* why;      // the refusal, or nullptr and:
  bool split;
  int KTp;
  size_t lds;
  long grid;
};
static const AssignRow kAssign[] = {
    // f32 kernel: LDS bytes, tile counts at both sides of 16 / 32 / 64 codes
    {1, 256, 15, false, false, true, nullptr, false, 1, 16592, 1},
    {1, 256, 16, false, false, true, nullptr, false, 1, 16592, 1},
    {1, 256, 64, false, true, true, nullptr, false, 4, 66320, 1},          // the first shape above 64 KiB
    {1, 256, 65, false, false, true, nullptr, false, 8, 132624, 1},
    {1, 256, 128, false, false, true, nullptr, false, 8, 132624, 1},
    {1, 20, 40, true, false, true, nullptr, false, 4, 8976, 1},
    {1, 256, 129, false, false, true, kTooManyCodes, false, 0, 0, 0},
    {1, 512, 128, false, false, true, kNoFit, false, 0, 0, 0},              // 263696 B
    {1, 304, 128, false, false, true, nullptr, false, 8, 157200, 1},        // 19 steps of 16 features: the last that fits
    {1, 308, 128, false, false, true, kNoFit, false, 0, 0, 0},              // 20 steps: 165392 B
    // the prefiltered kernel: 16 < K <= 64, D <= 256, no mask, no distances, the switch on
    {1, 256, 64, false, false, true, nullptr, true, 4, 131632, 1},
    {1, 256, 33, false, false, true, nullptr, true, 4, 131632, 1},
    {1, 256, 32, false, false, true, nullptr, true, 2, 65840, 1},
    {1, 256, 17, false, false, true, nullptr, true, 2, 65840, 1},
    {1, 64, 32, false, false, true, nullptr, true, 2, 41264, 1},
    {1, 256, 16, false, false, true, nullptr, false, 1, 16592, 1},          // K = 16: f32
    {1, 256, 65, false, false, true, nullptr, false, 8, 132624, 1},         // K = 65: f32
    {1, 260, 64, false, false, true, nullptr, false, 4, 70416, 1},          // D = 260: f32
    {1, 256, 64, true, false, true, nullptr, false, 4, 66320, 1},           // a mask: f32
    {1, 256, 64, false, true, true, nullptr, false, 4, 66320, 1},           // distances: f32
    {1, 256, 64, false, false, false, nullptr, false, 4, 66320, 1},         // the switch off: f32
    // grids: one wave per 16 rows, 4 (f32) or 8 (split) waves per workgroup, 8 or 1 workgroups per CU
    {0, 256, 15, false, false, true, nullptr, false, 1, 16592, 1},          // at least one
    {64, 256, 15, false, false, true, nullptr, false, 1, 16592, 1},
    {65, 256, 15, false, false, true, nullptr, false, 1, 16592, 2},
    {131072, 256, 15, false, false, true, nullptr, false, 1, 16592, 2048},
    {200000, 256, 15, false, false, true, nullptr, false, 1, 16592, 2048},
    {131008, 256, 15, false, false, true, nullptr, false, 1, 16592, 2047},
    {3000, 256, 64, false, false, true, nullptr, true, 4, 131632, 24},
    {128, 256, 64, false, false, true, nullptr, true, 4, 131632, 1},
    {129, 256, 64, false, false, true, nullptr, true, 4, 131632, 2},
    {32768, 256, 64, false, false, true, nullptr, true, 4, 131632, 256},
    {200000, 256, 64, false, false, true, nullptr, true, 4, 131632, 256},
};

struct EmaRow {
  long N;
  int D, K;
  bool has_dw;
  VqEmaForm form;
  int KT;
  size_t lds;
  long grid;
  int64_t ws_bytes;
};
static const EmaRow kEma[] = {
    {2048, 256, 64, true, VQ_EMA_MFMA, 4, 66048, 128, 8421376},
    {5000, 256, 15, true, VQ_EMA_MFMA, 1, 16512, 313, 5148224},
    {33, 64, 5, true, VQ_EMA_MFMA, 1, 4224, 3, 12480},
    {17, 64, 20, true, VQ_EMA_MFMA, 2, 8448, 2, 16640},
    {1, 64, 40, true, VQ_EMA_MFMA, 4, 16896, 1, 16640},
    {1000000, 64, 32, true, VQ_EMA_MFMA, 2, 8448, 512, 4259840},            // two workgroups per CU up to 32 codes ...
    {1000000, 64, 33, true, VQ_EMA_MFMA, 4, 16896, 256, 4259840},           // ... one beyond
    {500, 20, 40, true, VQ_EMA_TWO_PASS, 0, 13440, 8, 107520},
    {1, 20, 40, true, VQ_EMA_TWO_PASS, 0, 13440, 1, 13440},
    {1000000, 64, 65, true, VQ_EMA_ATOMIC, 0, 16900, 1024, 0},              // K = 65, K * D = 4160: neither workspace form
    {1000000, 60, 64, true, VQ_EMA_TWO_PASS, 0, 62464, 512, 31981568},      // D = 60: no matrix pipe; K * D = 3840 <= 4096
    {1000000, 64, 64, true, VQ_EMA_MFMA, 4, 16896, 256, 4259840},           // D = 64, K = 64: the matrix pipe's last
    {1000000, 320, 12, true, VQ_EMA_TWO_PASS, 0, 61632, 512, 31555584},     // D = 320 > 256: no matrix pipe; K * D = 3840
    {1000000, 1024, 4, true, VQ_EMA_TWO_PASS, 0, 65600, 512, 33587200},     // K * D = 4096: the two-pass form's last, two per CU
    {1000000, 1028, 4, true, VQ_EMA_ATOMIC, 0, 16464, 1024, 0},             // K * D = 4112
    {333, 252, 64, true, VQ_EMA_ATOMIC, 0, 64768, 6, 0},
    {500, 22, 40, true, VQ_EMA_ATOMIC, 0, 3680, 8, 0},                      // D % 4 != 0 (the entry point then refuses it)
    {0, 256, 64, true, VQ_EMA_ATOMIC, 0, 65792, 1, 0},                      // no rows: the outputs are zeroed, nothing runs
    {1, 256, 64, false, VQ_EMA_COUNTS, 0, 256, 1, 0},
    {4097, 256, 64, false, VQ_EMA_COUNTS, 0, 256, 2, 0},
    {100000000, 20, 5, false, VQ_EMA_COUNTS, 0, 20, 1024, 0},
};

int main() {
  for (size_t i = 0; i < sizeof(kAssign) / sizeof(kAssign[0]); ++i) {
    const AssignRow& r = kAssign[i];
    VqAssign p;
    memset(&p, 0, sizeof(p));
    const char* why = vq_assign_plan(r.N, r.D, r.K, r.sel, r.dist, r.split_on, &p);
    if (r.why != nullptr) {
      expect(why != nullptr && strcmp(why, r.why) == 0, "assign refusal", (int)i);
      continue;
    }
    expect(why == nullptr && p.split == r.split && p.KTp == r.KTp && p.lds == r.lds && p.grid.count(CUS) == r.grid &&
               p.threads == (r.split ? 512 : 256) && p.D16 == (r.D + 15) / 16 &&
               vq_split_ok(r.D, r.K, r.sel, r.dist, r.split_on) == r.split,
           "assign plan", (int)i);
  }
  for (size_t i = 0; i < sizeof(kEma) / sizeof(kEma[0]); ++i) {
    const EmaRow& r = kEma[i];
    const VqEma e = vq_ema_plan(r.N, r.D, r.K, r.has_dw);
    expect(e.form == r.form && e.KT == r.KT && e.lds == r.lds && e.grid.count(CUS) == r.grid && e.ws_bytes(CUS) == r.ws_bytes, "ema plan", (int)i);
    // what runs when the workspace is missing or too small
    const VqEma a = vq_ema_atomic(r.N, r.D, r.K);
    expect(a.form == VQ_EMA_ATOMIC && a.ws_bytes(CUS) == 0 && a.lds == ((size_t)r.K * r.D + r.K) * 4, "ema fallback", (int)i);
  }
  // the remaining grids: normalise as the f32 assign; the loss one partial per 1024 float4s and VQN_STE_WS_FLOATS at the most
  expect(vq_normalize_grid(200000).count(CUS) == 2048 && vq_normalize_grid(1).count(CUS) == 1, "normalise grid", 0);
  expect(vq_ste_grid(1) == 1 && vq_ste_grid(1024) == 1 && vq_ste_grid(1025) == 2 && vq_ste_grid(1024 * 1024) == VQN_STE_WS_FLOATS &&
             vq_ste_grid((long)1 << 40) == VQN_STE_WS_FLOATS && VQN_STE_WS_FLOATS == 1024,
         "loss grid", 0);
  // the per-workgroup loss sums of the fused forms fit VQN_QUANT_WS_FLOATS on this device size; the grid rule itself
  expect(vq_assign_grid((long)1 << 40).count(CUS) + 1 <= VQN_QUANT_WS_FLOATS && vq_assign_grid((long)1 << 40).count(512) + 1 > VQN_QUANT_WS_FLOATS,
         "workspace of the fused forms", 0);
  expect(vqn_grid_rule(0, 8, CUS) == 0 && vqn_grid1_rule(0, 8, CUS) == 1 && vqn_grid_rule(2049, 8, CUS) == 2048 && vqn_grid_rule(7, 8, CUS) == 7, "grid rule", 0);
  expect(vqn_grid_in_scratch(256, 0, 0) == 256 && vqn_grid_in_scratch(256, 1024, 256 * 1024) == 256 && vqn_grid_in_scratch(256, 1024, 256 * 1024 - 1) == 255 &&
             vqn_grid_in_scratch(256, 1024, 1023) == 0,
         "scratch limit", 0);
  if (failures) return 1;
  printf("vq plan ok: %d rows\n", rows);
  return 0;
}
