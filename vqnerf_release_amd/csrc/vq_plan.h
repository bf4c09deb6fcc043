// Every decision of the VQ host side (csrc/vq.hip) as pure functions of the shapes: tiling, LDS bytes, which kernel runs, the grids and
// the form of the EMA statistics.  Host only, plain C++ (tests/native/vq_plan_host.cpp builds it without HIP: the CU count is a
// parameter).  Not a public header.
#pragma once
#include "launch.h"
#include "vqnerf_hip.h"

constexpr size_t VQ_LDS_MAX = 160 * 1024;

// a persistent grid: `units` of work, at most `per_cu` workgroups per CU, at least one workgroup
struct VqGrid {
  long units;
  int per_cu;
  long count(const int cus) const { return vqn_grid1_rule(units, per_cu, cus); }
};

// ---- nearest-code assignment (vqn_vq_assign, vqn_vq_quantize_rows*) ----
// LDS of the f32 kernel: the codebook's B fragments, |c|^2, the mask and the histogram per code, four wave sums
static inline size_t vq_assign_lds(const int KTp, const int D16) { return ((size_t)KTp * D16 * 256 + 3 * KTp * 16 + 4) * sizeof(float); }
// ... and of the prefiltered (split) kernel
static inline size_t vq_split_lds(const int KTp, const int D16) {
  return (size_t)KTp * D16 * 1024 + (size_t)2 * KTp * 8 * 1024 + ((size_t)2 * KTp * 16 + 4 + 8) * sizeof(float);
}

// one wave owns 16 rows; the f32 kernel has 4 waves and up to 8 workgroups per CU, the split kernel 8 waves and one workgroup per CU.
// The grid is also the number of per-workgroup loss sums of the fused forms (VQN_QUANT_WS_FLOATS holds them and one float more).
static inline VqGrid vq_assign_grid(const long N) { return {(((N + 15) >> 4) + 3) / 4, 8}; }
static inline VqGrid vq_split_grid(const long N) { return {(((N + 15) >> 4) + 7) / 8, 1}; }
static inline VqGrid vq_normalize_grid(const long N) { return vq_assign_grid(N); }

// The prefiltered kernel serves 16 < K <= 64 and D <= 256 without a code-dropout mask or a distance output, where `split_on` (the
// VQN_VQ_SPLIT switch) allows it.
static inline bool vq_split_ok(const int D, const int K, const bool has_sel, const bool has_dist, const bool split_on) {
  return split_on && K > 16 && K <= 64 && D <= 256 && !has_sel && !has_dist;
}

struct VqAssign {
  bool split;        // the prefiltered kernel (vq_assign_split_kernel), else the f32 kernel (vq_assign_kernel)
  int KTp, D16;      // code tiles of 16 the kernel is compiled for (1, 2, 4, 8; the split kernel 2, 4), 16-feature steps
  size_t lds;
  int threads;
  VqGrid grid;
};

// nullptr and *p, or the reason the shape is refused
static inline const char* vq_assign_plan(const long N, const int D, const int K, const bool has_sel, const bool has_dist, const bool split_on,
                                         VqAssign* p) {
  const int KT = (K + 15) / 16;
  if (KT > 8) return "K <= 128";
  p->KTp = KT <= 1 ? 1 : KT <= 2 ? 2 : KT <= 4 ? 4 : 8;
  p->D16 = (D + 15) / 16;
  if (vq_assign_lds(p->KTp, p->D16) > VQ_LDS_MAX) return "codebook does not fit in 160 KB of LDS";
  p->split = vq_split_ok(D, K, has_sel, has_dist, split_on);
  p->lds = p->split ? vq_split_lds(p->KTp, p->D16) : vq_assign_lds(p->KTp, p->D16);
  if (p->lds > VQ_LDS_MAX) return "codebook does not fit in 160 KB of LDS";
  p->threads = p->split ? 512 : 256;
  p->grid = p->split ? vq_split_grid(N) : vq_assign_grid(N);
  return nullptr;
}

// ---- EMA statistics (vqn_vq_ema_stats, vqn_vq_ema_stats_ws_bytes) ----
enum VqEmaForm {
  VQ_EMA_COUNTS,       // dw == NULL: code usage only
  VQ_EMA_MFMA,         // x^T @ onehot on the matrix pipe, per-workgroup partials in `ws`, then a reduction
  VQ_EMA_TWO_PASS,     // small K * D: per-wave partials in `ws`, then a reduction
  VQ_EMA_ATOMIC,       // single pass, LDS atomics; needs no workspace
};

struct VqEma {
  VqEmaForm form;
  int KT;                  // VQ_EMA_MFMA: code tiles the kernel is compiled for (1, 2, 4)
  size_t lds;
  VqGrid grid;
  int64_t ws_per_wg;       // workspace bytes per workgroup
  int64_t ws_bytes(const int cus) const { return grid.count(cus) * ws_per_wg; }
};

// code usage alone: 4096 indices per workgroup, 1024 workgroups at the most (a constant cap: the CU cap of VqGrid never binds)
static inline VqGrid vq_counts_grid(const long N) { return {(N + 4095) / 4096 < 1024 ? (N + 4095) / 4096 : 1024, 1024}; }

// the single-pass form: what runs when the preferred form's workspace is missing or too small
static inline VqEma vq_ema_atomic(const long N, const int D, const int K) {
  return {VQ_EMA_ATOMIC, 0, ((size_t)K * D + K) * sizeof(float), {(N + 63) / 64, 4}, 0};      // >= 16 rows per wave
}

// the form the statistics take given a workspace of ws_bytes(cus)
static inline VqEma vq_ema_plan(const long N, const int D, const int K, const bool has_dw) {
  if (!has_dw) return {VQ_EMA_COUNTS, 0, sizeof(int) * (size_t)K, vq_counts_grid(N), 0};
  if (N > 0 && D > 0 && (D & 63) == 0 && D <= 256 && K > 0 && K <= 64) {
    const int KT = K <= 16 ? 1 : K <= 32 ? 2 : 4, KP = 16 * KT;
    // >= one 4-row step per wave; KT = 4 keeps 256 accumulator registers: one wave per SIMD
    return {VQ_EMA_MFMA, KT, ((size_t)KP * (D + 1) + KP) * sizeof(float), {((N + 3) / 4 + 3) / 4, KT == 4 ? 1 : 2},
            ((int64_t)KP * D + KP) * (int64_t)sizeof(float)};
  }
  if (N <= 0 || D <= 0 || K <= 0 || (long)K * D > 4096 || (D & 3)) return vq_ema_atomic(N, D, K);
  const size_t lds = (size_t)4 * (K * D + K) * sizeof(float);
  return {VQ_EMA_TWO_PASS, 0, lds, {(N + 63) / 64, lds * 2 <= VQ_LDS_MAX ? 2 : 1}, 4 * (int64_t)(K * D + K) * (int64_t)sizeof(float)};
}

// ---- straight-through loss (vqn_vq_ste_loss): one partial per workgroup of 1024 float4s, VQN_STE_WS_FLOATS at the most ----
static inline long vq_ste_grid(const long n4) { return (n4 + 1023) / 1024 < VQN_STE_WS_FLOATS ? (n4 + 1023) / 1024 : VQN_STE_WS_FLOATS; }
