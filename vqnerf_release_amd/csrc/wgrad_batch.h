// What the entry points of the weight-gradient contraction share (vqn_wgrad_partials, csrc/wgrad.hip; vqn_wgrad_partials_x3 and
// vqn_wgrad_partials_batched, csrc/wgrad_x3.hip): the check of one problem, the rule that picks its kernel, and the problem table of
// the batched launches -- blockIdx.y picks the problem, blockIdx.x / gridDim.x keep their meaning (the split over point tiles), so
// the kernel bodies are the single-problem ones.
#pragma once
#include "common.h"

constexpr int WG_MAX = 24;
struct WgProblem {
  const float* A; const float* B; float* ws; float* rs;
  int a_tiles, a_t0, a_nt, b_tiles, b_t0, b_nt;
};
struct WgTable { WgProblem p[WG_MAX]; };

// Small blocks (a_nt <= 4: at most 128 output features) at the reference batch (64 point tiles) are latency-, not matrix-bound: the
// f32 kernels with their deeper rings -- no difference measured there (6.50 vs 6.52 ms per 2048-point step).  From this many point
// tiles on they take the x3 kernel too: 262,144-point reflectance step 22.9 -> 22.0 ms (A / B / A on one box).
constexpr long WG_X3_SMALL_FROM = 1024;

// The kernel class of a problem.  0..2, the f32-input kernels by shape: a_nt <= 4 and b_nt <= 4; a_nt <= 4; the rest.  3..5, the
// exact-split LDS kernel: full (8 x 8 tiles, no guards); guarded; guarded with at most four A tiles (narrow: one output tile per wave,
// two workgroups per CU -- batched launches only; the single-problem x3 entry runs the guarded kernel for it).
static inline int wgrad_class(const int a_nt, const int b_nt, const int x3, const long n_point_tiles) {
  if (!x3 || (a_nt <= 4 && n_point_tiles < WG_X3_SMALL_FROM)) return (a_nt <= 4 && b_nt <= 4) ? 0 : (a_nt <= 4 ? 1 : 2);
  return (a_nt == 8 && b_nt == 8) ? 3 : (a_nt <= 4 ? 5 : 4);
}

// one problem's arguments; `in_batch` words the messages for a problem of a batched call
static inline int wgrad_check_problem(const char* fn, const bool in_batch, const float* A, const int a_tiles, const int a_t0, const int a_nt,
                                      const float* B, const int b_tiles, const int b_t0, const int b_nt, const int64_t n_point_tiles,
                                      const int n_split, const float* ws) {
  VQN_CHECK_ARG_IN(fn, A && B && ws, in_batch ? "null pointer in problem" : "null pointer");
  VQN_CHECK_ARG_IN(fn, n_point_tiles >= 1 && n_split >= 1, "n_point_tiles >= 1, n_split >= 1");
  VQN_CHECK_SHAPE_IN(fn, a_nt >= 1 && a_nt <= 8 && b_nt >= 1 && b_nt <= 8,
                     in_batch ? "1..8 feature tiles per operand and problem" : "1..8 feature tiles per operand and call");
  VQN_CHECK_SHAPE_IN(fn, a_t0 >= 0 && a_t0 + a_nt <= a_tiles && b_t0 >= 0 && b_t0 + b_nt <= b_tiles, "feature-tile range outside the tensor");
  VQN_CHECK_SHAPE_IN(fn, ((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0, "operands must be 16-byte aligned");
  return VQN_OK;
}

// the f32-input kernels (csrc/wgrad.hip): vqn_wgrad_partials itself / their launch for `count` problems of one class 0..2
int vqn_wgrad_partials_f32_internal(const float* A, int a_tiles, int a_t0, int a_nt, const float* B, int b_tiles, int b_t0, int b_nt,
                                    int64_t n_point_tiles, int n_split, float* ws, float* rowsum_ws, void* stream);
int vqn_wgrad_f32_batched_internal(const WgProblem* probs, int count, int cls, long n_point_tiles, long grid, void* stream);
