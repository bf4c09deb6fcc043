// The tile format [point tile][feature tile][32 features][32 points] f32 (csrc/tile_vm.hip) -- what the training kernels leave for each
// other and for the weight-gradient contraction -- as the engines' registers see it: a row quad of an f32 activation image, an
// accumulator tile and a K step of the pair engines, each with its store and (where a backward reads it) its load.  Stores are
// streaming (written once, read by later launches: past the L2-resident packs); loads are plain (streaming `nt` loads -- so that the
// saved tensors, 14 KB per point passing through once, leave the weight packs in L2 -- measured no better: reflectance backward
// 3.18 -> 3.26 ms per 262,144 points).  -DVQN_DIAG_RT_NO_ST / -DVQN_DIAG_RT_NO_LD (timing only, results are wrong) take the stores /
// the loads out.  Not a public header.
#pragma once
#include "common.h"

namespace eng {

// A row quad of an f32 activation image -- lane (p, h), component j = feature 2 (4 rq + j) + h of the tile -- goes out as four
// 256-byte stores (feature rows 8 rq + 2 j and 8 rq + 2 j + 1 are adjacent).
__device__ __forceinline__ void tfmt_store_quad(float* __restrict__ T, const long ptile, const int n_ft, const int ft, const int rq,
                                                const int lane, const f32x4 v) {
#ifdef VQN_DIAG_RT_NO_ST
  asm volatile("" ::"v"(v));
  return;
#endif
  float* base = T + ((ptile * n_ft + ft) * 32 + 8 * rq) * 32 + lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(v[j], base + 64 * j);
}
__device__ __forceinline__ f32x4 tfmt_load_quad(const float* __restrict__ T, const long ptile, const int n_ft, const int ft, const int rq,
                                                const int lane) {
#ifdef VQN_DIAG_RT_NO_LD
  return (f32x4){0.5f, 0.5f, 0.5f, 0.5f} + 0.001f * (float)lane;
#endif
  const float* base = T + ((ptile * n_ft + ft) * 32 + 8 * rq) * 32 + lane;
  return (f32x4){base[0], base[64], base[128], base[192]};
}

// an accumulator tile of the pair engines: register i of lane (p, h) is feature (i & 3) + 8 (i >> 2) + 4 h of the tile
__device__ __forceinline__ void tfmt_store_acc(float* __restrict__ T, const long ptile, const int n_ft, const int ot, const int lane, const float (&v)[16]) {
#ifdef VQN_DIAG_RT_NO_ST
  asm volatile("" ::"v"(v[0]), "v"(v[5]), "v"(v[10]), "v"(v[15]));
  return;
#endif
  float* base = T + ((ptile * n_ft + ot) * 32 + 4 * (lane >> 5)) * 32 + (lane & 31);
#pragma unroll
  for (int i = 0; i < 16; ++i) __builtin_nontemporal_store(v[i], base + ((i & 3) + 8 * (i >> 2)) * 32);
}
__device__ __forceinline__ void tfmt_load_acc(const float* __restrict__ T, const long ptile, const int n_ft, const int ot, const int lane, float (&v)[16]) {
#ifdef VQN_DIAG_RT_NO_LD
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.5f + 0.001f * (float)(lane + i);
  return;
#endif
  const float* base = T + ((ptile * n_ft + ot) * 32 + 4 * (lane >> 5)) * 32 + (lane & 31);
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = base[((i & 3) + 8 * (i >> 2)) * 32];
}

// a K step of an image of the pair engines: slot jj of lane (p, h) is feature 16 sl + 8 (jj >> 2) + 4 h + (jj & 3)
__device__ __forceinline__ void tfmt_store_step(float* __restrict__ T, const long ptile, const int n_ft, const int sl, const int lane, const float (&x)[8]) {
#ifdef VQN_DIAG_RT_NO_ST
  asm volatile("" ::"v"(x[0]), "v"(x[3]), "v"(x[7]));
  return;
#endif
  float* base = T + ((ptile * n_ft + (sl >> 1)) * 32 + 16 * (sl & 1) + 4 * (lane >> 5)) * 32 + (lane & 31);
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) __builtin_nontemporal_store(x[jj], base + (8 * (jj >> 2) + (jj & 3)) * 32);
}

}  // namespace eng
