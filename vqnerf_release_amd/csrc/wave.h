// Wave64 primitives shared by the kernels (device only).  Summation order is part of every float result, so only ONE order lives
// here: the full-wave xor tree from 32 down to 1.  A kernel that sums in another order (the ascending trees of decomp_loss.hip and
// vq.hip, the 16-lane and DPP reductions, the partial trees of brdf_shade.hip, wgrad.hip, the suffix scan of neus_rays.hip) keeps
// its own loop next to the code that depends on it.
#pragma once
#include <hip/hip_runtime.h>

// the sum over the 64 lanes, in every lane: v += shfl_xor(v, m) for m = 32, 16, ..., 1
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// -> the sum of v over the lanes below this one; *total: over all 64
__device__ __forceinline__ int wave_exclusive_sum(const int v, const int lane, int* total) {
  int s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(s, d, 64);
    if (lane >= d) s += t;
  }
  *total = __shfl(s, 63, 64);
  return s - v;
}

// Adds `cnt` to table[key] for every lane with `has`, equal keys of the wave merged first: the first pending lane's key is broadcast, a
// ballot finds the lanes that hold it, their counts are added (popcount x count when they agree, else a butterfly), the leader adds the
// sum; repeated while a round absorbed MIN_MERGE lanes or more, the rest add for themselves.  Called by all 64 lanes together.
template <int MIN_MERGE>
__device__ __forceinline__ void wave_add(unsigned* table, bool has, const int key, const unsigned cnt, const int lane) {
  unsigned long long pending = __ballot(has);
  while (pending) {                                                          // wave-uniform
    const int leader = __ffsll((long long)pending) - 1;
    const int k = __builtin_amdgcn_readlane(key, leader);
    const unsigned c0 = (unsigned)__builtin_amdgcn_readlane((int)cnt, leader);
    const bool mine = has && key == k;
    const unsigned long long same = __ballot(mine);
    const int m = __popcll(same);
    const unsigned total = __ballot(mine && cnt != c0) == 0 ? c0 * (unsigned)m : wave_sum(mine ? cnt : 0u);
    if (lane == leader) atomicAdd(&table[k], total);
    has = has && !mine;
    pending &= ~same;
    if (m < MIN_MERGE) break;
  }
  if (has) atomicAdd(&table[key], cnt);
}
