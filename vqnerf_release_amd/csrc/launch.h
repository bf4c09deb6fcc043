// How every host side sizes a persistent grid and launches a kernel: one grid rule, one launch, one dispatch of a runtime int to a
// template argument.  Host only, not a public header.  The rule itself needs no HIP (csrc/vq_plan.h and its stand-alone test state
// grids with the CU count as a parameter); what does stands below __HIPCC__ and is included after common.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

// as many workgroups as there are `units` of work, at most `per_cu` on each of the `cus` compute units
static inline long vqn_grid_rule(const long units, const long per_cu, const long cus) { return units < cus * per_cu ? units : cus * per_cu; }
// ... and at least one (the kernels whose workgroups write a partial or zero an output even when there are no rows)
static inline long vqn_grid1_rule(const long units, const long per_cu, const long cus) {
  const long g = vqn_grid_rule(units, per_cu, cus);
  return g < 1 ? 1 : g;
}

// no more workgroups than `scratch_bytes` holds at `bytes_per_wg` each (0: the kernel keeps none).  0 = not even one: the caller refuses
static inline long vqn_grid_in_scratch(const long grid, const int64_t bytes_per_wg, const int64_t scratch_bytes) {
  // (bytes_per_wg == 0 makes the comparison false, so the division never sees a zero divisor)
  return (int64_t)grid * bytes_per_wg > scratch_bytes ? (long)(scratch_bytes / bytes_per_wg) : grid;
}

#ifdef __HIPCC__
#include <type_traits>

// the rule on this device
static inline long vqn_grid(const long units, const int per_cu) { return vqn_grid_rule(units, per_cu, vqn_num_cus()); }
static inline long vqn_grid1(const long units, const int per_cu) { return vqn_grid1_rule(units, per_cu, vqn_num_cus()); }
// every unit gets a workgroup of its own at `per_cu` per CU (the cap does not bind)
static inline bool vqn_fits_cus(const long units, const int per_cu) { return vqn_grid(units, per_cu) == units; }

// a persistent launch of 4- or 8-wave workgroups over 32-point tiles (the chain kernels, the tile-program interpreter): two 4-wave
// workgroups per CU where the LDS holds two, else one
static inline long vqn_tile_grid(const int n_waves, const size_t lds, const long n_tiles) {
  return vqn_grid(n_tiles, (n_waves == 4 && 2 * lds <= 160 * 1024) ? 2 : 1);
}

// Launch `kernel` with `lds` bytes of dynamic LDS: beyond the 64 KiB a kernel gets unasked its limit is raised first.  Errors report
// under the entry point's name `fn`; a HIP error names this header as its location.
template <class Kernel, class... Args>
static int vqn_launch(const char* fn, const Kernel kernel, const dim3 grid, const int threads, const size_t lds, void* stream, const Args... args) {
  if (lds > 64 * 1024) VQN_HIP_IN(fn, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, (hipStream_t)stream, args...);
  VQN_HIP_IN(fn, hipGetLastError());
  return VQN_OK;
}

// A runtime int chooses a template argument out of a short list: f(std::integral_constant<int, V>) for the V that equals `v`, its
// int returned.  A value outside the list is the caller's bug: VQN_ESHAPE under the entry point's name `fn`, nothing runs.
template <int V, int... Rest, class F>
static int vqn_pick(const char* fn, const int v, const F& f) {
  if (v == V) return f(std::integral_constant<int, V>{});
  if constexpr (sizeof...(Rest) > 0) return vqn_pick<Rest...>(fn, v, f);
  vqn_set_error("%s: unsupported shape: no kernel variant is compiled for %d", fn, v);
  return VQN_ESHAPE;
}
#endif
