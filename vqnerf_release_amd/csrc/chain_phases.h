// Device pieces that the two Dense-stack kernels (mlp_chain.hip, mlp_chain_f16s.hip) share: what does not depend on the matrix engine.
// The per-engine halves -- input loads, GEMM epilogues, the row dots of the <= 4-output layers, the weight look-ahead -- stay in their
// files.  Plain inline functions.  Not a public header.
#pragma once
#include "chain_launch.h"
#include "mlp_prims.h"

__device__ __forceinline__ float act_rt(int act, float x) {
  switch (act) {
    case eng::ACT_RELU: return fmaxf(x, 0.f);
    case eng::ACT_SIGMOID: return eng::fast_rcp(1.f + eng::fast_exp(-x));
    case eng::ACT_SOFTPLUS100: return eng::act_fwd<eng::ACT_SOFTPLUS100>(x);
    default: return x;
  }
}

// the <= 4-output layers' weight images are tiny and the same for every point tile: one LDS copy per workgroup (their
// VALU dots would otherwise wait on an L2 round trip per row)
template <int NW>
__device__ __forceinline__ void chain_stage_smalls(const ChainDesc& d, const f32x4* __restrict__ wbuf, f32x4* smallw) {
  const int tid = threadIdx.x;
  for (int l = 0; l < d.n_layers; ++l)
    if (d.layers[l].kind == 1) {
      const int n4 = d.layers[l].n_out_tiles * (d.layers[l].kA_rows + d.layers[l].kB_rows) * 2;
      for (int i = tid; i < n4; i += NW * 64) smallw[d.layers[l].dst_row0 + i] = wbuf[d.layers[l].w_off + i];
    }
}

// A <= 4-output layer after the engine's row dots: s[o] is this lane's share of output o for point p (this wave's rows, this
// half-wave's features).  The two half-waves are joined and every wave's partial sums are left in `sm` for the fixed-order combine.
// h = (tid >> 5) & 1, p = tid & 31 and wave are the caller's own values.  The combine itself (sum in wave order, bias4 by constant
// index, act_rt, store) stays in the two kernels: as a function it costs mlp_chain_vq_kernel<2> and <4> two SGPR spills (86 -> 88).
__device__ __forceinline__ void chain_small_join(float (&s)[4], ChainSmalls* sm, const int h, const int p, const int wave) {
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    s[o] += __shfl_xor(s[o], 32);
    if (h == 0) sm->part[(wave * 32 + p) * 4 + o] = s[o];
  }
  __syncthreads();
}
