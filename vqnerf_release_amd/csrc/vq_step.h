// What the two statements of the VQ step share: vq_assign_kernel (vq.hip: rows from HBM, codebook fragments in LDS, general D) and
// vq_tail (mlp_chain.hip: rows from the LDS image of the fused front, fragments from global memory, D = 256).  The plain-C
// statement of the order of operations is oracle/vq_strict.c.  Only the pieces that leave every instantiation's registers as they
// were are here.  The normalisation, the K step, the best-of-codes update, the 16-lane argmin, the row-code pick, the
// straight-through chain, the group tree and the epilogue were shared as well and taken back: each of them, as a function, moves
// SGPR spills of some vq_assign_kernel<KT, MAXONLY, FUSE = true> (DESIGN, "Where to look", has the pairs), and no benchmark leg times
// those forms.  tests/test_gpu_decomp.py::test_fused_front_is_bit_identical_to_the_separate_launches keeps the twins together.
// Not a public header.
#pragma once
#include "common.h"

// a row's four quarter sums (lane (col, q) holds quarter q of row col): (s0 + s1) + (s2 + s3)
__device__ __forceinline__ float vq_sum_quarters(float s) {
  s = s + __shfl_xor(s, 16);
  s = s + __shfl_xor(s, 32);
  return s;
}

// dist = (|x|^2 - 2 x.c) + |c|^2
__device__ __forceinline__ float vq_dist(const float x2, const float dot, const float c2) {
  const float t1 = x2 - 2.0f * dot;
  return t1 + c2;
}
