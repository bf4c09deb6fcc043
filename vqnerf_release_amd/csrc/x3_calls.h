// The GEMM-call stream of the training kernels built on the exact-split engine (mlp_prims_x3.h): neus_train_bwd_x3.hip and
// refl_train_x3.hip (neus_mlp_x3.hip, where the scheme began, keeps its own copy: the fine render kernel measured 0.8 % slower on this
// header, see the note there).  Their weights stream through a register ring that runs ahead across layers, so a wave must know, while it is
// still in one GEMM, where its first fragment of the NEXT one lies.  The kernels therefore write the GEMM calls of one unit of work
// (a tile pair) into an LDS table in program order, once per workgroup, and every call looks its successor up there -- past calls in
// which the wave owns no tile, and from the last call of a unit round into the first of the next unit.  Here: the image constants
// these kernels share, the table, the look-up, the ring prime and the two-image call wrappers.  Everything is inlined, and
// descriptor fields and pointers come in one by one (see the note in neus_phases.h on what a reference to a descriptor costs).
// Not a public header.
#pragma once
#include "mlp_prims_x3.h"

namespace eng {
namespace x3 {

constexpr int E0 = 0;         // LDS rows [0, 12) of an image: embedding / colour-net extras / d sdf / d embedding (up to 4 steps = 64 features)
constexpr int E_ROWS = 12;
constexpr int X0 = E_ROWS;    // the activation buffer (6 rows per 32 features; layers run in place)
constexpr int RING = 2;       // blocks of 2 K steps in a wave's weight ring
constexpr int NW = 8;         // waves of a workgroup = most output tiles of a layer in place
constexpr int MAX_CALLS = 40;

// (A kernel keeps the table as a member `calls` of its LDS scalars and hands `&sm->calls` to every call below.  Through a pointer
//  taken once at the kernel's top the compiler addresses the table apart from the scalars around it: three more spilled SGPRs in
//  refl_train_fwd_x3_kernel<2>, one more in <1>.)
struct CallTab {
  int tab[MAX_CALLS * 4];     // GEMM calls of one unit in program order: {float4 offset, weight buffer 0 / 1, K blocks, out tiles}
  int n_calls;
};

// K blocks (2 steps = 6 rows of the pack) of `krows` activation rows
__device__ __forceinline__ int blocks_of(const int krows) { return (krows / 3 + 1) >> 1; }

// call number n (counted by the one thread that builds the table; it stores n_calls = n at the end)
__device__ __forceinline__ void add_call(CallTab* ct, int& n, const int off, const int which, const int krows, const int tiles) {
  ct->tab[4 * n] = off; ct->tab[4 * n + 1] = which; ct->tab[4 * n + 2] = blocks_of(krows); ct->tab[4 * n + 3] = tiles; ++n;
}

// The wave's first weight fragment (nwp) and K block count (nnb) of the next call after `idx`, wrapping into the next unit, in which
// it owns a tile.  own(tiles) = the wave's first tile in a GEMM of `tiles` output tiles; it owns one iff that is below `tiles`.
// w0 / w1: the weight buffers the table's second word selects.  n_calls >= 1 and wave-uniform; without any owned call: a valid dummy.
template <class Own>
__device__ __forceinline__ void next_stream(const CallTab* ct, const int n_calls, const int idx, const f32x4* w0, const f32x4* w1,
                                            const int lane, const Own own, const f32x4*& nwp, int& nnb) {
  nwp = w0 + lane; nnb = 1;
  for (int k = 1; k <= n_calls; ++k) {
    const int m = (idx + k) % n_calls;
    const int tiles = __builtin_amdgcn_readfirstlane(ct->tab[4 * m + 3]);
    const int mine = own(tiles);
    if (mine < tiles) {
      const int off = __builtin_amdgcn_readfirstlane(ct->tab[4 * m]), which = __builtin_amdgcn_readfirstlane(ct->tab[4 * m + 1]);
      nnb = __builtin_amdgcn_readfirstlane(ct->tab[4 * m + 2]);
      nwp = (which ? w1 : w0) + off + (size_t)mine * nnb * 384 + lane;
      return;
    }
  }
}

// the ring before the first unit: the wave's first fragments of the first call in which it owns a tile
template <class Own>
__device__ __forceinline__ void prime_stream(const CallTab* ct, const int n_calls, const f32x4* w0, const f32x4* w1, const int lane,
                                             const Own own, f32x4 (&ring)[RING][6]) {
  const f32x4* wp0; int nb0;
  next_stream(ct, n_calls, n_calls - 1, w0, w1, lane, own, wp0, nb0);
  ring_prime_x3<RING>(ring, wp0, nb0);
}

// Call number `call` (counted here) of the two-image kernels, wave w owning tile w: gemm_tiles_x3_ring2 with the ring refilled towards
// the next call.  COMMIT -- a layer IN PLACE (its output tile `wave` goes over its own input, the X buffer): the accumulators stay where
// the K loop left them, a barrier sees every wave out of its K loop -- the input rows are dead --, then the epilogues write their tiles
// straight over the input (store_tile_x3) and a second barrier publishes them; waves without a tile in this GEMM reach the same two
// barriers from the branch below.  (Round 3's form parked the finished, already split tiles in 48 registers across the barrier: they
// ended in scratch, and every layer re-read 18 x 16 B per lane behind the epilogue's global stores -- round 4, found with in-kernel
// stamps on csrc/refl_train_x3.hip, where the same change took a third off the backward.)
template <int NACC, bool COMMIT, class Init, class Epi>
__device__ __forceinline__ void gemm_call2(const CallTab* ct, const int n_calls, int& call, const f32x4* w0, const f32x4* w1,
                                           const f32x4* lds, const int img_stride, const KSegs ks, const f32x4* wbase, const int tiles,
                                           const int wave, const int lane, f32x4 (&ring)[RING][6], Init init, Epi epi) {
  const f32x4* nwp; int nnb;
  next_stream(ct, n_calls, call, w0, w1, lane, [&](int) { return wave; }, nwp, nnb);
  ++call;
  if constexpr (!COMMIT) gemm_tiles_x3_ring2<NW, RING, NACC>(lds, img_stride, ks, wbase, tiles, wave, lane, ring, nwp, nnb, init, epi);
  else {
    gemm_tiles_x3_ring2<NW, RING, NACC>(lds, img_stride, ks, wbase, tiles, wave, lane, ring, nwp, nnb, init,
                                        [&](int ot, auto im_c, const f32x16& acc) __attribute__((always_inline)) {
          if (decltype(im_c)::value == 0) __syncthreads(); epi(ot, im_c, acc); });
    if (wave >= tiles) __syncthreads();
    __syncthreads();
  }
}

}  // namespace x3
}  // namespace eng
