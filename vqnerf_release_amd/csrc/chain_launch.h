// Host side of the entry points of the Dense-stack kernels (mlp_chain.hip: vqn_mlp_chain_fwd, vqn_mlp_chain_vq_fwd; mlp_chain_f16s.hip:
// vqn_mlp_chain_fwd_f16s): the descriptor rules, the output-table checks, LDS size, grid sizing, launch.  Not a public header.  The
// descriptor rules need no HIP (tests/native/chain_check_host.cpp compiles them with g++); what does stands below __HIPCC__.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vqn_chain_desc.h"

// per-workgroup images of the <= 4-output layers: the waves' partial dots, [wave][point][output]
struct ChainSmalls {
  float part[8 * 32 * 4];
};

struct OutPtrs {
  float* p[VQN_CHAIN_MAX_OUTS];
  int ld[VQN_CHAIN_MAX_OUTS];
};

// what an engine asks of a program beyond the common rules
struct ChainEngineRules {
  int row_granule;        // LDS rows per K step: every K segment and the input are whole steps (f32: 1; f16 hi / lo row pairs: 2)
  bool in_place;          // the kernel takes layers that write over their own K rows after a barrier (bit 8 of ChainLayer::act)
};
constexpr ChainEngineRules kChainRulesF32 = {1, true};
constexpr ChainEngineRules kChainRulesF16s = {2, false};

// dynamic LDS of one program: its rows, the partial dots, the <= 4-output layers' weight images
static inline size_t chain_lds_bytes(const ChainDesc& d) {
  return (size_t)d.total_rows * 1024 + sizeof(ChainSmalls) + (size_t)d.small_w4 * 16;
}

// 0 = a program the engine takes; otherwise the number of the rule it breaks (reported as "check %d")
static inline int chain_check_desc(const ChainDesc& d, const ChainEngineRules& r) {
  const int g = r.row_granule;
  if (d.n_layers < 1 || d.n_layers > VQN_CHAIN_MAX_LAYERS) return 1;
  if (d.n_waves != 4 && d.n_waves != 8) return 2;
  if (d.total_rows < 1 || d.small_w4 < 0 || chain_lds_bytes(d) > 160 * 1024) return 3;
  if (d.in_rows < g || d.in_rows % g || d.in_row0 < 0 || d.in_row0 + d.in_rows > d.total_rows) return 4;
  if (d.in_mode == 1 && (d.in_feats != 3 + 6 * d.n_freqs || d.n_freqs > 16)) return 5;
  if (d.in_feats < 1 || d.in_feats > 8 * d.in_rows || d.in_stride < 1) return 6;
  for (int l = 0; l < d.n_layers; ++l) {
    const ChainLayer& L = d.layers[l];
    if (L.kind == 2) {
      if (L.dst_row0 < 0 || L.dst_row0 + d.in_rows > d.total_rows) return 20;
      continue;
    }
    if (L.kA_rows < 0 || L.kB_rows < 0 || L.kA_rows + L.kB_rows < g || L.kA_rows % g || L.kB_rows % g) return 10;
    if (L.kA_row0 < 0 || L.kA_row0 + L.kA_rows > d.total_rows) return 11;
    if (L.kB_rows > 0 && (L.kB_row0 < 0 || L.kB_row0 + L.kB_rows > d.total_rows)) return 12;
    if (L.out_slot >= VQN_CHAIN_MAX_OUTS) return 13;
    if (L.kind == 0) {
      if (L.n_out_tiles < 1 || L.dst_row0 < 0 || L.dst_row0 + 4 * L.n_out_tiles > d.total_rows) return 14;
      if (L.out_slot >= 0 && (L.out_feats < 1 || L.out_feats > 32 * L.n_out_tiles)) return 15;
      // a layer must not overwrite its own K rows -- unless it writes after a barrier (bit 8 of act), one tile per wave
      const int d0 = L.dst_row0, d1 = L.dst_row0 + 4 * L.n_out_tiles;
      if (r.in_place && (L.act & 0x100)) {
        if (L.n_out_tiles > d.n_waves) return 22;
      } else {
        if (d0 < L.kA_row0 + L.kA_rows && L.kA_row0 < d1) return 16;
        if (L.kB_rows > 0 && d0 < L.kB_row0 + L.kB_rows && L.kB_row0 < d1) return 17;
      }
    } else if (L.kind == 1) {
      if (L.n_out_tiles < 1 || L.n_out_tiles > 4 || L.out_slot < 0) return 18;
      if (L.dst_row0 < 0 || L.dst_row0 + L.n_out_tiles * (L.kA_rows + L.kB_rows) * 2 > d.small_w4) return 21;
    } else return 19;
  }
  return 0;
}

#ifdef __HIPCC__
#include "common.h"
#include "launch.h"

// The checks report under the entry point's own name (`fn`); a HIP error names launch.h as its location.

// every output a program writes: a pointer (`null_msg` if not: the entry points word it differently), room for the layer's width,
// 16-byte alignment where the kernel stores float4s.  `allow_null_slot0` (program A of the fused front): z may stay on the chip
static int chain_check_outs(const char* fn, const ChainDesc& d, const OutPtrs& o, const bool allow_null_slot0, const char* null_msg) {
  for (int l = 0; l < d.n_layers; ++l) {
    const ChainLayer& L = d.layers[l];
    const int s = L.out_slot;
    if (s < 0) continue;
    if (allow_null_slot0 && s == 0 && o.p[0] == nullptr) continue;
    VQN_CHECK_ARG_IN(fn, o.p[s] != nullptr, null_msg);
    VQN_CHECK_ARG_IN(fn, o.ld[s] >= (L.kind == 0 ? L.out_feats : L.n_out_tiles),
                     "output leading dimension smaller than the layer's width");
    if (L.kind == 0 && (o.ld[s] & 3) == 0)
      VQN_CHECK_ARG_IN(fn, ((uintptr_t)o.p[s] & 15) == 0, "outputs with ld % 4 == 0 must be 16-byte aligned");
  }
  return VQN_OK;
}

// Every refusal of vqn_mlp_chain_fwd / _f16s, before anything touches the device.  On VQN_OK with N > 0, *d holds the checked
// descriptor; N == 0 is VQN_OK with nothing to do.
static int chain_fwd_args(const char* fn, const ChainEngineRules& rules, const int32_t* desc, const float* wbuf, const float* in,
                          const int64_t N, const OutPtrs& o, ChainDesc* d) {
  VQN_CHECK_ARG_IN(fn, desc && wbuf, "desc and wbuf must be non-null");
  VQN_CHECK_ARG_IN(fn, N >= 0, "N >= 0");
  if (N == 0) return VQN_OK;
  VQN_CHECK_ARG_IN(fn, in != nullptr, "in must be non-null");
  memcpy(d, desc, sizeof(ChainDesc));
  const int bad = chain_check_desc(*d, rules);
  if (bad) {
    vqn_set_error("%s: unsupported shape: invalid chain descriptor (check %d)", fn, bad);
    return VQN_ESHAPE;
  }
  const int rc = chain_check_outs(fn, *d, o, false, "an output the descriptor writes is null");
  if (rc != VQN_OK) return rc;
  if (d->in_mode == 0 && (d->in_stride & 3) == 0) VQN_CHECK_ARG_IN(fn, ((uintptr_t)in & 15) == 0, "in must be 16-byte aligned");
  return VQN_OK;
}

// launch an NW-wave kernel over the N points with `lds` bytes of dynamic LDS
template <int NW, class Kernel, class... Args>
static int chain_launch(const char* fn, const Kernel kernel, const size_t lds, const int64_t N, void* stream, const Args... args) {
  return vqn_launch(fn, kernel, vqn_tile_grid(NW, lds, (N + 31) / 32), NW * 64, lds, stream, args...);
}
#endif
