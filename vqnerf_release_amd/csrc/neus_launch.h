// Host side of the entry points of the fused NeuS kernels -- the point kernels (neus_mlp.hip, neus_mlp_f16s.hip, neus_mlp_x3.hip) and
// the backward (neus_train_bwd.hip, neus_train_bwd_x3.hip): descriptors, argument checks, grid sizing, launch.  Not a public header.
#pragma once
#include "neus_phases.h"
#include "launch.h"
#include <stdio.h>

// The checks report under the entry point's own name (`fn`), so that an argument or shape message reads as it would from the entry
// point itself; a HIP error names launch.h as its location.

// the sdf form (vqn_neus_sdf_points*): on VQN_OK with P > 0, *sd holds the checked descriptor; P == 0 is VQN_OK with nothing to do
static int neus_sdf_args(const char* fn, const int32_t* sdf_desc, const float* wbuf_sdf, const float* rays_o, const float* rays_d,
                         const float* z, const float* pts, const int64_t P, const int S, const float* out_sdf,
                         int (*check_desc)(const SdfDesc&), const char* desc_msg, SdfDesc* sd) {
  VQN_CHECK_ARG_IN(fn, sdf_desc && wbuf_sdf && out_sdf, "sdf_desc, wbuf_sdf, out_sdf must be non-null");
  VQN_CHECK_ARG_IN(fn, P >= 0, "P >= 0");
  if (P == 0) return VQN_OK;
  VQN_CHECK_ARG_IN(fn, pts != nullptr || (rays_o && rays_d && z && S > 0), "either pts or (rays_o, rays_d, z, S) required");
  memcpy(sd, sdf_desc, sizeof(SdfDesc));
  VQN_CHECK_SHAPE_IN(fn, check_desc(*sd) == 0, desc_msg);
  return VQN_OK;
}

// the fine form (vqn_neus_fine_points*); extras_rows_ok is the engine's rule for ColDesc::extra_rows
static int neus_fine_args(const char* fn, const int32_t* sdf_desc, const float* wbuf_sdf, const int32_t* col_desc, const float* wbuf_col,
                          const float* rays_o, const float* rays_d, const float* z, const float* pts, const float* dirs, const int64_t P,
                          const int S, const void* scratch, const float* out_sdf, const float* out_grad, const float* out_rgb,
                          int (*check_desc)(const SdfDesc&), const char* desc_msg, bool (*extras_rows_ok)(const ColDesc&),
                          SdfDesc* sd, ColDesc* cd) {
  VQN_CHECK_ARG_IN(fn, sdf_desc && wbuf_sdf && col_desc && wbuf_col, "descriptors and weight packs must be non-null");
  VQN_CHECK_ARG_IN(fn, out_sdf && out_grad && scratch, "out_sdf, out_grad and scratch must be non-null");
  VQN_CHECK_ARG_IN(fn, P >= 0, "P >= 0");
  if (P == 0) return VQN_OK;
  VQN_CHECK_ARG_IN(fn, (pts != nullptr && dirs != nullptr) || (rays_o && rays_d && z && S > 0),
                   "either (pts, dirs) or (rays_o, rays_d, z, S) required");
  memcpy(sd, sdf_desc, sizeof(SdfDesc));
  memcpy(cd, col_desc, sizeof(ColDesc));
  VQN_CHECK_SHAPE_IN(fn, check_desc(*sd) == 0, desc_msg);
  if (cd->n_lin != 0) {
    VQN_CHECK_ARG_IN(fn, out_rgb != nullptr, "out_rgb must be non-null when a colour net is given");
    VQN_CHECK_SHAPE_IN(fn, sd->layers[sd->n_lin - 1].n_out_tiles >= 1, "SDF network has no feature outputs (d_out == 1)");
    VQN_CHECK_SHAPE_IN(fn, cd->n_lin >= 2 && cd->n_lin <= VQN_MAX_COL_LAYERS && cd->d_out == 3, "colour net: 2..8 layers, d_out == 3");
    VQN_CHECK_SHAPE_IN(fn, cd->extra_feats >= 3 && cd->extra_feats <= 64 && extras_rows_ok(*cd), "colour net extras");
    for (int l = 0; l < cd->n_lin - 1; ++l)
      VQN_CHECK_SHAPE_IN(fn, cd->layers[l].n_out_tiles >= 1 && cd->layers[l].n_out_tiles <= sd->max_tiles, "colour layer wider than max_tiles");
  }
  return VQN_OK;
}

// the saved tensors of a training forward, in the order of its `tensors` argument: [E, OUTF, EXTR, U_1..U_nL, GH_0..GH_{nL-1}, C_1..C_nC]
static eng::TrainOut neus_train_out(float* const* tensors, const int nL, const int nC, const int e_tiles, const int outf_tiles, const int extr_tiles) {
  eng::TrainOut to;
  memset(&to, 0, sizeof(to));
  to.E = tensors[0]; to.OUTF = tensors[1]; to.EXTR = tensors[2];
  for (int l = 1; l <= nL; ++l) to.U[l] = tensors[3 + (l - 1)];
  for (int l = 0; l < nL; ++l) to.GH[l] = tensors[3 + nL + l];
  for (int l = 1; l <= nC; ++l) to.C[l] = tensors[3 + 2 * nL + (l - 1)];
  to.e_tiles = e_tiles; to.outf_tiles = outf_tiles; to.extr_tiles = extr_tiles;
  return to;
}

// bytes of activation stash one image needs (the fine forms; see vqn_neus_fine_scratch_bytes)
static int64_t neus_stash_bytes(const SdfDesc& sd) { return (int64_t)(sd.n_lin - 1) * 4 * sd.max_tiles * 1024; }

// Workgroups of a persistent launch over groups of `images` tiles: as many as stay resident (`per_cu` on each CU: one 512-thread
// multi-image workgroup, two 256-thread ping-pong one-image ones, two to four in-place one-image ones), no more than there are groups,
// and no more than `scratch_bytes` holds stashes of `per_img` bytes per image (per_img == 0: the kernel keeps no stash).  0 = the
// scratch holds not even one workgroup's.
static long pair_grid(const long n_tiles, const int images, const int per_cu, const int64_t per_img, const int64_t scratch_bytes) {
  return vqn_grid_in_scratch(vqn_grid((n_tiles + images - 1) / images, per_cu), images * per_img, scratch_bytes);
}

// ---- the backward (vqn_neus_train_bwd, vqn_neus_train_bwd_x3): one pass, two engines.  What differs between them stays in their files:
// the kernel, its LDS size and the engine's own descriptor rules (`engine_rules`: max_tiles, the embedding rows, the call count).
constexpr int TB_MAX_L = 12;

struct TrainBwdDesc {        // int32 words, filled by the host (geo/train_programs.py: NeusTrainEngine._bwd_static)
  int nL, nC, skip, emb_rows, emb_feats, e_tiles, max_tiles, feat_tiles;     // emb_rows: rows of the engine's image (x3: 3 per 16 features)
  int outf_tiles, squeeze, offBtop, offWrow, offCBfeat, offCBnrm;            // offsets: float4 units into the engine's pack(s)
  float scale, inv_scale;
  int ts[TB_MAX_L];          // feature tiles of SDF hidden layer l's output
  int tc[TB_MAX_L];          // feature tiles of colour hidden layer l's output
  int offT[TB_MAX_L];        // W_l (K = [u_{l-1} (, e)])
  int offB[TB_MAX_L];        // W_l[:, :out_{l-1}]^T, l = 1..nL-1
  int offCB[TB_MAX_L];       // Wc_l^T, l = 1..nC (l = nC: K = one row)
};
constexpr int TB_DESC_INTS = 16 + 5 * TB_MAX_L;
static_assert(sizeof(TrainBwdDesc) == TB_DESC_INTS * 4, "descriptor layout");

struct TrainBwdPtrs {
  const float* X; const float* G_RGB; const float* RGB; const float* G_N; const float* G_SDF;
  const float* U[TB_MAX_L];    // U[l], l = 1..nL: output of SDF layer l - 1
  const float* GH[TB_MAX_L];   // GH[l], l = 0..nL-1
  const float* C[TB_MAX_L];    // C[l], l = 1..nC: output of colour layer l - 1
  float* DC[TB_MAX_L];         // DC[l], l = 0..nC
  float* UD[TB_MAX_L];         // UD[l], l = 1..nL
  float* AB[TB_MAX_L];         // AB[l], l = 0..nL-1
  float* GOUTF; float* ED;
};

// 0 = a descriptor the engine takes
static int train_bwd_load_desc(const int32_t* desc, int (*engine_rules)(const TrainBwdDesc&), TrainBwdDesc* bd) {
  memcpy(bd, desc, sizeof(TrainBwdDesc));
  if (bd->nL < 2 || bd->nL >= TB_MAX_L || bd->nC < 1 || bd->nC >= TB_MAX_L) return 1;
  if (engine_rules(*bd) != 0) return 2;
  if (bd->skip == 0 || bd->skip >= bd->nL) return 4;
  if (bd->feat_tiles < 1 || bd->feat_tiles > bd->max_tiles || bd->outf_tiles < bd->feat_tiles) return 5;      // (GOUTF stores are bounded by outf_tiles)
  for (int l = 0; l < bd->nL; ++l) if (bd->ts[l] < 1 || bd->ts[l] > bd->max_tiles) return 6;
  for (int l = 0; l < bd->nC; ++l) if (bd->tc[l] < 1 || bd->tc[l] > bd->max_tiles) return 7;
  if (!(bd->scale > 0.f)) return 8;
  return 0;
}

// bytes of stash one image needs: S_0..S_{nL-1} and g_feat, accumulator-order quads
static int64_t train_bwd_stash_bytes(const TrainBwdDesc& bd) { return (int64_t)(bd.nL + 1) * 4 * bd.max_tiles * 1024; }

// the _scratch_bytes queries: room for every resident workgroup's two images, -1 for a descriptor the engine refuses
static int64_t train_bwd_scratch_bytes(const int32_t* desc, int (*engine_rules)(const TrainBwdDesc&)) {
  TrainBwdDesc bd;
  if (!desc || train_bwd_load_desc(desc, engine_rules, &bd) != 0) return -1;
  return (int64_t)vqn_num_cus() * 2 * train_bwd_stash_bytes(bd);
}

// Every refusal of the two entry points, before anything touches the device.  w0 / w1: the engine's weight buffer(s).  On VQN_OK
// *bd holds the checked descriptor, *tp the tensors of `saved` = [U_1..U_nL, GH_0..GH_{nL-1}, C_1..C_nC] and `outs` = [DC_0..DC_nC,
// GOUTF, ED, UD_1..UD_nL, AB_0..AB_{nL-1}], *grid the workgroups to launch.
static int train_bwd_args(const char* fn, const int32_t* desc, const void* w0, const void* w1, const float* pts, const float* g_rgb,
                          const float* rgb, const float* g_n, const float* g_sdf, const int64_t P, const void* scratch,
                          const int64_t scratch_bytes, const float* const* saved, const int n_saved, float* const* outs, const int n_outs,
                          int (*engine_rules)(const TrainBwdDesc&), const char* desc_msg, TrainBwdDesc* bd, TrainBwdPtrs* tp, long* grid) {
  VQN_CHECK_ARG_IN(fn, desc && w0 && w1 && pts && g_rgb && scratch && saved && outs, "null pointer");
  VQN_CHECK_ARG_IN(fn, P >= 1, "P >= 1");
  VQN_CHECK_SHAPE_IN(fn, train_bwd_load_desc(desc, engine_rules, bd) == 0, desc_msg);
  const int nL = bd->nL, nC = bd->nC;
  VQN_CHECK_ARG_IN(fn, n_saved == 2 * nL + nC, "saved: [U_1..U_nL, GH_0..GH_{nL-1}, C_1..C_nC]");
  VQN_CHECK_ARG_IN(fn, n_outs == (nC + 1) + 2 + 2 * nL, "outs: [DC_0..DC_nC, GOUTF, ED, UD_1..UD_nL, AB_0..AB_{nL-1}]");
  VQN_CHECK_ARG_IN(fn, (rgb != nullptr) == (bd->squeeze != 0), "rgb: the forward's colours when the colour net ends in a sigmoid, else NULL");
  for (int i = 0; i < n_saved; ++i) VQN_CHECK_ARG_IN(fn, saved[i] != nullptr, "null saved tensor");
  for (int i = 0; i < n_outs; ++i) VQN_CHECK_ARG_IN(fn, outs[i] != nullptr, "null output tensor");
  const int64_t per_img = train_bwd_stash_bytes(*bd);
  char scratch_msg[96];
  snprintf(scratch_msg, sizeof(scratch_msg), "scratch too small (see %s_scratch_bytes)", fn);
  VQN_CHECK_ARG_IN(fn, scratch_bytes >= 2 * per_img, scratch_msg);      // (not even one workgroup's: pair_grid would say 0)
  memset(tp, 0, sizeof(*tp));
  tp->X = pts; tp->G_RGB = g_rgb; tp->RGB = rgb; tp->G_N = g_n; tp->G_SDF = g_sdf;
  for (int l = 1; l <= nL; ++l) tp->U[l] = saved[l - 1];
  for (int l = 0; l < nL; ++l) tp->GH[l] = saved[nL + l];
  for (int l = 1; l <= nC; ++l) tp->C[l] = saved[2 * nL + l - 1];
  for (int l = 0; l <= nC; ++l) tp->DC[l] = outs[l];
  tp->GOUTF = outs[nC + 1];
  tp->ED = outs[nC + 2];
  for (int l = 1; l <= nL; ++l) tp->UD[l] = outs[nC + 3 + l - 1];
  for (int l = 0; l < nL; ++l) tp->AB[l] = outs[nC + 3 + nL + l];
  *grid = pair_grid((P + 31) / 32, 2, 1, per_img, scratch_bytes);
  return VQN_OK;
}
