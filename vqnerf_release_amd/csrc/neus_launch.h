// Host side of the entry points of the fused NeuS point kernels (neus_mlp.hip, neus_mlp_f16s.hip, neus_mlp_x3.hip): argument checks,
// grid sizing, launch.  Not a public header.
#pragma once
#include "neus_phases.h"

// The checks report under the entry point's own name (`fn`), so that an argument or shape message reads as it would from the entry
// point itself; a HIP error names this header as its location.

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

// Workgroups of a persistent launch over groups of `images` tiles: as many as stay resident (one 512-thread two-image workgroup per CU,
// two 256-thread one-image ones), no more than there are groups, and no more than `scratch_bytes` holds stashes of `per_img` bytes per
// image (per_img == 0: the kernel keeps no stash).  0 = the scratch holds not even one workgroup's.
static long pair_grid(const long n_tiles, const int images, const int64_t per_img, const int64_t scratch_bytes) {
  long grid = (long)vqn_num_cus() * (images == 1 ? 2 : 1);
  const long groups = (n_tiles + images - 1) / images;
  if (grid > groups) grid = groups;
  // (per_img == 0 makes the comparison false, so the division below never sees a zero divisor)
  if ((int64_t)grid * images * per_img > scratch_bytes) grid = (long)(scratch_bytes / (images * per_img));
  return grid;
}

// launch the kernel with `lds` bytes of dynamic LDS; `opt_in`: raise its limit first (the two-image forms always, the one-image forms
// beyond the 64 KiB a kernel gets unasked)
template <class Kernel, class... Args>
static int neus_launch(const char* fn, const Kernel kernel, const bool opt_in, const long grid, const int threads, const size_t lds, void* stream,
                       const Args... args) {
  if (opt_in) VQN_HIP_IN(fn, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, (hipStream_t)stream, args...);
  VQN_HIP_IN(fn, hipGetLastError());
  return VQN_OK;
}
