// What the fused NeuS point kernels share outside their GEMMs (neus_mlp.hip, neus_mlp_f16s.hip, neus_mlp_x3.hip; the tile-format
// accessors their training forms use are in tfmt.h).  The three engines differ in how an activation image lies in LDS
// and in their GEMM loops, epilogues and weight rings, which stay in their own files; the VALU phases around the GEMMs -- point load,
// sdf output, chain through the embedding, colour-net extras, rgb output -- are the same arithmetic in the same order everywhere and
// live here once, as plain functions of their inputs.  The host side of the entry points is in neus_launch.h.  Not a public header.
#pragma once
#include "mlp_prims.h"
#include "tfmt.h"
#include "vqn_neus_desc.h"

namespace eng {

// per-tile scalars of NIMG 32-point images, after the activation rows (an engine with a call table appends it)
template <int NIMG>
struct Smalls {
  float pts[NIMG][96], dirs[NIMG][96], part[NIMG][512], grad[NIMG][96];
};

// ---- points of a tile: point `pt` (clamped to the last one, so that a ragged or phantom tile computes on valid data) into the
// triples pts3 / dirs3 of its image slot, either given directly or formed from its ray and depth
template <bool FINE>
__device__ __forceinline__ void load_point(long pt, const long P, const int S, const float* __restrict__ rays_o,
                                           const float* __restrict__ rays_d, const float* __restrict__ zv,
                                           const float* __restrict__ pts_direct, const float* __restrict__ dirs_direct,
                                           float* pts3, float* dirs3) {
  if (pt >= P) pt = P - 1;
  float x, y, z, dx = 0.f, dy = 0.f, dz = 0.f;
  if (pts_direct != nullptr) {
    x = pts_direct[pt * 3 + 0]; y = pts_direct[pt * 3 + 1]; z = pts_direct[pt * 3 + 2];
    if (FINE) { dx = dirs_direct[pt * 3 + 0]; dy = dirs_direct[pt * 3 + 1]; dz = dirs_direct[pt * 3 + 2]; }
  } else {
    const long ray = pt / S;
    const float t = zv[pt];
    dx = rays_d[ray * 3 + 0]; dy = rays_d[ray * 3 + 1]; dz = rays_d[ray * 3 + 2];
    // o + d * z with separate mul/add roundings, as the reference's broadcasted expression
    x = rays_o[ray * 3 + 0] + __fmul_rn(dx, t);
    y = rays_o[ray * 3 + 1] + __fmul_rn(dy, t);
    z = rays_o[ray * 3 + 2] + __fmul_rn(dz, t);
  }
  pts3[0] = x; pts3[1] = y; pts3[2] = z;
  dirs3[0] = dx; dirs3[1] = dy; dirs3[2] = dz;
}

// ---- embedding feature f of the scaled point, zero beyond the last feature (the padding of the last K row)
__device__ __forceinline__ float emb_feat(const int f, const int emb_feats, const float xs, const float ys, const float zs) {
  return f < emb_feats ? posenc_feat(f, xs, ys, zs) : 0.f;
}

// (The helpers below take descriptor fields one by one, not `const SdfDesc&` / `const ColDesc&`: a reference to the kernel's by-value
// descriptor argument cost the x3 training forward 40 scalar-register spills, 119 -> 159.)

// ---- sdf output of point t of an image from the four waves' partial row dots: the raw network output (sdf_raw / scale is what the
// caller gets); the bias is in the pack at float4 offset last_b_off if that is > 0, else last_bias
__device__ __forceinline__ float sdf_raw(const float* pr, const int t, const int last_b_off, const float last_bias, const f32x4* __restrict__ wsdf) {
  return ((pr[t] + pr[32 + t]) + (pr[64 + t] + pr[96 + t])) + (last_b_off > 0 ? wsdf[last_b_off][0] : last_bias);
}

// ---- chain through the embedding: component c of d sdf / d x of a point from d sdf / d embedding, G(f) = the adjoint of embedding
// feature f of that point as the engine's image holds it; the features are summed in a fixed order
template <class Feat>
__device__ __forceinline__ float embed_chain(const Feat G, const int c, const int multires, const float* pts3, const float scale) {
  const float x0 = pts3[0] * scale, x1 = pts3[1] * scale, x2 = pts3[2] * scale;
  float g = G(c);
  int cc;
  for (int k = 0; k < multires; ++k) {
    const int fs = 3 + 6 * k + c, fc = fs + 3;
    g = fmaf(G(fs), posenc_jac(fs, x0, x1, x2, &cc), g);
    g = fmaf(G(fc), posenc_jac(fc, x0, x1, x2, &cc), g);
  }
  return g;
}

// ---- colour-net extras [pts, posenc(view), normal]: feature f of a point, zero beyond the last one
__device__ __forceinline__ float col_extra_feat(const int f, const float px, const float py, const float pz, const float dx,
                                                const float dy, const float dz, const float* grad3, const int n_view_feats,
                                                const int extra_feats) {
  float val = 0.f;
  if (f < 3) val = f == 0 ? px : (f == 1 ? py : pz);
  else if (f < 3 + n_view_feats) val = posenc_feat(f - 3, dx, dy, dz);
  else if (f < extra_feats) val = grad3[f - 3 - n_view_feats];
  return val;
}

// ---- rgb output: channel o of point pp of an image from the four waves' partial row dots (bias as for the sdf row; squeeze: sigmoid)
__device__ __forceinline__ float rgb_out(const float* pr, const int pp, const int o, const int last_b_off, const float last_bias_o,
                                         const int squeeze_out, const f32x4* __restrict__ wcol) {
  float v = ((pr[(0 * 32 + pp) * 3 + o] + pr[(1 * 32 + pp) * 3 + o]) + (pr[(2 * 32 + pp) * 3 + o] + pr[(3 * 32 + pp) * 3 + o])) +
            (last_b_off > 0 ? wcol[last_b_off][o] : last_bias_o);
  if (squeeze_out) v = 1.f / (1.f + expf(-v));
  return v;
}

// ---- training forward (TRAIN): the two-image fine kernels also leave what the backward tile programs and the weight-gradient
// contraction read (geo/train_programs.py, prog_fwd's stores) in the tile format of csrc/tile_vm.hip, [point tile][feature tile][32
// features][32 points] f32: E (embedding), U_1..U_nL (hidden activations), OUTF ([sdf ; features], 257 rows), GH_0..GH_{nL-1} (adjoints of
// the reverse sweep), EXTR (colour-net extras), C_1..C_nC (colour activations).
struct TrainOut {
  float* E; float* OUTF; float* EXTR;
  float* U[VQN_MAX_SDF_LAYERS]; float* GH[VQN_MAX_SDF_LAYERS]; float* C[VQN_MAX_COL_LAYERS];
  int e_tiles, outf_tiles, extr_tiles;
};

}  // namespace eng

