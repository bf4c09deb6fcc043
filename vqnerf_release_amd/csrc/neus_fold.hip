// Fold of the SDF network's feature layer into the colour network's first layer (C ABI: vqn_neus_fold_pack, include/vqn_neus_fold.h).
//
// The last SDF layer hands the colour net 256 feature rows with NO activation (fields.py:84-91: the activation stops at layer
// n - 2), and the first colour layer is linear in them (fields.py:147-166):
//     feat   = W8f . h7 + b8f                                   W8f = rows 1.. of the last SDF matrix
//     c0_pre = Wc0[:, feat] . feat + Wc0[:, extras] . extras + bc0
//            = (Wfold . h7 + bfold) + Wc0[:, extras] . extras,  Wfold = Wc0[:, feat] . W8f,  bfold = bc0 + Wc0[:, feat] . b8f
// so on the inference path, where nothing else reads `feat`, the fine kernel runs ONE K = hidden GEMM on Wfold where it ran
// the feature layer and a K = extras GEMM where it ran colour layer 0 over K = features + extras (csrc/neus_mlp.hip).
// Wfold / bfold depend on the weights only: this file computes them once per weight version -- float64 accumulation in the
// plain feature order, ONE rounding to f32 -- straight into the layouts the kernel reads (csrc/mlp_prims.h):
//     forward pack  [n_out_tiles][4 tiles(hidden)][64 lanes][4]   of Wfold            -> ColDesc::reserved1
//     bias pack     [n_out_tiles][2][16]                          of bfold            -> ColDesc::reserved2
//     forward pack  [n_out_tiles][extra_rows][64 lanes][4]        of Wc0[:, extras]   -> ColDesc::reserved3
// appended after a verbatim copy of the colour pack.  No scale is involved: the skip layer's 1/sqrt(2) sits in the skip layer's
// own pack (never the last layer: the planners refuse a skip into it), and SDFNetwork.scale touches the input and the sdf row only.
#include "common.h"
#include "vqn_neus_desc.h"
#include "vqn_neus_fold.h"

namespace {

struct FoldShape {
  int H, F, C, extra;            // SDF hidden width, features, colour hidden width, colour-net extras
  int hid_rows, extra_rows, n_out_tiles;
  int64_t base, n_w, n_b, n_e;   // floats: the copied colour pack, then the three blocks
};

__device__ __forceinline__ int phi(int i) { return 2 * (i & 3) + 8 * (i >> 3) + ((i >> 2) & 1); }
__device__ __forceinline__ int row_feat(int r, int h, int j) { return 32 * (r >> 2) + 2 * (4 * (r & 3) + j) + h; }

// one thread per f32 word of the output buffer
__global__ __launch_bounds__(256) void neus_fold_kernel(const FoldShape s, const float* __restrict__ wbuf_col,
                                                        const float* __restrict__ w8, const float* __restrict__ b8,
                                                        const float* __restrict__ wc0, const float* __restrict__ bc0,
                                                        float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.base + s.n_w + s.n_b + s.n_e) return;
  if (i < s.base) { out[i] = wbuf_col[i]; return; }
  const int ldc = s.extra + s.F;                     // Wc0 [C, extras + F]: input order [pts, view, normal, feat] (fields.py:147-158)
  int64_t k = i - s.base;
  if (k < s.n_w) {                                   // Wfold[c][kk] = sum_f Wc0[c][extra + f] * W8[1 + f][kk]
    const int j = (int)(k & 3), lane = (int)((k >> 2) & 63);
    const int64_t gq = k >> 8;
    const int g = (int)(gq % s.hid_rows), ot = (int)(gq / s.hid_rows);
    const int c = 32 * ot + phi(lane & 31), kk = row_feat(g, lane >> 5, j);
    double acc = 0.0;
    if (c < s.C && kk < s.H) {
      const float* __restrict__ a = wc0 + (size_t)c * ldc + s.extra;
      const float* __restrict__ b = w8 + s.H + kk;
      for (int f = 0; f < s.F; ++f) acc = fma((double)a[f], (double)b[(size_t)f * s.H], acc);
    }
    out[i] = (float)acc;
    return;
  }
  k -= s.n_w;
  if (k < s.n_b) {                                   // bfold[c] = bc0[c] + sum_f Wc0[c][extra + f] * b8[1 + f]
    const int r = (int)(k & 15), h = (int)((k >> 4) & 1), ot = (int)(k >> 5);
    const int c = 32 * ot + 2 * r + h;
    double acc = 0.0;
    if (c < s.C) {
      const float* __restrict__ a = wc0 + (size_t)c * ldc + s.extra;
      for (int f = 0; f < s.F; ++f) acc = fma((double)a[f], (double)b8[1 + f], acc);
      acc += (double)bc0[c];
    }
    out[i] = (float)acc;
    return;
  }
  k -= s.n_b;
  {                                                  // Wc0[:, extras] alone, as a K = extra_rows pack
    const int j = (int)(k & 3), lane = (int)((k >> 2) & 63);
    const int64_t gq = k >> 8;
    const int g = (int)(gq % s.extra_rows), ot = (int)(gq / s.extra_rows);
    const int c = 32 * ot + phi(lane & 31), f = row_feat(g, lane >> 5, j);
    out[i] = (c < s.C && f < s.extra) ? wc0[(size_t)c * ldc + f] : 0.0f;
  }
}

}  // namespace

extern "C" int64_t vqn_neus_fold_pack(const int32_t* sdf_desc, const int32_t* col_desc, const float* wbuf_col, int64_t col_floats,
                                      const float* sdf_w_last, const float* sdf_b_last, int sdf_hidden, int d_feature,
                                      const float* col_w0, const float* col_b0, int col_hidden, float* wbuf_out, int64_t out_floats,
                                      int32_t* col_desc_out, void* stream) {
  VQN_CHECK_ARG(sdf_desc && col_desc, "descriptors must be non-null");
  SdfDesc sd;
  ColDesc cd;
  memcpy(&sd, sdf_desc, sizeof(SdfDesc));
  memcpy(&cd, col_desc, sizeof(ColDesc));
  VQN_CHECK_SHAPE(sd.n_lin >= 2 && sd.n_lin <= VQN_MAX_SDF_LAYERS && cd.n_lin >= 2 && cd.n_lin <= VQN_MAX_COL_LAYERS, "layer counts");
  VQN_CHECK_ARG(sdf_hidden >= 1 && d_feature >= 1 && col_hidden >= 1, "widths must be positive");
  VQN_CHECK_ARG(col_floats > 0 && (col_floats & 3) == 0, "col_floats: the colour pack's size (a whole number of float4)");
  FoldShape s;
  s.H = sdf_hidden; s.F = d_feature; s.C = col_hidden; s.extra = cd.extra_feats;
  s.hid_rows = 4 * sd.layers[sd.n_lin - 2].n_out_tiles;
  s.extra_rows = cd.extra_rows;
  s.n_out_tiles = cd.layers[0].n_out_tiles;
  VQN_CHECK_SHAPE(s.hid_rows == 4 * ((s.H + 31) / 32) && sd.layers[sd.n_lin - 1].n_out_tiles == (s.F + 31) / 32 &&
                  s.n_out_tiles == (s.C + 31) / 32, "widths do not match the descriptors' tile counts");
  VQN_CHECK_SHAPE(s.extra >= 3 && s.extra <= 64 && s.extra_rows == (((s.extra + 1) / 2) + 3) / 4, "colour-net extras (f32 packs only)");
  VQN_CHECK_SHAPE(cd.reserved1 == 0 && cd.reserved2 == 0 && cd.reserved3 == 0, "col_desc is folded already");
  s.base = col_floats;
  s.n_w = (int64_t)s.n_out_tiles * s.hid_rows * 256;
  s.n_b = (int64_t)s.n_out_tiles * 32;
  s.n_e = (int64_t)s.n_out_tiles * s.extra_rows * 256;
  const int64_t total = s.base + s.n_w + s.n_b + s.n_e;
  VQN_CHECK_SHAPE(total / 4 < (int64_t)1 << 31, "pack too large for 32-bit float4 offsets");
  if (col_desc_out != nullptr) {
    cd.reserved1 = (int)(s.base / 4);
    cd.reserved2 = (int)((s.base + s.n_w) / 4);
    cd.reserved3 = (int)((s.base + s.n_w + s.n_b) / 4);
    memcpy(col_desc_out, &cd, sizeof(ColDesc));
  }
  if (wbuf_out == nullptr || out_floats < total) return total;
  VQN_CHECK_ARG(wbuf_col && sdf_w_last && sdf_b_last && col_w0 && col_b0, "weight pointers must be non-null");
  hipLaunchKernelGGL(neus_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s, wbuf_col, sdf_w_last,
                     sdf_b_last, col_w0, col_b0, wbuf_out);
  VQN_LAUNCH_CHECK();
  return total;
}
