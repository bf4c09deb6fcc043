// Fused NeuS network evaluation for gfx950: ray -> points -> posenc -> SDF MLP [-> analytic
// d sdf / d x -> colour MLP], one launch, activations never leave the CU except for the per-tile
// backward stash.  Replaces the framework-op sequences at
//   geo/NeuS-ours2/models/renderer.py:337-338,180-185   (coarse / up-sampling SDF evaluations)   -> vqn_neus_sdf_points
//   geo/NeuS-ours2/models/renderer.py:216-227 + fields.py:72-107,147-172
//        (sdf_network(pts), sdf_network.gradient(pts) = autograd wrt the input, color_network)   -> vqn_neus_fine_points
// The reference's gradient() re-runs the whole SDF forward (fields.py:98) and then calls autograd;
// here the input gradient is an explicit reverse sweep over the same packed weights (transposed
// packs), reusing the forward activations stashed per tile, so the forward runs once.
//
// Execution model: persistent workgroups over tiles of 32 points.  Narrow networks: one image per 256-thread workgroup, two
// workgroups per CU (neus_points_kernel).  Networks of 5 .. 8 tiles: the fine entry runs two in-place images per 256-thread
// workgroup, two independent workgroups per CU (neus_points2w_kernel); the SDF-only entry four in-place images per 512-thread
// workgroup (neus_pointsN_kernel); the training forward two ping-pong images per 512-thread workgroup (neus_points2_kernel).
// See mlp_prims.h for the LDS "activation image" and the weight-pack layout.
#include "neus_launch.h"
#include <stdlib.h>

using namespace eng;

// In-kernel phase stamps (cdna_hip_programming.md section 7): a DIAGNOSTIC build only (make stamps -> lib/libvqnerf_hip_stamps.so,
// -DVQN_STAMPS); the shipped library contains none of this.  Wave 0 of every workgroup accumulates shader-clock cycles per
// phase and adds them to g_stamps at exit: [0] tile set-up (points, posenc), [1] GEMM main loops (operand waits included),
// [2] epilogues, [3] barrier waits, [4] everything else, [5] total, [6] workgroups.
#ifdef VQN_STAMPS
__device__ unsigned long long g_stamps[8];
#define VQN_STAMP_DECL unsigned long long st_[6] = {0, 0, 0, 0, 0, 0}; unsigned long long st_prev = __builtin_amdgcn_s_memtime(); const unsigned long long st_begin = st_prev;
#define VQN_STAMP(i) { const unsigned long long st_now = __builtin_amdgcn_s_memtime(); st_[i] += st_now - st_prev; st_prev = st_now; }
#define VQN_STAMP_FLUSH if (threadIdx.x == 0) { st_[5] = __builtin_amdgcn_s_memtime() - st_begin; for (int i_ = 0; i_ < 6; ++i_) atomicAdd(&g_stamps[i_], st_[i_]); atomicAdd(&g_stamps[6], 1ull); }
extern "C" int vqn_debug_read_stamps(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8) != hipSuccess) return -3;
  if (reset) { unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)) != hipSuccess) return -3; }
  return 0;
}
#else
#define VQN_STAMP_DECL
#define VQN_STAMP(i)
#define VQN_STAMP_FLUSH
#endif

// 16-phase stamps of the two-image kernel (same DIAGNOSTIC build): [0] set-up [1] forward K loops [2] forward epilogues [3] forward
// barrier waits [4] sdf row + feature layer + sdf out [5] G_pre [6] reverse K loops (+ wTE) [7] reverse epilogues [8] reverse barrier
// waits [9] embedding chain rule [10] colour set-up [11] colour layers [12] colour out / turn-around [14] total [15] workgroups.
#ifdef VQN_STAMPS
__device__ unsigned long long g_stamps2[16];
#define FS_DECL unsigned long long fs_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long fs_prev = __builtin_amdgcn_s_memtime(); const unsigned long long fs_begin = fs_prev;
#define FS(i) { const unsigned long long fs_now = __builtin_amdgcn_s_memtime(); fs_[i] += fs_now - fs_prev; fs_prev = fs_now; }
#define FS_FLUSH if (threadIdx.x == 0) { fs_[14] = __builtin_amdgcn_s_memtime() - fs_begin; for (int i_ = 0; i_ < 15; ++i_) atomicAdd(&g_stamps2[i_], fs_[i_]); atomicAdd(&g_stamps2[15], 1ull); }
extern "C" int vqn_debug_read_stamps2(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps2), sizeof(unsigned long long) * 16) != hipSuccess) return -3;
  if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps2), z, sizeof(z)) != hipSuccess) return -3; }
  return 0;
}
#else
#define FS_DECL
#define FS(i)
#define FS_FLUSH
#endif

namespace {

constexpr int E0 = 0;        // LDS rows [0,8): embedding / colour-net extras / d sdf / d embedding
constexpr int E_ROWS = 8;

template <bool FINE>
__global__ __launch_bounds__(256, 2) void neus_points_kernel(
    const SdfDesc sd, const ColDesc cd, const f32x4* __restrict__ wsdf, const f32x4* __restrict__ wcol,
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ zv,
    const float* __restrict__ pts_direct, const float* __restrict__ dirs_direct, const long P, const int S,
    f32x4* __restrict__ scratch, float* __restrict__ out_sdf, float* __restrict__ out_grad,
    float* __restrict__ out_rgb) {
  extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
  const int MT = sd.max_tiles;
  const int X0 = E_ROWS, Y0 = E_ROWS + 4 * MT;
  Smalls<1>* sm = reinterpret_cast<Smalls<1>*>(lds + (size_t)(E_ROWS + 8 * MT) * 64);
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, p = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform by construction: let the compiler know
  const int n_lin = sd.n_lin;
  const int emb_tiles = (sd.emb_feats + 31) >> 5;
  const long n_tiles = (P + 31) >> 5;
  f32x4* save = FINE ? scratch + (size_t)blockIdx.x * (size_t)(n_lin - 1) * 4 * MT * 64 : nullptr;
  const int feat_slot = (n_lin - 2) * 4 * MT;

  VQN_STAMP_DECL
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long p0 = tile << 5;
    VQN_STAMP(4)
    // ---------------- points of this tile ----------------
    if (tid < 32)
      load_point<FINE>(p0 + tid, P, S, rays_o, rays_d, zv, pts_direct, dirs_direct, sm->pts[0] + tid * 3, sm->dirs[0] + tid * 3);
    __syncthreads();
    const float xs = sm->pts[0][p * 3 + 0] * sd.scale, ys = sm->pts[0][p * 3 + 1] * sd.scale, zs = sm->pts[0][p * 3 + 2] * sd.scale;
    // ---------------- positional encoding -> E rows ----------------
    for (int r = wave; r < sd.emb_rows; r += 4) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = emb_feat(row_feat(r, h, j), sd.emb_feats, xs, ys, zs);
      lds[(E0 + r) * 64 + lane] = v;
    }
    __syncthreads();

    VQN_STAMP(0)
    // ---------------- SDF hidden layers ----------------
    int cur = X0, oth = Y0;
    f32x4 pre[4];                                  // first weight fragments of the next layer's first tile of this wave
    {
      const f32x4* wp0 = wsdf + sd.layers[0].w_off + (size_t)wave * sd.emb_rows * 64 + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i) pre[i] = wp0[i * 64];
    }
    for (int l = 0; l < n_lin - 1; ++l) {
      const LayerDesc L = sd.layers[l];
      const f32x4* next_wp = nullptr;              // layer l + 1 has K rows = this layer's outputs (+ embedding at the skip)
      if (l + 1 < n_lin - 1)
        next_wp = wsdf + sd.layers[l + 1].w_off + (size_t)wave * (4 * L.n_out_tiles + ((l + 1 == sd.skip) ? sd.emb_rows : 0)) * 64 + lane;
      const KSegs ks = (l == 0) ? KSegs{E0, sd.emb_rows, 0, 0}
                                : KSegs{cur, 4 * sd.layers[l - 1].n_out_tiles, E0, (l == sd.skip) ? sd.emb_rows : 0};
      const int dst = (l == 0) ? X0 : oth;
      const bool do_save = FINE && (l < n_lin - 2);
      const f32x4* bp = wsdf + L.b_off;
      f32x4* sv = save + (size_t)l * 4 * MT * 64;
      gemm_tiles_chain(lds, ks, wsdf + L.w_off, L.n_out_tiles, wave, lane, pre, next_wp,
                 [&](int ot, f32x16& acc) { VQN_STAMP(2) init_bias(bp, ot, lane, acc); },
                 [&](int ot, const f32x16& acc) {
                   VQN_STAMP(1)
#pragma unroll
                   for (int rq = 0; rq < 4; ++rq) {
                     f32x4 v = acc_quad(acc, rq);
#pragma unroll
                     for (int j = 0; j < 4; ++j) v[j] = act_fwd<ACT_SOFTPLUS100>(v[j]);
                     lds[(dst + ot * 4 + rq) * 64 + lane] = v;
                     if (do_save) st_stream(sv + (ot * 4 + rq) * 64 + lane, v);
                   }
                 });
      VQN_STAMP(2)
      __syncthreads();
      VQN_STAMP(3)
      if (l == 0) { cur = X0; oth = Y0; } else { const int t = cur; cur = oth; oth = t; }
    }
    const int hid_rows = 4 * sd.layers[n_lin - 2].n_out_tiles;

    // ---------------- last layer: sdf row (VALU dot) [+ feature rows -> stash] ----------------
    rowdot<1>(lds, cur, hid_rows, wsdf + sd.last_w_off, sm->part[0], wave, lane);
    if (FINE && sd.layers[n_lin - 1].n_out_tiles > 0) {
      const LayerDesc L = sd.layers[n_lin - 1];
      const f32x4* bp = wsdf + L.b_off;
      f32x4* sv = save + (size_t)feat_slot * 64;
      gemm_tiles(lds, KSegs{cur, hid_rows, 0, 0}, wsdf + L.w_off, L.n_out_tiles, wave, lane,
                 [&](int ot, f32x16& acc) { init_bias(bp, ot, lane, acc); },
                 [&](int ot, const f32x16& acc) {
#pragma unroll
                   for (int rq = 0; rq < 4; ++rq) st_stream(sv + (ot * 4 + rq) * 64 + lane, acc_quad(acc, rq));
                 });
    }
    __syncthreads();
    if (tid < 32 && p0 + tid < P) out_sdf[p0 + tid] = sdf_raw(sm->part[0], tid, sd.last_b_off, sd.last_bias, wsdf) / sd.scale;
    if (!FINE) { __syncthreads(); continue; }

    // ---------------- reverse sweep: d sdf / d x ----------------
    // G_pre(last hidden) = w_sdf_row (.) act'(h), in place
    for (int r0 = wave; r0 < hid_rows; r0 += 32) {            // 8 rows per pass: all fetches first (one L2 round trip per pass)
      f32x4 v[8], wv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int r = min(r0 + 4 * c, hid_rows - 1);
        v[c] = lds[(cur + r) * 64 + lane];
        wv[c] = wsdf[sd.last_w_off + r * 2 + h];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (r0 + 4 * c < hid_rows) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[c][j] = wv[c][j] * act_bwd_from_out<ACT_SOFTPLUS100>(v[c][j]);
          lds[(cur + r0 + 4 * c) * 64 + lane] = v[c];
        }
    }
    __syncthreads();
    for (int l = n_lin - 2; l >= 1; --l) {
      const LayerDesc L = sd.layers[l];
      const KSegs ks{cur, 4 * L.n_out_tiles, 0, 0};
      const f32x4* sv = save + (size_t)(l - 1) * 4 * MT * 64;
      const int dst = oth;
      f32x4 hv[4];                                   // stashed forward activations of this tile: requested BEFORE the K loop so that
                                                     // their (L2 / Infinity-Cache) latency hides under the MFMAs, not behind them
      gemm_tiles(lds, ks, wsdf + L.wT_off, sd.layers[l - 1].n_out_tiles, wave, lane,
                 [&](int ot, f32x16& acc) {
#pragma unroll
                   for (int rq = 0; rq < 4; ++rq) hv[rq] = ld_stream(sv + (ot * 4 + rq) * 64 + lane);
                   init_zero(acc);
                 },
                 [&](int ot, const f32x16& acc) {
#pragma unroll
                   for (int rq = 0; rq < 4; ++rq) {
                     f32x4 v = acc_quad(acc, rq);
#pragma unroll
                     for (int j = 0; j < 4; ++j) v[j] *= act_bwd_from_out<ACT_SOFTPLUS100>(hv[rq][j]);
                     lds[(dst + ot * 4 + rq) * 64 + lane] = v;
                   }
                 });
      if (l == sd.skip)
        gemm_tiles(lds, ks, wsdf + L.wTE_off, emb_tiles, wave, lane,
                   [&](int, f32x16& acc) { init_zero(acc); },
                   [&](int ot, const f32x16& acc) {
#pragma unroll
                     for (int rq = 0; rq < 4; ++rq) lds[(E0 + ot * 4 + rq) * 64 + lane] = acc_quad(acc, rq);
                   });
      __syncthreads();
      const int t = cur; cur = oth; oth = t;
    }
    {
      const LayerDesc L = sd.layers[0];
      const bool accumulate = sd.skip >= 1;
      gemm_tiles(lds, KSegs{cur, 4 * L.n_out_tiles, 0, 0}, wsdf + L.wTE_off, emb_tiles, wave, lane,
                 [&](int ot, f32x16& acc) {
                   if (accumulate) init_rows(lds + (E0 + ot * 4) * 64, lane, acc); else init_zero(acc);
                 },
                 [&](int ot, const f32x16& acc) {
#pragma unroll
                   for (int rq = 0; rq < 4; ++rq) lds[(E0 + ot * 4 + rq) * 64 + lane] = acc_quad(acc, rq);
                 });
    }
    __syncthreads();
    // chain through the embedding: thread (point pp, component c) sums its features in a fixed order
    if (tid < 96) {
      const int pp = tid & 31, c = tid >> 5;
      const float g = embed_chain([&](int f) { return lds_feat(lds, E0, f, pp); }, c, sd.multires, sm->pts[0] + pp * 3, sd.scale);
      sm->grad[0][pp * 3 + c] = g;
      if (p0 + pp < P) out_grad[(p0 + pp) * 3 + c] = g;
    }
    __syncthreads();
    if (cd.n_lin == 0) continue;          // SDFNetwork.gradient(): no colour net

    // ---------------- colour network ----------------
    {
      const float px = sm->pts[0][p * 3 + 0], py = sm->pts[0][p * 3 + 1], pz = sm->pts[0][p * 3 + 2];
      const float dx = sm->dirs[0][p * 3 + 0], dy = sm->dirs[0][p * 3 + 1], dz = sm->dirs[0][p * 3 + 2];
      for (int r = wave; r < cd.extra_rows; r += 4) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = col_extra_feat(row_feat(r, h, j), px, py, pz, dx, dy, dz, sm->grad[0] + p * 3, cd.n_view_feats, cd.extra_feats);
        lds[(E0 + r) * 64 + lane] = v;
      }
      const f32x4* sv = save + (size_t)feat_slot * 64;
      const int feat_rows = 4 * sd.layers[n_lin - 1].n_out_tiles;
      for (int r0 = wave; r0 < feat_rows; r0 += 32) {          // feature rows back from the stash: 8 fetches in flight per pass
        f32x4 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = ld_stream(sv + min(r0 + 4 * c, feat_rows - 1) * 64 + lane);
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (r0 + 4 * c < feat_rows) lds[(X0 + r0 + 4 * c) * 64 + lane] = v[c];
      }
      __syncthreads();
      cur = X0; oth = Y0;
      int in_rows = feat_rows;
      for (int l = 0; l < cd.n_lin - 1; ++l) {
        const LayerDesc L = cd.layers[l];
        const KSegs ks{cur, in_rows, E0, l == 0 ? cd.extra_rows : 0};
        const f32x4* bp = wcol + L.b_off;
        const int dst = oth;
        gemm_tiles(lds, ks, wcol + L.w_off, L.n_out_tiles, wave, lane,
                   [&](int ot, f32x16& acc) { init_bias(bp, ot, lane, acc); },
                   [&](int ot, const f32x16& acc) {
#pragma unroll
                     for (int rq = 0; rq < 4; ++rq) {
                       f32x4 v = acc_quad(acc, rq);
#pragma unroll
                       for (int j = 0; j < 4; ++j) v[j] = act_fwd<ACT_RELU>(v[j]);
                       lds[(dst + ot * 4 + rq) * 64 + lane] = v;
                     }
                   });
        __syncthreads();
        const int t = cur; cur = oth; oth = t;
        in_rows = 4 * L.n_out_tiles;
      }
      rowdot<3>(lds, cur, in_rows, wcol + cd.last_w_off, sm->part[0], wave, lane);
      __syncthreads();
      if (tid < 96) {
        const int pp = tid & 31, o = tid >> 5;
        const float v = rgb_out(sm->part[0], pp, o, cd.last_b_off, cd.last_bias[o], cd.squeeze_out, wcol);
        if (p0 + pp < P) out_rgb[(p0 + pp) * 3 + o] = v;
      }
    }
    __syncthreads();
  }
  VQN_STAMP(4)
  VQN_STAMP_FLUSH
}

// ---------------------------------------------------------------------------------------------------------------------
// Two-image form (the default for networks of >= 5 tiles that fit): one 512-thread workgroup per CU holds TWO 32-point
// images; wave w owns output tiles w, w + 8, ... and applies each weight fragment to both images (gemm_tiles2).  All eight
// waves do the same matrix work between two barriers and no second workgroup competes for the matrix pipe, so the waves
// of a layer finish together (the one-image form loses ~20 % to barrier skew between its two co-resident workgroups);
// barriers and the L2 weight stream per point halve.  The VALU phases split by image: waves 0-3 image 0, waves 4-7 image 1.
// Same per-point arithmetic as the one-image kernel except the two embedding-gradient GEMMs of the reverse sweep, which are
// split over K (wte_split_k: a different, still fixed, summation order for d sdf / d x).
// d sdf / d embedding of one layer for both images: E rows (+)= W_E^T . G over the K rows [k_row0, k_row0 + ng).  The result
// has only emb_tiles (<= 2) output tiles, so as a plain gemm_tiles2 call it keeps 2 of the 8 waves busy for a whole K = 256 pass;
// here the waves split it as (tile, K slice) units, park their partial tiles in the free activation buffer `tmp_row0`
// (4 rows per unit and image, `tmp_rows` available: 8 units at d_hidden = 256) and sum them in a fixed slice order.  Ends with the E rows written and a barrier passed.
__device__ __forceinline__ void wte_split_k(f32x4* __restrict__ lds, const int IS, const int k_row0, const int ng,
                                            const f32x4* __restrict__ w, const int emb_tiles, const int tmp_row0, const int tmp_rows,
                                            const int e_row0, const bool accumulate, const int wave, const int lane) {
  const int KS = min(8, tmp_rows >> 2) / emb_tiles, gk = (ng + KS - 1) / KS;          // K slices (4 parking rows each), groups per slice
  const int t = wave % emb_tiles, kq = wave / emb_tiles;
  if (kq < KS) {
    f32x16 acc0, acc1;
    init_zero(acc0); init_zero(acc1);
    const int g0 = kq * gk, g1 = min(ng, g0 + gk);
    const f32x4* __restrict__ wp = w + (size_t)t * ng * 64 + lane;
    for (int g = g0; g < g1; g += 8) {
      f32x4 a[8], p[8], q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int gg = min(g + i, ng - 1), r = (k_row0 + gg) * 64 + lane;
        a[i] = wp[gg * 64]; p[i] = lds[r]; q[i] = lds[r + IS];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (g + i < g1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][j], p[i][j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][j], q[i][j], acc1, 0, 0, 0);
          }
        }
    }
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      lds[(tmp_row0 + wave * 4 + rq) * 64 + lane] = acc_quad(acc0, rq);
      lds[IS + (tmp_row0 + wave * 4 + rq) * 64 + lane] = acc_quad(acc1, rq);
    }
  }
  __syncthreads();
  for (int r = wave; r < 8 * emb_tiles; r += 8) {                   // (image, tile, row quad) units
    const int im = r / (4 * emb_tiles), er = r - im * 4 * emb_tiles, tt = er >> 2, rq = er & 3;
    f32x4* li = lds + (size_t)im * IS;
    f32x4 sum = li[(tmp_row0 + tt * 4 + rq) * 64 + lane];
    for (int k = 1; k < KS; ++k) sum += li[(tmp_row0 + (k * emb_tiles + tt) * 4 + rq) * 64 + lane];
    if (accumulate) sum += li[(e_row0 + er) * 64 + lane];
    li[(e_row0 + er) * 64 + lane] = sum;
  }
  __syncthreads();
}

template <bool FINE, bool TRAIN = false, bool FOLD = false>
__global__ __launch_bounds__(512, 1) void neus_points2_kernel(
    const SdfDesc sd, const ColDesc cd, const f32x4* __restrict__ wsdf, const f32x4* __restrict__ wcol,
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ zv,
    const float* __restrict__ pts_direct, const float* __restrict__ dirs_direct, const long P, const int S,
    f32x4* __restrict__ scratch, float* __restrict__ out_sdf, float* __restrict__ out_grad,
    float* __restrict__ out_rgb, const TrainOut to) {
  extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
  const int MT = sd.max_tiles;
  const int IMG = E_ROWS + 8 * MT, IS = IMG * 64;
  const int X0 = E_ROWS, Y0 = E_ROWS + 4 * MT;
  Smalls<2>* sm = reinterpret_cast<Smalls<2>*>(lds + (size_t)2 * IS);
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, p = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int img = wave >> 2, w4 = wave & 3;
  f32x4* ldsi = lds + (size_t)img * IS;
  const int n_lin = sd.n_lin;
  const int emb_tiles = (sd.emb_feats + 31) >> 5;
  const long n_tiles = (P + 31) >> 5, n_pairs = (n_tiles + 1) >> 1;
  const size_t per_img = (size_t)(n_lin - 1) * 4 * MT * 64;
#ifdef VQN_DIAG_STASH_ROT     // timing only (make diag FLAG=VQN_DIAG_STASH_ROT=4): every workgroup walks ROT stash regions in turn, so ROT x 128 MB of
                              // stash are in flight instead of 128 MB -- is the stash fast because it sits in the 256 MiB Infinity Cache?
  f32x4* save0 = nullptr;
#else
  f32x4* save0 = FINE ? scratch + (size_t)blockIdx.x * 2 * per_img : nullptr;
#endif
  const int feat_slot = (n_lin - 2) * 4 * MT;
  // Folded colour input (csrc/neus_fold.hip, inference only): the GEMM at the feature layer's position runs on Wfold = Wc0[:, feat] . W8f
  // and leaves P = Wfold . h + bfold in the stash slot of the features; colour layer 0 is then a K = extras GEMM on top of P.
  // FOLD is chosen by the host from the descriptor (ColDesc::reserved1..3 != 0); the unfolded instance is the kernel as it was.
  constexpr bool fold = FOLD;
  static_assert(!FOLD || (FINE && !TRAIN), "the fold is an inference path: the backward and the weight gradients read OUTF");
  f32x4 pre[4];
  f32x4 nopre[4];

  FS_DECL
  for (long pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
#ifdef VQN_DIAG_STASH_ROT
    if (FINE) save0 = scratch + ((size_t)((pair / gridDim.x) % VQN_DIAG_STASH_ROT) * gridDim.x + blockIdx.x) * 2 * per_img;
#endif
    FS(12)
    // ---------------- points of both tiles ----------------
    if (tid < 64) {
      const int im = tid >> 5, t = tid & 31;
      load_point<FINE>(((2 * pair + im) << 5) + t, P, S, rays_o, rays_d, zv, pts_direct, dirs_direct, sm->pts[im] + t * 3, sm->dirs[im] + t * 3);
    }
    __syncthreads();
    const float xs = sm->pts[img][p * 3 + 0] * sd.scale, ys = sm->pts[img][p * 3 + 1] * sd.scale, zs = sm->pts[img][p * 3 + 2] * sd.scale;
    const long ptile_w = 2 * pair + img;                   // (TRAIN) the point tile of this wave's image; stores are skipped for a phantom tile
    for (int r = w4; r < (TRAIN ? 4 * to.e_tiles : sd.emb_rows); r += 4) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = r < sd.emb_rows ? emb_feat(row_feat(r, h, j), sd.emb_feats, xs, ys, zs) : 0.f;
      if (r < sd.emb_rows) ldsi[(E0 + r) * 64 + lane] = v;
      if (TRAIN && ptile_w < n_tiles) tfmt_store_quad(to.E, ptile_w, to.e_tiles, r >> 2, r & 3, lane, v);
    }
    __syncthreads();

    FS(0)
    // ---------------- SDF hidden layers ----------------
    int cur = X0, oth = Y0;
    if (wave < sd.layers[0].n_out_tiles) {
      const f32x4* wp0 = wsdf + sd.layers[0].w_off + (size_t)wave * sd.emb_rows * 64 + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i) pre[i] = wp0[min(i, sd.emb_rows - 1) * 64];
    }
    for (int l = 0; l < n_lin - 1; ++l) {
      const LayerDesc L = sd.layers[l];
      const f32x4* next_wp = nullptr;
      if (l + 1 < n_lin - 1 && wave < sd.layers[l + 1].n_out_tiles)
        next_wp = wsdf + sd.layers[l + 1].w_off + (size_t)wave * (4 * L.n_out_tiles + ((l + 1 == sd.skip) ? sd.emb_rows : 0)) * 64 + lane;
      const KSegs ks = (l == 0) ? KSegs{E0, sd.emb_rows, 0, 0}
                                : KSegs{cur, 4 * sd.layers[l - 1].n_out_tiles, E0, (l == sd.skip) ? sd.emb_rows : 0};
      const int dst = (l == 0) ? X0 : oth;
      const bool do_save = FINE && (l < n_lin - 2);
      const f32x4* bp = wsdf + L.b_off;
      float* const t_u = TRAIN ? to.U[l + 1] : nullptr;          // (one scalar load per layer: no dynamic index inside the epilogue)
      auto bias_init = [&](int ot, int im, f32x16& acc) { if (im == 0) { FS(2) } init_bias(bp, ot, lane, acc); };
      auto epi_rq = [&](int ot, int im, int rq, const f32x16& acc) {
        if (im == 0 && rq == 0) { FS(1) }
        f32x4* li = lds + (size_t)im * IS;
        f32x4* sv = save0 + (size_t)im * per_img + (size_t)l * 4 * MT * 64;
        f32x4 v = {acc[4 * rq], acc[4 * rq + 1], acc[4 * rq + 2], acc[4 * rq + 3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = act_fwd<ACT_SOFTPLUS100>(v[j]);
        li[(dst + ot * 4 + rq) * 64 + lane] = v;
        if (do_save) st_stream(sv + (ot * 4 + rq) * 64 + lane, v);
        if (TRAIN && 2 * pair + im < n_tiles) tfmt_store_quad(t_u, 2 * pair + im, L.n_out_tiles, ot, rq, lane, v);
      };
      gemm_tiles2<8>(lds, IS, ks, wsdf + L.w_off, L.n_out_tiles, wave, lane, pre, true, next_wp, bias_init, epi_rq);
      FS(2)
      __syncthreads();
      FS(3)
      if (l == 0) { cur = X0; oth = Y0; } else { const int t = cur; cur = oth; oth = t; }
    }
    const int hid_rows = 4 * sd.layers[n_lin - 2].n_out_tiles;

    // ---------------- last layer: sdf row (VALU dot, per image) [+ feature rows -> stash] ----------------
    rowdot<1>(ldsi, cur, hid_rows, wsdf + sd.last_w_off, sm->part[img], w4, lane);
    if (FINE && sd.layers[n_lin - 1].n_out_tiles > 0) {
      const LayerDesc L = sd.layers[n_lin - 1];
      const f32x4* bp = fold ? wcol + cd.reserved2 : wsdf + L.b_off;
      gemm_tiles2<8>(lds, IS, KSegs{cur, hid_rows, 0, 0}, fold ? wcol + cd.reserved1 : wsdf + L.w_off,
                     fold ? cd.layers[0].n_out_tiles : L.n_out_tiles, wave, lane, nopre, false, nullptr,
                     [&](int ot, int, f32x16& acc) { init_bias(bp, ot, lane, acc); },
                     [&](int ot, int im, int rq, const f32x16& acc) {
                       f32x4* sv = save0 + (size_t)im * per_img + (size_t)feat_slot * 64;
                       const f32x4 v = {acc[4 * rq], acc[4 * rq + 1], acc[4 * rq + 2], acc[4 * rq + 3]};
                       st_stream(sv + (ot * 4 + rq) * 64 + lane, v);
                       if (TRAIN && 2 * pair + im < n_tiles) {              // OUTF = [sdf ; features]: feature f of this GEMM is row f + 1
                         float* base = to.OUTF + (2 * pair + im) * (long)to.outf_tiles * 1024;
#pragma unroll
                         for (int j = 0; j < 4; ++j) {
                           const int f = 32 * ot + 2 * (4 * rq + j) + h + 1;
                           if (f < 32 * to.outf_tiles) __builtin_nontemporal_store(v[j], base + f * 32 + p);
                         }
                       }
                     });
    }
    __syncthreads();
    if (tid < 64) {
      const int im = tid >> 5, t = tid & 31;
      const long pt = ((2 * pair + im) << 5) + t;
      if (pt < P) out_sdf[pt] = sdf_raw(sm->part[im], t, sd.last_b_off, sd.last_bias, wsdf) / sd.scale;
      if (TRAIN && 2 * pair + im < n_tiles) {                        // row 0 of OUTF (the raw sdf output) and the zero tail beyond row F - 1
        float* base = to.OUTF + (2 * pair + im) * (long)to.outf_tiles * 1024;
        base[t] = sdf_raw(sm->part[im], t, sd.last_b_off, sd.last_bias, wsdf);
        for (int f = 32 * sd.layers[n_lin - 1].n_out_tiles + 1; f < 32 * to.outf_tiles; ++f) base[f * 32 + t] = 0.f;
      }
    }
    if (!FINE) { __syncthreads(); FS(4) continue; }
    FS(4)

    // ---------------- reverse sweep: d sdf / d x ----------------
    float* const t_gh_top = TRAIN ? to.GH[n_lin - 2] : nullptr;
    for (int r0 = w4; r0 < hid_rows; r0 += 32) {
      f32x4 v[8], wv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int r = min(r0 + 4 * c, hid_rows - 1);
        v[c] = ldsi[(cur + r) * 64 + lane];
        wv[c] = wsdf[sd.last_w_off + r * 2 + h];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (r0 + 4 * c < hid_rows) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[c][j] = wv[c][j] * act_bwd_from_out<ACT_SOFTPLUS100>(v[c][j]);
          ldsi[(cur + r0 + 4 * c) * 64 + lane] = v[c];
          if (TRAIN && ptile_w < n_tiles)
            tfmt_store_quad(t_gh_top, ptile_w, sd.layers[n_lin - 2].n_out_tiles, (r0 + 4 * c) >> 2, (r0 + 4 * c) & 3, lane, v[c]);
        }
    }
    __syncthreads();
    FS(5)
    for (int l = n_lin - 2; l >= 1; --l) {
      const LayerDesc L = sd.layers[l];
      const KSegs ks{cur, 4 * L.n_out_tiles, 0, 0};
      const int dst = oth;
      if (l == sd.skip)                                 // embedding part of the skip layer first: `oth` is still free for the partials
        wte_split_k(lds, IS, cur, 4 * L.n_out_tiles, wsdf + L.wTE_off, emb_tiles, oth, 4 * MT, E0, false, wave, lane);
      f32x4 hv[2][4];
      float* const t_gh = TRAIN ? to.GH[l - 1] : nullptr;
      const int gh_tiles = sd.layers[l - 1].n_out_tiles;
      gemm_tiles2<8>(lds, IS, ks, wsdf + L.wT_off, sd.layers[l - 1].n_out_tiles, wave, lane, nopre, false, nullptr,
                     [&](int ot, int im, f32x16& acc) {
                       if (im == 0) { FS(7) }
                       const f32x4* sv = save0 + (size_t)im * per_img + (size_t)(l - 1) * 4 * MT * 64;
#pragma unroll
                       for (int rq = 0; rq < 4; ++rq) hv[im][rq] = ld_stream(sv + (ot * 4 + rq) * 64 + lane);
                       init_zero(acc);
                     },
                     [&](int ot, int im, int rq, const f32x16& acc) {
                       if (im == 0 && rq == 0) { FS(6) }
                       f32x4* li = lds + (size_t)im * IS;
                       f32x4 v = {acc[4 * rq], acc[4 * rq + 1], acc[4 * rq + 2], acc[4 * rq + 3]};
#pragma unroll
                       for (int j = 0; j < 4; ++j) v[j] *= act_bwd_from_out<ACT_SOFTPLUS100>(hv[im][rq][j]);
                       li[(dst + ot * 4 + rq) * 64 + lane] = v;
                       if (TRAIN && 2 * pair + im < n_tiles) tfmt_store_quad(t_gh, 2 * pair + im, gh_tiles, ot, rq, lane, v);
                     });
      FS(7)
      __syncthreads();
      FS(8)
      const int t = cur; cur = oth; oth = t;
    }
    wte_split_k(lds, IS, cur, 4 * sd.layers[0].n_out_tiles, wsdf + sd.layers[0].wTE_off, emb_tiles, oth, 4 * MT, E0, sd.skip >= 1, wave, lane);
    FS(6)
    if (tid < 192) {
      const int im = tid / 96, r = tid - 96 * im, pp = r & 31, c = r >> 5;
      const f32x4* li = lds + (size_t)im * IS;
      const float g = embed_chain([&](int f) { return lds_feat(li, E0, f, pp); }, c, sd.multires, sm->pts[im] + pp * 3, sd.scale);
      sm->grad[im][pp * 3 + c] = g;
      const long pt = ((2 * pair + im) << 5) + pp;
      if (pt < P) out_grad[pt * 3 + c] = g;
    }
    __syncthreads();
    FS(9)
    if (cd.n_lin == 0) continue;

    // ---------------- colour network ----------------
    {
      const float px = sm->pts[img][p * 3 + 0], py = sm->pts[img][p * 3 + 1], pz = sm->pts[img][p * 3 + 2];
      const float dx = sm->dirs[img][p * 3 + 0], dy = sm->dirs[img][p * 3 + 1], dz = sm->dirs[img][p * 3 + 2];
      for (int r = w4; r < (TRAIN ? 4 * to.extr_tiles : cd.extra_rows); r += 4) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = r < cd.extra_rows ? col_extra_feat(row_feat(r, h, j), px, py, pz, dx, dy, dz, sm->grad[img] + p * 3, cd.n_view_feats, cd.extra_feats) : 0.f;
        if (r < cd.extra_rows) ldsi[(E0 + r) * 64 + lane] = v;
        if (TRAIN && ptile_w < n_tiles) tfmt_store_quad(to.EXTR, ptile_w, to.extr_tiles, r >> 2, r & 3, lane, v);
      }
      const f32x4* sv = save0 + (size_t)img * per_img + (size_t)feat_slot * 64;
      const int feat_rows = 4 * sd.layers[n_lin - 1].n_out_tiles;
      for (int r0 = w4; r0 < (fold ? 0 : feat_rows); r0 += 32) {         // (unfolded) the feature rows back from the stash
        f32x4 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = ld_stream(sv + min(r0 + 4 * c, feat_rows - 1) * 64 + lane);
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (r0 + 4 * c < feat_rows) ldsi[(X0 + r0 + 4 * c) * 64 + lane] = v[c];
      }
      __syncthreads();
      FS(10)
      cur = X0; oth = Y0;
      int in_rows = feat_rows;
      if (fold) {                                   // colour layer 0 = relu(P + Wc0[:, extras] . extras): K = the extras rows only
        const LayerDesc L = cd.layers[0];
        const int dst = oth;
        gemm_tiles2<8>(lds, IS, KSegs{E0, cd.extra_rows, 0, 0}, wcol + cd.reserved3, L.n_out_tiles, wave, lane, nopre, false, nullptr,
                       [&](int ot, int im, f32x16& acc) {
                         const f32x4* pp = save0 + (size_t)im * per_img + (size_t)feat_slot * 64 + ot * 256 + lane;
#pragma unroll
                         for (int rq = 0; rq < 4; ++rq) {
                           const f32x4 v = ld_stream(pp + rq * 64);
                           acc[4 * rq + 0] = v[0]; acc[4 * rq + 1] = v[1]; acc[4 * rq + 2] = v[2]; acc[4 * rq + 3] = v[3];
                         }
                       },
                       [&](int ot, int im, int rq, const f32x16& acc) {
                         f32x4* li = lds + (size_t)im * IS;
                         f32x4 v = {acc[4 * rq], acc[4 * rq + 1], acc[4 * rq + 2], acc[4 * rq + 3]};
#pragma unroll
                         for (int j = 0; j < 4; ++j) v[j] = act_fwd<ACT_RELU>(v[j]);
                         li[(dst + ot * 4 + rq) * 64 + lane] = v;
                       });
        __syncthreads();
        const int t = cur; cur = oth; oth = t;
        in_rows = 4 * L.n_out_tiles;
      }
      for (int l = fold ? 1 : 0; l < cd.n_lin - 1; ++l) {
        const LayerDesc L = cd.layers[l];
        const KSegs ks{cur, in_rows, E0, l == 0 ? cd.extra_rows : 0};
        const f32x4* bp = wcol + L.b_off;
        const int dst = oth;
        float* const t_c = TRAIN ? to.C[l + 1] : nullptr;
        gemm_tiles2<8>(lds, IS, ks, wcol + L.w_off, L.n_out_tiles, wave, lane, nopre, false, nullptr,
                       [&](int ot, int, f32x16& acc) { init_bias(bp, ot, lane, acc); },
                       [&](int ot, int im, int rq, const f32x16& acc) {
                         f32x4* li = lds + (size_t)im * IS;
                         f32x4 v = {acc[4 * rq], acc[4 * rq + 1], acc[4 * rq + 2], acc[4 * rq + 3]};
#pragma unroll
                         for (int j = 0; j < 4; ++j) v[j] = act_fwd<ACT_RELU>(v[j]);
                         li[(dst + ot * 4 + rq) * 64 + lane] = v;
                         if (TRAIN && 2 * pair + im < n_tiles) tfmt_store_quad(t_c, 2 * pair + im, L.n_out_tiles, ot, rq, lane, v);
                       });
        __syncthreads();
        const int t = cur; cur = oth; oth = t;
        in_rows = 4 * L.n_out_tiles;
      }
      FS(11)
      rowdot<3>(ldsi, cur, in_rows, wcol + cd.last_w_off, sm->part[img], w4, lane);
      __syncthreads();
      if (tid < 192) {
        const int im = tid / 96, r = tid - 96 * im, pp = r & 31, o = r >> 5;
        const float v = rgb_out(sm->part[im], pp, o, cd.last_b_off, cd.last_bias[o], cd.squeeze_out, wcol);
        const long pt = ((2 * pair + im) << 5) + pp;
        if (pt < P) out_rgb[pt * 3 + o] = v;
      }
    }
    __syncthreads();
  }
  FS(12)
  FS_FLUSH
}

// ---------------------------------------------------------------------------------------------------------------------
// NIMG-image form of the SDF-only kernel (NIMG = 3, 4): the per-layer cost of the two-image form that is not matrix work (operand
// pipeline fill, epilogue, barrier) stays what it is and NIMG / 2 times the matrix work goes between two barriers.  Without a stash, a
// reverse sweep or a colour net an image needs no second activation buffer: a layer is computed IN PLACE -- K loop, epilogue into the
// accumulator registers (gemm_tilesN), barrier, the tile's rows over the layer's input, barrier -- so an image is its embedding rows
// (sd.emb_rows of them, not E_ROWS) plus 4 max_tiles activation rows.  One output tile per wave: max_tiles <= 8.  The VALU phases are
// dealt over the eight waves as (image, row) and (image, quarter) units; per point the arithmetic and its order are those of
// neus_points2_kernel<false>, so the outputs are the same bits.
template <int NIMG>
struct SmallsSdf {           // Smalls without what only the fine kernels use (grad, the rgb partials): what lets four images fit
  float pts[NIMG][96], dirs[NIMG][96], part[NIMG][128];
};

template <int NIMG>
__global__ __launch_bounds__(512, 1) void neus_pointsN_kernel(
    const SdfDesc sd, const f32x4* __restrict__ wsdf, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
    const float* __restrict__ zv, const float* __restrict__ pts_direct, const long P, const int S, float* __restrict__ out_sdf) {
  extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
  const int MT = sd.max_tiles;
  const int X0 = sd.emb_rows, IS = (sd.emb_rows + 4 * MT) * 64;
  SmallsSdf<NIMG>* sm = reinterpret_cast<SmallsSdf<NIMG>*>(lds + (size_t)NIMG * IS);
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, p = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_lin = sd.n_lin;
  const long n_tiles = (P + 31) >> 5, n_groups = (n_tiles + NIMG - 1) / NIMG;
  f32x4 pre[4];
  f32x16 acc[NIMG];

  for (long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    // ---------------- points of the NIMG tiles (a tile past n_tiles: clamped points, nothing stored) ----------------
    if (tid < 32 * NIMG) {
      const int im = tid >> 5, t = tid & 31;
      load_point<false>(((NIMG * grp + im) << 5) + t, P, S, rays_o, rays_d, zv, pts_direct, nullptr, sm->pts[im] + t * 3, sm->dirs[im] + t * 3);
    }
    __syncthreads();
    for (int u = wave; u < NIMG * sd.emb_rows; u += 8) {                  // (image, embedding row) units
      const int im = u / sd.emb_rows, r = u - im * sd.emb_rows;
      const float xs = sm->pts[im][p * 3 + 0] * sd.scale, ys = sm->pts[im][p * 3 + 1] * sd.scale, zs = sm->pts[im][p * 3 + 2] * sd.scale;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = emb_feat(row_feat(r, h, j), sd.emb_feats, xs, ys, zs);
      lds[(size_t)im * IS + (E0 + r) * 64 + lane] = v;
    }
    __syncthreads();

    // ---------------- SDF hidden layers, in place ----------------
    if (wave < sd.layers[0].n_out_tiles) {
      const f32x4* wp0 = wsdf + sd.layers[0].w_off + (size_t)wave * sd.emb_rows * 64 + lane;
#pragma unroll
      for (int i = 0; i < 4; ++i) pre[i] = wp0[min(i, sd.emb_rows - 1) * 64];
    }
    for (int l = 0; l < n_lin - 1; ++l) {
      const LayerDesc L = sd.layers[l];
      const f32x4* next_wp = nullptr;
      if (l + 1 < n_lin - 1 && wave < sd.layers[l + 1].n_out_tiles)
        next_wp = wsdf + sd.layers[l + 1].w_off + (size_t)wave * (4 * L.n_out_tiles + ((l + 1 == sd.skip) ? sd.emb_rows : 0)) * 64 + lane;
      const KSegs ks = (l == 0) ? KSegs{E0, sd.emb_rows, 0, 0}
                                : KSegs{X0, 4 * sd.layers[l - 1].n_out_tiles, E0, (l == sd.skip) ? sd.emb_rows : 0};
      const f32x4* bp = wsdf + L.b_off;
      gemm_tilesN<NIMG, 8>(lds, IS, ks, wsdf + L.w_off, L.n_out_tiles, wave, lane, pre, next_wp, acc,
                           [&](int ot, int, f32x16& a) { init_bias(bp, ot, lane, a); },
                           [&](int, int, int rq, f32x16& a) {
#pragma unroll
                             for (int j = 0; j < 4; ++j) a[4 * rq + j] = act_fwd<ACT_SOFTPLUS100>(a[4 * rq + j]);
                           });
      if (l > 0) __syncthreads();                      // every wave is done reading X (layer 0 reads the E rows only)
      if (wave < L.n_out_tiles) {
#pragma unroll
        for (int im = 0; im < NIMG; ++im) {
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) lds[(size_t)im * IS + (X0 + wave * 4 + rq) * 64 + lane] = acc_quad(acc[im], rq);
        }
      }
      __syncthreads();
    }
    const int hid_rows = 4 * sd.layers[n_lin - 2].n_out_tiles;

    // ---------------- last layer: sdf row (VALU dot), four partials per image ----------------
    for (int u = wave; u < 4 * NIMG; u += 8)
      rowdot<1>(lds + (size_t)(u >> 2) * IS, X0, hid_rows, wsdf + sd.last_w_off, sm->part[u >> 2], u & 3, lane);
    __syncthreads();
    if (tid < 32 * NIMG) {
      const int im = tid >> 5, t = tid & 31;
      const long pt = ((NIMG * grp + im) << 5) + t;
      if (pt < P) out_sdf[pt] = sdf_raw(sm->part[im], t, sd.last_b_off, sd.last_bias, wsdf) / sd.scale;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Workgroup form of the fine kernel (its default for networks of 5 .. 8 tiles; the SDF-only entry measured slower on it than on its
// four-image form and keeps that: profiles/neus_wg_ab.json):
// TWO 32-point images per 256-thread workgroup, every layer IN PLACE (gemm_tiles2_in_place), so an image is its E rows
// (no more than the embedding and the colour extras fill) plus ONE 4 max_tiles-row activation buffer, 37 KB at the shipped shape, and
// TWO INDEPENDENT workgroups share a CU: the two waves of a SIMD belong to different workgroups in unrelated phases, one's epilogues,
// barrier waits and VALU-only phases under the other's K loops, where the 512-thread forms above run them in lockstep with the matrix
// pipe empty.  A weight fragment still feeds both images (8 MFMAs per fetched float4: the L2 weight stream of the two-image form).
// max_tiles <= 8: a wave holds tiles w and w + 4.  Per point the arithmetic and its order are those of neus_points2_kernel, the
// embedding-gradient GEMMs included (wte_split_k's K slices: a fresh accumulator per slice, the partials added in slice order in
// registers -- there are no parking rows in place --, then the E rows).
struct SmallsW {             // Smalls<2> with the row-dot partials of four waves, not eight
  float pts[2][96], dirs[2][96], part[2][384], grad[2][96];
};

__device__ __forceinline__ void wte_in_place(f32x4* __restrict__ lds, const int IS, const int k_row0, const int ng,
                                             const f32x4* __restrict__ w, const int emb_tiles, const int KS, const int e_row0,
                                             const int e_rows, const bool accumulate, const int wave, const int lane) {
  const int gk = (ng + KS - 1) / KS;
  for (int u = wave; u < 2 * emb_tiles; u += 4) {                     // (tile, image) units; no barrier in here
    const int t = u % emb_tiles;
    f32x4* li = lds + (size_t)(u / emb_tiles) * IS;
    const f32x4* __restrict__ wp = w + (size_t)t * ng * 64 + lane;
    f32x16 sum;
    for (int k = 0; k < KS; ++k) {
      f32x16 acc;
      init_zero(acc);
      const int g0 = k * gk, g1 = min(ng, g0 + gk);
      for (int g = g0; g < g1; g += 8) {
        f32x4 a[8], b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int gg = min(g + i, ng - 1);
          a[i] = wp[gg * 64]; b[i] = li[(k_row0 + gg) * 64 + lane];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (g + i < g1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][j], b[i][j], acc, 0, 0, 0);
          }
      }
      if (k == 0) sum = acc; else sum += acc;
    }
#pragma unroll
    for (int rq = 0; rq < 4; ++rq)
      if (t * 4 + rq < e_rows) {                                       // (rows past the last embedding feature are never read)
        f32x4 v = acc_quad(sum, rq);
        if (accumulate) v += li[(e_row0 + t * 4 + rq) * 64 + lane];
        li[(e_row0 + t * 4 + rq) * 64 + lane] = v;
      }
  }
}

template <bool FOLD>
__global__ __launch_bounds__(256, 2) void neus_points2w_kernel(
    const SdfDesc sd, const ColDesc cd, const f32x4* __restrict__ wsdf, const f32x4* __restrict__ wcol,
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ zv,
    const float* __restrict__ pts_direct, const float* __restrict__ dirs_direct, const long P, const int S,
    f32x4* __restrict__ scratch, float* __restrict__ out_sdf, float* __restrict__ out_grad,
    float* __restrict__ out_rgb) {
  extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
  const int MT = sd.max_tiles;
  const int X0 = max(sd.emb_rows, cd.extra_rows);
  const int IS = (X0 + 4 * MT) * 64;
  SmallsW* sm = reinterpret_cast<SmallsW*>(lds + (size_t)2 * IS);
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, p = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_lin = sd.n_lin;
  const int emb_tiles = (sd.emb_feats + 31) >> 5;
  const int ks_wte = min(8, MT) / emb_tiles;             // wte_split_k's K slices
  const long n_tiles = (P + 31) >> 5, n_pairs = (n_tiles + 1) >> 1;
  const size_t per_img = (size_t)(n_lin - 1) * 4 * MT * 64;
  f32x4* save0 = scratch + (size_t)blockIdx.x * 2 * per_img;
  const int feat_slot = (n_lin - 2) * 4 * MT;
  f32x4 nopre[4];

  for (long pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
    // ---------------- points of both tiles, positional encoding -> E rows ----------------
    if (tid < 64) {
      const int im = tid >> 5, t = tid & 31;
      load_point<true>(((2 * pair + im) << 5) + t, P, S, rays_o, rays_d, zv, pts_direct, dirs_direct, sm->pts[im] + t * 3, sm->dirs[im] + t * 3);
    }
    __syncthreads();
    for (int u = wave; u < 2 * sd.emb_rows; u += 4) {                 // (image, embedding row) units
      const int im = u / sd.emb_rows, r = u - im * sd.emb_rows;
      const float xs = sm->pts[im][p * 3 + 0] * sd.scale, ys = sm->pts[im][p * 3 + 1] * sd.scale, zs = sm->pts[im][p * 3 + 2] * sd.scale;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = emb_feat(row_feat(r, h, j), sd.emb_feats, xs, ys, zs);
      lds[(size_t)im * IS + (E0 + r) * 64 + lane] = v;
    }
    __syncthreads();

    // ---------------- SDF hidden layers, in place ----------------
    for (int l = 0; l < n_lin - 1; ++l) {
      const LayerDesc L = sd.layers[l];
      const KSegs ks = (l == 0) ? KSegs{E0, sd.emb_rows, 0, 0}
                                : KSegs{X0, 4 * sd.layers[l - 1].n_out_tiles, E0, (l == sd.skip) ? sd.emb_rows : 0};
      const bool do_save = l < n_lin - 2;
      const f32x4* bp = wsdf + L.b_off;
      gemm_tiles2_in_place(lds, IS, ks, wsdf + L.w_off, L.n_out_tiles, wave, lane, X0,
                           [&](int ot, int, f32x16& acc) { init_bias(bp, ot, lane, acc); },
                           [&](int ot, int im, int rq, f32x4& v) {
#pragma unroll
                             for (int j = 0; j < 4; ++j) v[j] = act_fwd<ACT_SOFTPLUS100>(v[j]);
                             if (do_save) st_stream(save0 + (size_t)im * per_img + (size_t)l * 4 * MT * 64 + (ot * 4 + rq) * 64 + lane, v);
                           });
    }
    const int hid_rows = 4 * sd.layers[n_lin - 2].n_out_tiles;

    // ---------------- last layer: sdf row (VALU dot, per image) [+ feature rows, or the folded colour input, -> stash] ----------------
    for (int im = 0; im < 2; ++im) rowdot<1>(lds + (size_t)im * IS, X0, hid_rows, wsdf + sd.last_w_off, sm->part[im], wave, lane);
    if (sd.layers[n_lin - 1].n_out_tiles > 0) {
      const LayerDesc L = sd.layers[n_lin - 1];
      const f32x4* bp = FOLD ? wcol + cd.reserved2 : wsdf + L.b_off;
      gemm_tiles2<4>(lds, IS, KSegs{X0, hid_rows, 0, 0}, FOLD ? wcol + cd.reserved1 : wsdf + L.w_off,
                     FOLD ? cd.layers[0].n_out_tiles : L.n_out_tiles, wave, lane, nopre, false, nullptr,
                     [&](int ot, int, f32x16& acc) { init_bias(bp, ot, lane, acc); },
                     [&](int ot, int im, int rq, const f32x16& acc) {
                       st_stream(save0 + (size_t)im * per_img + (size_t)feat_slot * 64 + (ot * 4 + rq) * 64 + lane, acc_quad(acc, rq));
                     });
    }
    __syncthreads();
    if (tid < 64) {
      const int im = tid >> 5, t = tid & 31;
      const long pt = ((2 * pair + im) << 5) + t;
      if (pt < P) out_sdf[pt] = sdf_raw(sm->part[im], t, sd.last_b_off, sd.last_bias, wsdf) / sd.scale;
    }
    // ---------------- reverse sweep: d sdf / d x ----------------
    // G_pre(last hidden) = w_sdf_row (.) act'(h), in place
    for (int im = 0; im < 2; ++im) {
      f32x4* li = lds + (size_t)im * IS;
      for (int r0 = wave; r0 < hid_rows; r0 += 32) {            // 8 rows per pass: all fetches first (one L2 round trip per pass)
        f32x4 v[8], wv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int r = min(r0 + 4 * c, hid_rows - 1);
          v[c] = li[(X0 + r) * 64 + lane];
          wv[c] = wsdf[sd.last_w_off + r * 2 + h];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (r0 + 4 * c < hid_rows) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[c][j] = wv[c][j] * act_bwd_from_out<ACT_SOFTPLUS100>(v[c][j]);
            li[(X0 + r0 + 4 * c) * 64 + lane] = v[c];
          }
      }
    }
    __syncthreads();
    for (int l = n_lin - 2; l >= 1; --l) {
      const LayerDesc L = sd.layers[l];
      if (l == sd.skip)                                 // the embedding part of the skip layer reads the same rows: before they are overwritten
        wte_in_place(lds, IS, X0, 4 * L.n_out_tiles, wsdf + L.wTE_off, emb_tiles, ks_wte, E0, sd.emb_rows, false, wave, lane);
      f32x4 hv[2][4];                                   // the stashed forward activations of a tile: requested before its K loop
      gemm_tiles2_in_place(lds, IS, KSegs{X0, 4 * L.n_out_tiles, 0, 0}, wsdf + L.wT_off, sd.layers[l - 1].n_out_tiles, wave, lane, X0,
                           [&](int ot, int im, f32x16& acc) {
                             const f32x4* sv = save0 + (size_t)im * per_img + (size_t)(l - 1) * 4 * MT * 64;
#pragma unroll
                             for (int rq = 0; rq < 4; ++rq) hv[im][rq] = ld_stream(sv + (ot * 4 + rq) * 64 + lane);
                             init_zero(acc);
                           },
                           [&](int, int im, int rq, f32x4& v) {
#pragma unroll
                             for (int j = 0; j < 4; ++j) v[j] *= act_bwd_from_out<ACT_SOFTPLUS100>(hv[im][rq][j]);
                           });
    }
    wte_in_place(lds, IS, X0, 4 * sd.layers[0].n_out_tiles, wsdf + sd.layers[0].wTE_off, emb_tiles, ks_wte, E0, sd.emb_rows, sd.skip >= 1,
                 wave, lane);
    __syncthreads();
    // chain through the embedding: thread (image, point pp, component c) sums its features in a fixed order
    if (tid < 192) {
      const int im = tid / 96, r = tid - 96 * im, pp = r & 31, c = r >> 5;
      const f32x4* li = lds + (size_t)im * IS;
      const float g = embed_chain([&](int f) { return lds_feat(li, E0, f, pp); }, c, sd.multires, sm->pts[im] + pp * 3, sd.scale);
      sm->grad[im][pp * 3 + c] = g;
      const long pt = ((2 * pair + im) << 5) + pp;
      if (pt < P) out_grad[pt * 3 + c] = g;
    }
    __syncthreads();
    if (cd.n_lin == 0) continue;          // SDFNetwork.gradient(): no colour net (the same for every wave: a kernel argument)

    // ---------------- colour network, in place ----------------
    const int feat_rows = 4 * sd.layers[n_lin - 1].n_out_tiles;
    for (int im = 0; im < 2; ++im) {
      f32x4* li = lds + (size_t)im * IS;
      const float px = sm->pts[im][p * 3 + 0], py = sm->pts[im][p * 3 + 1], pz = sm->pts[im][p * 3 + 2];
      const float dx = sm->dirs[im][p * 3 + 0], dy = sm->dirs[im][p * 3 + 1], dz = sm->dirs[im][p * 3 + 2];
      for (int r = wave; r < cd.extra_rows; r += 4) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = col_extra_feat(row_feat(r, h, j), px, py, pz, dx, dy, dz, sm->grad[im] + p * 3, cd.n_view_feats, cd.extra_feats);
        li[(E0 + r) * 64 + lane] = v;
      }
      const f32x4* sv = save0 + (size_t)im * per_img + (size_t)feat_slot * 64;
      for (int r0 = wave; r0 < (FOLD ? 0 : feat_rows); r0 += 32) {          // (unfolded) the feature rows back from the stash
        f32x4 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = ld_stream(sv + min(r0 + 4 * c, feat_rows - 1) * 64 + lane);
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (r0 + 4 * c < feat_rows) li[(X0 + r0 + 4 * c) * 64 + lane] = v[c];
      }
    }
    __syncthreads();
    int in_rows = feat_rows;
    auto relu = [&](int, int, int, f32x4& v) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = act_fwd<ACT_RELU>(v[j]);
    };
    if (FOLD) {                                   // colour layer 0 = relu(P + Wc0[:, extras] . extras): K = the extras rows only
      const LayerDesc L = cd.layers[0];
      gemm_tiles2_in_place(lds, IS, KSegs{E0, cd.extra_rows, 0, 0}, wcol + cd.reserved3, L.n_out_tiles, wave, lane, X0,
                           [&](int ot, int im, f32x16& acc) {
                             const f32x4* pp = save0 + (size_t)im * per_img + (size_t)feat_slot * 64 + ot * 256 + lane;
#pragma unroll
                             for (int rq = 0; rq < 4; ++rq) {
                               const f32x4 v = ld_stream(pp + rq * 64);
                               acc[4 * rq + 0] = v[0]; acc[4 * rq + 1] = v[1]; acc[4 * rq + 2] = v[2]; acc[4 * rq + 3] = v[3];
                             }
                           },
                           relu);
      in_rows = 4 * L.n_out_tiles;
    }
    for (int l = FOLD ? 1 : 0; l < cd.n_lin - 1; ++l) {
      const LayerDesc L = cd.layers[l];
      const f32x4* bp = wcol + L.b_off;
      gemm_tiles2_in_place(lds, IS, KSegs{X0, in_rows, E0, l == 0 ? cd.extra_rows : 0}, wcol + L.w_off, L.n_out_tiles, wave, lane, X0,
                           [&](int ot, int, f32x16& acc) { init_bias(bp, ot, lane, acc); }, relu);
      in_rows = 4 * L.n_out_tiles;
    }
    for (int im = 0; im < 2; ++im) rowdot<3>(lds + (size_t)im * IS, X0, in_rows, wcol + cd.last_w_off, sm->part[im], wave, lane);
    __syncthreads();
    if (tid < 192) {
      const int im = tid / 96, r = tid - 96 * im, pp = r & 31, o = r >> 5;
      const float v = rgb_out(sm->part[im], pp, o, cd.last_b_off, cd.last_bias[o], cd.squeeze_out, wcol);
      const long pt = ((2 * pair + im) << 5) + pp;
      if (pt < P) out_rgb[pt * 3 + o] = v;
    }
    __syncthreads();
  }
}


int check_sdf_desc(const SdfDesc& d) {
  if (d.n_lin < 2 || d.n_lin > VQN_MAX_SDF_LAYERS) return 1;
  if (d.max_tiles < 1 || d.max_tiles > 16) return 2;
  if (d.emb_feats < 3 || d.emb_feats > 64 || d.emb_rows < 1 || d.emb_rows > 8) return 3;
  if (d.skip >= d.n_lin - 1 || d.skip == 0) return 4;
  for (int l = 0; l < d.n_lin; ++l)
    if (d.layers[l].n_out_tiles < 0 || d.layers[l].n_out_tiles > d.max_tiles) return 5;
  if (!(d.scale > 0.f)) return 6;
  return 0;
}

template <int NIMG>
size_t lds_bytes(int MT) { return (size_t)NIMG * (E_ROWS + 8 * MT) * 1024 + sizeof(Smalls<NIMG>); }

// two 32-point images per workgroup for networks wide enough to give eight waves a tile each (and small enough to fit),
// unless VQN_NEUS_TILE32 is set
bool use_two_images(int MT) {
  static const bool forced32 = getenv("VQN_NEUS_TILE32") != nullptr;
  return !forced32 && MT >= 5 && lds_bytes<2>(MT) <= 160 * 1024;
}

template <int NIMG>
size_t lds_bytes_sdf(const SdfDesc& sd) { return (size_t)NIMG * (sd.emb_rows + 4 * sd.max_tiles) * 1024 + sizeof(SmallsSdf<NIMG>); }

// Images per workgroup of the SDF-only entry: the most of {4, 3} that fit the 160 KB of LDS (neus_pointsN_kernel: 5 <= max_tiles <= 8,
// one output tile per wave), else the two-image or one-image form as before.  VQN_NEUS_SDF_IMAGES=2|3|4 (read once) caps the count for
// A/B runs and tests; a count that does not fit falls back to the next smaller form.
constexpr int SDF_IMAGES_DEFAULT = 4;
int sdf_images(const SdfDesc& sd) {
  static const int cap = [] {
    const char* e = getenv("VQN_NEUS_SDF_IMAGES");
    const int v = e != nullptr ? atoi(e) : SDF_IMAGES_DEFAULT;
    return v >= 2 && v <= 4 ? v : SDF_IMAGES_DEFAULT;
  }();
  if (!use_two_images(sd.max_tiles)) return 1;
  if (sd.max_tiles <= 8) {
    if (cap >= 4 && lds_bytes_sdf<4>(sd) <= 160 * 1024) return 4;
    if (cap >= 3 && lds_bytes_sdf<3>(sd) <= 160 * 1024) return 3;
  }
  return 2;
}

template <int NIMG>
int launch_sdf_images(const char* fn, const SdfDesc& sd, const f32x4* ws, const float* rays_o, const float* rays_d, const float* z,
                      const float* pts, const int64_t P, const int S, float* out_sdf, void* stream) {
  return vqn_launch(fn, neus_pointsN_kernel<NIMG>, pair_grid((P + 31) / 32, NIMG, 1, 0, 0), 512, lds_bytes_sdf<NIMG>(sd), stream, sd, ws,
                    rays_o, rays_d, z, pts, (long)P, S, out_sdf);
}

// ---- the workgroup form (neus_points2w_kernel): two in-place two-image workgroups on a CU
size_t lds_bytes_wg(const SdfDesc& sd, const int extra_rows) {
  return (size_t)2 * ((sd.emb_rows > extra_rows ? sd.emb_rows : extra_rows) + 4 * sd.max_tiles) * 1024 + sizeof(SmallsW);
}

// The workgroup form for this network?  Where the two-image form would run, max_tiles <= 8 and the LDS holds two workgroups; else the
// two-image form as before.  VQN_NEUS_FORM=images (read once) keeps the two-image form everywhere: for A/B runs and tests, like
// VQN_NEUS_SDF_IMAGES and VQN_NEUS_TILE32 (which keeps the ping-pong one-image form).
bool use_wg_form(const SdfDesc& sd, const int extra_rows) {
  static const bool images = [] {
    const char* e = getenv("VQN_NEUS_FORM");
    return e != nullptr && strcmp(e, "images") == 0;
  }();
  return !images && use_two_images(sd.max_tiles) && sd.max_tiles <= 8 && 2 * lds_bytes_wg(sd, extra_rows) <= 160 * 1024;
}

bool extras_rows_ok(const ColDesc& cd) { return cd.extra_rows >= 1 && cd.extra_rows <= 8; }

}  // namespace

extern "C" int vqn_neus_sdf_points(const int32_t* sdf_desc, const float* wbuf_sdf, const float* rays_o,
                                   const float* rays_d, const float* z, const float* pts, int64_t P, int S,
                                   float* out_sdf, void* stream) {
  SdfDesc sd;
  const int rc = neus_sdf_args(__func__, sdf_desc, wbuf_sdf, rays_o, rays_d, z, pts, P, S, out_sdf, check_sdf_desc,
                               "invalid SDF network descriptor", &sd);
  if (rc != VQN_OK || P == 0) return rc;
  ColDesc cd;
  memset(&cd, 0, sizeof(cd));
  const long n_tiles = (P + 31) / 32;
  const f32x4* ws = reinterpret_cast<const f32x4*>(wbuf_sdf);
  const int images = sdf_images(sd);
  if (images == 4) return launch_sdf_images<4>(__func__, sd, ws, rays_o, rays_d, z, pts, P, S, out_sdf, stream);
  if (images == 3) return launch_sdf_images<3>(__func__, sd, ws, rays_o, rays_d, z, pts, P, S, out_sdf, stream);
  if (images == 2)
    return vqn_launch(__func__, neus_points2_kernel<false>, pair_grid(n_tiles, 2, 1, 0, 0), 512, lds_bytes<2>(sd.max_tiles), stream, sd, cd, ws,
                      nullptr, rays_o, rays_d, z, pts, nullptr, (long)P, S, nullptr, out_sdf, nullptr, nullptr, TrainOut{});
  const size_t lds = lds_bytes<1>(sd.max_tiles);
  VQN_CHECK_SHAPE(lds <= 160 * 1024, "network too wide for LDS");
  return vqn_launch(__func__, neus_points_kernel<false>, pair_grid(n_tiles, 1, 2, 0, 0), 256, lds, stream, sd, cd, ws, nullptr, rays_o, rays_d,
                    z, pts, nullptr, (long)P, S, nullptr, out_sdf, nullptr, nullptr);
}

// Training forward: vqn_neus_fine_points at explicit (pts, dirs) that ALSO writes the saved tensors of the training engine (see
// TrainOut in neus_phases.h).  tensors: device pointers in the order [E, OUTF, EXTR, U_1..U_nL, GH_0..GH_{nL-1}, C_1..C_nC] with nL = n_lin - 1
// SDF hidden layers and nC = col n_lin - 1 colour hidden layers; each [ceil(P/32)][tiles][32][32] f32 with tiles = ceil(width / 32)
// (e_tiles / outf_tiles / extr_tiles given, the others from the descriptors).  Needs the two-image form (networks of >= 5 tiles that fit).
extern "C" int vqn_neus_train_fwd(const int32_t* sdf_desc, const float* wbuf_sdf, const int32_t* col_desc, const float* wbuf_col,
                                  const float* pts, const float* dirs, int64_t P, void* scratch, int64_t scratch_bytes,
                                  float* const* tensors, int n_tensors, int e_tiles, int outf_tiles, int extr_tiles, float* out_sdf,
                                  float* out_n, float* out_rgb, void* stream) {
  VQN_CHECK_ARG(sdf_desc && wbuf_sdf && col_desc && wbuf_col && pts && dirs && scratch && tensors && out_sdf && out_n && out_rgb, "null pointer");
  VQN_CHECK_ARG(P >= 1, "P >= 1");
  SdfDesc sd;
  ColDesc cd;
  memcpy(&sd, sdf_desc, sizeof(SdfDesc));
  memcpy(&cd, col_desc, sizeof(ColDesc));
  VQN_CHECK_SHAPE(check_sdf_desc(sd) == 0, "invalid SDF network descriptor");
  VQN_CHECK_SHAPE(cd.n_lin >= 2 && cd.n_lin <= VQN_MAX_COL_LAYERS && cd.d_out == 3 && sd.layers[sd.n_lin - 1].n_out_tiles >= 1, "colour net");
  VQN_CHECK_SHAPE(use_two_images(sd.max_tiles), "the training forward kernel is the two-image form only");
  const int nL = sd.n_lin - 1, nC = cd.n_lin - 1;
  VQN_CHECK_ARG(n_tensors == 3 + 2 * nL + nC, "tensors: [E, OUTF, EXTR, U_1..U_nL, GH_0..GH_{nL-1}, C_1..C_nC]");
  VQN_CHECK_SHAPE(e_tiles * 4 >= sd.emb_rows && e_tiles <= 2 && extr_tiles * 4 >= cd.extra_rows && extr_tiles <= 2 &&
                  outf_tiles >= sd.layers[sd.n_lin - 1].n_out_tiles, "tile counts");   // (outf_tiles = ceil(F / 32): with F - 1 no multiple of 32
                  // that is the features' own tile count, and row 32 outf_tiles -- padding past the last feature -- is not stored, see the kernel)
  for (int i = 0; i < n_tensors; ++i) VQN_CHECK_ARG(tensors[i] != nullptr, "null tensor pointer");
  const long grid = pair_grid((P + 31) / 32, 2, 1, neus_stash_bytes(sd), scratch_bytes);
  VQN_CHECK_ARG(grid >= 1, "scratch too small (see vqn_neus_fine_scratch_bytes)");
  return vqn_launch(__func__, neus_points2_kernel<true, true>, grid, 512, lds_bytes<2>(sd.max_tiles), stream, sd, cd,
                    reinterpret_cast<const f32x4*>(wbuf_sdf), reinterpret_cast<const f32x4*>(wbuf_col), nullptr, nullptr, nullptr, pts, dirs,
                    (long)P, 1, reinterpret_cast<f32x4*>(scratch), out_sdf, out_n, out_rgb,
                    neus_train_out(tensors, nL, nC, e_tiles, outf_tiles, extr_tiles));
}

extern "C" int64_t vqn_neus_fine_scratch_bytes(const int32_t* sdf_desc) {
  if (!sdf_desc) return -1;
  SdfDesc sd;
  memcpy(&sd, sdf_desc, sizeof(SdfDesc));
  // (descriptors of every engine: the x3 packs count 3 rows per 16 embedding features, up to 12)
  const int emb_rows = sd.emb_rows;
  if (emb_rows >= 1 && emb_rows <= 12) sd.emb_rows = 1;
  if (check_sdf_desc(sd) != 0) return -2;
#ifdef VQN_DIAG_STASH_ROT
  return (int64_t)VQN_DIAG_STASH_ROT * vqn_num_cus() * 2 * neus_stash_bytes(sd);
#else
  // (two images per workgroup; the workgroup form keeps two workgroups on a CU, the others one: never less than before.  Asked
  // without a colour net, so for the narrowest E rows: room for the workgroup form whenever some launch on this network may take it)
  return (int64_t)vqn_num_cus() * (use_wg_form(sd, 0) ? 4 : 2) * neus_stash_bytes(sd);
#endif
}

extern "C" int vqn_neus_fine_points(const int32_t* sdf_desc, const float* wbuf_sdf, const int32_t* col_desc,
                                    const float* wbuf_col, const float* rays_o, const float* rays_d, const float* z,
                                    const float* pts, const float* dirs, int64_t P, int S, void* scratch,
                                    int64_t scratch_bytes, float* out_sdf, float* out_grad, float* out_rgb,
                                    void* stream) {
  SdfDesc sd;
  ColDesc cd;
  const int rc = neus_fine_args(__func__, sdf_desc, wbuf_sdf, col_desc, wbuf_col, rays_o, rays_d, z, pts, dirs, P, S, scratch, out_sdf,
                                out_grad, out_rgb, check_sdf_desc, "invalid SDF network descriptor", extras_rows_ok, &sd, &cd);
  if (rc != VQN_OK || P == 0) return rc;
  if (cd.n_lin != 0)       // a folded colour pack (vqn_neus_fold_pack) announces its three blocks together; 0 = not folded
    VQN_CHECK_ARG((cd.reserved1 > 0 && cd.reserved2 > cd.reserved1 && cd.reserved3 > cd.reserved2) ||
                  (cd.reserved1 == 0 && cd.reserved2 == 0 && cd.reserved3 == 0), "col_desc: fold offsets (reserved1..3) inconsistent");
  const long n_tiles = (P + 31) / 32;
  const int64_t per_img = neus_stash_bytes(sd);
  const f32x4* ws = reinterpret_cast<const f32x4*>(wbuf_sdf);
  const f32x4* wc = reinterpret_cast<const f32x4*>(wbuf_col);
  if (use_wg_form(sd, cd.extra_rows)) {
    const bool fold = cd.n_lin != 0 && cd.reserved1 > 0;
    const long grid = pair_grid(n_tiles, 2, 2, per_img, scratch_bytes);
    VQN_CHECK_ARG(grid >= 1, "scratch too small (see vqn_neus_fine_scratch_bytes)");
    return vqn_launch(__func__, fold ? neus_points2w_kernel<true> : neus_points2w_kernel<false>, grid, 256,
                      lds_bytes_wg(sd, cd.extra_rows), stream, sd, cd, ws, wc, rays_o, rays_d, z, pts, dirs, (long)P, S,
                      reinterpret_cast<f32x4*>(scratch), out_sdf, out_grad, out_rgb);
  }
  if (use_two_images(sd.max_tiles)) {
    const bool fold = cd.n_lin != 0 && cd.reserved1 > 0;
#ifdef VQN_DIAG_STASH_ROT
    const long grid = pair_grid(n_tiles, 2, 1, 0, 0);
    VQN_CHECK_ARG((int64_t)VQN_DIAG_STASH_ROT * grid * 2 * per_img <= scratch_bytes, "diag build: scratch must hold ROT regions per workgroup");
#else
    const long grid = pair_grid(n_tiles, 2, 1, per_img, scratch_bytes);
#endif
    VQN_CHECK_ARG(grid >= 1, "scratch too small (see vqn_neus_fine_scratch_bytes)");
    return vqn_launch(__func__, fold ? neus_points2_kernel<true, false, true> : neus_points2_kernel<true>, grid, 512, lds_bytes<2>(sd.max_tiles),
                      stream, sd, cd, ws, wc, rays_o, rays_d, z, pts, dirs, (long)P, S, reinterpret_cast<f32x4*>(scratch), out_sdf, out_grad,
                      out_rgb, TrainOut{});
  }
  const size_t lds = lds_bytes<1>(sd.max_tiles);
  VQN_CHECK_SHAPE(lds <= 160 * 1024, "network too wide for LDS");
  const long grid = pair_grid(n_tiles, 1, 2, per_img, scratch_bytes);
  VQN_CHECK_ARG(grid >= 1, "scratch too small (see vqn_neus_fine_scratch_bytes)");
  return vqn_launch(__func__, neus_points_kernel<true>, grid, 256, lds, stream, sd, cd, ws, wc, rays_o, rays_d, z, pts, dirs, (long)P, S,
                    reinterpret_cast<f32x4*>(scratch), out_sdf, out_grad, out_rgb);
}
