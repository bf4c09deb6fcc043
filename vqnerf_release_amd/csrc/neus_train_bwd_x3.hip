// vqn_neus_train_bwd on the exact-split engine (csrc/mlp_prims_x3.h): the same backward pass as csrc/neus_train_bwd.hip -- colour
// backward, tangent pass, reverse sweep with the second-order sources, one launch -- with every layer GEMM as six bf16 MFMAs per
// product over bf16 piece triples (products exact to 2^-24, f32 accumulation), the layers in place in one activation buffer (one
// output tile per wave, finished tiles parked in registers across the barrier), weights streamed through the engine's ring along
// a table of the pass's GEMM calls.  What it stands for in the reference: loss.backward() through renderer.py:216-227 under
// exp_runner.py:153-168.  Adjoints in and saved tensors in / out are the f32 ones of the f32 kernel (tile format, same contract).
//
// Also here: vqn_pack_x3_gather, the weight pack of this kernel in one launch (gather from the flat parameter vector + the exact
// three-way split of every gathered value into bf16 pieces, geo/packing.py: split_pack_x3).
#include "x3_calls.h"
#include "neus_launch.h"
#include "vqnerf_hip.h"
#include <stdlib.h>

using namespace eng;
using namespace eng::x3;

namespace {


struct SmallsB {
  float pts[2][96], dout[2][96], gn[2][96], v[2][96], gs[2][32], part[2][512];
  CallTab calls;               // GEMM calls of one tile pair (x3_calls.h)
};

template <int NACC>
__global__ __launch_bounds__(512, 1) void neus_train_bwd_x3_kernel(const TrainBwdDesc bd, const f32x4* __restrict__ wx, const f32x4* __restrict__ wf,
                                                                   const TrainBwdPtrs tp, const long P, f32x4* __restrict__ scratch) {
  extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
  const int MT = bd.max_tiles;
  const int IMG = E_ROWS + 6 * MT, IS = IMG * 64;
  SmallsB* sm = reinterpret_cast<SmallsB*>(lds + (size_t)2 * IS);
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, p = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int img = wave >> 2, w4 = wave & 3;
  f32x4* ldsi = lds + (size_t)img * IS;
  const int nL = bd.nL, nC = bd.nC;
  const long n_tiles = (P + 31) >> 5, n_pairs = (n_tiles + 1) >> 1;
  const size_t per_img = (size_t)(nL + 1) * 4 * MT * 64;           // stash: S_0..S_{nL-1}, g_feat (accumulator-order quads)
  f32x4* save0 = scratch + (size_t)blockIdx.x * 2 * per_img;
  const int feat_slot = nL * 4 * MT;

  // ---------------- the pass's GEMM calls, in order (the weight stream follows this table) ----------------
  if (tid == 0) {
    int n = 0;
    auto add = [&](int off, int krows, int tiles) { add_call(&sm->calls, n, off, 0, krows, tiles); };
    for (int l = nC; l >= 1; --l) add(bd.offCB[l], l == nC ? 3 : 6 * bd.tc[l], bd.tc[l - 1]);
    add(bd.offCBfeat, 6 * bd.tc[0], bd.feat_tiles);
    for (int l = 0; l < nL; ++l) add(bd.offT[l], l == 0 ? bd.emb_rows : 6 * bd.ts[l - 1] + (l == bd.skip ? bd.emb_rows : 0), bd.ts[l]);
    add(bd.offBtop, 6 * bd.feat_tiles, bd.ts[nL - 1]);
    for (int l = nL - 1; l >= 1; --l) add(bd.offB[l], 6 * bd.ts[l], bd.ts[l - 1]);
    sm->calls.n_calls = n;
  }
  __syncthreads();
  const int n_calls = __builtin_amdgcn_readfirstlane(sm->calls.n_calls);
  f32x4 ring[RING][6];
  prime_stream(&sm->calls, n_calls, wx, wx, lane, [&](int) { return wave; }, ring);
  int call = 0;
  // a GEMM call, and one whose output goes over its own input (a layer in place): x3_calls.h
  auto G = [&](const f32x4* wbase, const KSegs ks, const int tiles, auto init, auto epi) {
    gemm_call2<NACC, false>(&sm->calls, n_calls, call, wx, wx, lds, IS, ks, wbase, tiles, wave, lane, ring, init, epi);
  };
  auto GC = [&](const f32x4* wbase, const KSegs ks, const int tiles, auto init, auto epi) {
    gemm_call2<NACC, true>(&sm->calls, n_calls, call, wx, wx, lds, IS, ks, wbase, tiles, wave, lane, ring, init, epi);
  };
  // epilogue operands of this wave's tile, both images, requested right before the K loop.  (The f32 kernel's refinement -- the NEXT GEMM's
  // operands requested in place from inside the current epilogue -- measured slower here: 6.80 -> 7.19 ms, 39 -> 99 spilled VGPRs: the
  // operands would live across commit() and the ring refills, and this engine has no registers to spare.  Requesting them half way through
  // the K loop instead (a hook inside gemm_tiles_x3_ring2): 6.7 -> 7.0 ms, 39 -> 91 spilled VGPRs -- the same verdict.)
  float au[2][16], ab[2][16];

  for (long pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
    call = 0;
    const long ptile_w = 2 * pair + img;
    const bool live_w = ptile_w < n_tiles;
    // ---------------- points and incoming adjoints of both tiles ----------------
    if (tid < 64) {
      const int im = tid >> 5, t = tid & 31;
      const long pt = ((2 * pair + im) << 5) + t;
      const bool valid = pt < P;
      const long q = valid ? pt : P - 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sm->pts[im][t * 3 + c] = tp.X[q * 3 + c];
        float d = 0.f;
        if (valid) {
          d = tp.G_RGB[pt * 3 + c];
          if (tp.RGB != nullptr) { const float y = tp.RGB[pt * 3 + c]; d = d * y * (1.0f - y); }
        }
        sm->dout[im][t * 3 + c] = d;
        sm->gn[im][t * 3 + c] = (valid && tp.G_N != nullptr) ? tp.G_N[pt * 3 + c] : 0.f;
      }
      sm->gs[im][t] = (valid && tp.G_SDF != nullptr) ? tp.G_SDF[pt] * bd.inv_scale : 0.f;
    }
    __syncthreads();
    if (w4 < 2) {                                            // delta_nC: one K step in the E rows; DC_nC is one feature tile = two steps
      float x[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int f = step_feat(w4, h, jj);
        x[jj] = f < 3 ? sm->dout[img][p * 3 + f] : 0.f;
      }
      if (live_w) tfmt_store_step(tp.DC[nC], ptile_w, 1, w4, lane, x);
      if (w4 == 0) {
        f32x4 q0, q1, q2;
        split3x8(x, q0, q1, q2);
        ldsi[(E0 + 0) * 64 + lane] = q0; ldsi[(E0 + 1) * 64 + lane] = q1; ldsi[(E0 + 2) * 64 + lane] = q2;
      }
    }
    __syncthreads();

    // ---------------- colour network backward (in place) ----------------
    for (int l = nC; l >= 1; --l) {
      const KSegs ks = (l == nC) ? KSegs{E0, 3, 0, 0} : KSegs{X0, 6 * bd.tc[l], 0, 0};
      const int n_ot = bd.tc[l - 1];
      const float* const t_c = tp.C[l];
      float* const t_dc = tp.DC[l - 1];
      GC(wx + bd.offCB[l], ks, n_ot,
        [&](int ot, auto im_c, f32x16& acc) __attribute__((always_inline)) {
          constexpr int im = decltype(im_c)::value; (void)im;
          if (2 * pair + im < n_tiles) tfmt_load_acc(t_c, 2 * pair + im, n_ot, ot, lane, au[im]);
          else {
#pragma unroll
            for (int i = 0; i < 16; ++i) au[im][i] = 0.f;
          }
          init_zero(acc);
        },
        [&](int ot, auto im_c, const f32x16& acc) __attribute__((always_inline)) {
          constexpr int im = decltype(im_c)::value; (void)im;
          float v[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) v[i] = acc[i] * act_bwd_from_out<ACT_RELU>(au[im][i]);
          if (2 * pair + im < n_tiles) tfmt_store_acc(t_dc, 2 * pair + im, n_ot, ot, lane, v);
          store_tile_x3(lds + (size_t)im * IS, X0 + 6 * ot, lane, v);
        });
    }
    {
      const int in_rows = 6 * bd.tc[0];
      rowdot_x3<3>(ldsi, X0, in_rows, wf + bd.offCBnrm, sm->part[img], w4, lane);
      G(wx + bd.offCBfeat, KSegs{X0, in_rows, 0, 0}, bd.feat_tiles,
        [&](int, auto, f32x16& acc) __attribute__((always_inline)) { init_zero(acc); },
        [&](int ot, auto im_c, const f32x16& acc) __attribute__((always_inline)) {
          constexpr int im = decltype(im_c)::value; (void)im;
          f32x4* sv = save0 + (size_t)im * per_img + (size_t)feat_slot * 64;
#pragma unroll
          for (int q = 0; q < 4; ++q) st_stream(sv + (ot * 4 + q) * 64 + lane, (f32x4){acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]});
          if (2 * pair + im < n_tiles) {                     // GOUTF = [0 ; d features]: feature f is row f + 1
            float* base = tp.GOUTF + (2 * pair + im) * (long)bd.outf_tiles * 1024;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int f = 32 * ot + (i & 3) + 8 * (i >> 2) + 4 * h + 1;
              if (f < 32 * bd.outf_tiles) __builtin_nontemporal_store(acc[i], base + f * 32 + p);
            }
          }
        });
      __syncthreads();
      if (tid < 192) {
        const int im = tid / 96, r = tid - 96 * im, pp = r & 31, c = r >> 5;
        const float* pr = sm->part[im];
        const float g = (pr[(0 * 32 + pp) * 3 + c] + pr[(1 * 32 + pp) * 3 + c]) + (pr[(2 * 32 + pp) * 3 + c] + pr[(3 * 32 + pp) * 3 + c]);
        sm->v[im][pp * 3 + c] = sm->gn[im][pp * 3 + c] + g;
      } else if (tid < 256) {
        const int im = (tid - 192) >> 5, t = tid & 31;
        if (2 * pair + im < n_tiles) {
          float* base = tp.GOUTF + (2 * pair + im) * (long)bd.outf_tiles * 1024;
          base[t] = sm->gs[im][t];                                        // row 0: d loss / d sdf / scale -- the contraction GOUTF x u_L then
                                                                          // yields row 0 of the last layer's gradient (and its bias) by itself
          for (int f = 32 * bd.feat_tiles + 1; f < 32 * bd.outf_tiles; ++f) base[f * 32 + t] = 0.f;
        }
      }
      __syncthreads();
    }

    // ---------------- tangent pass ----------------
    {
      const float x0 = sm->pts[img][p * 3 + 0] * bd.scale, x1 = sm->pts[img][p * 3 + 1] * bd.scale, x2 = sm->pts[img][p * 3 + 2] * bd.scale;
      const float v0 = sm->v[img][p * 3 + 0], v1 = sm->v[img][p * 3 + 1], v2 = sm->v[img][p * 3 + 2];
      for (int sl = w4; sl < 2 * bd.e_tiles; sl += 4) {
        float x[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int f = step_feat(sl, h, jj);
          float val = 0.f;
          if (sl < bd.emb_rows / 3 && f < bd.emb_feats) {
            int c;
            const float jac = posenc_jac(f, x0, x1, x2, &c);
            val = jac * (c == 0 ? v0 : (c == 1 ? v1 : v2));
          }
          x[jj] = val;
        }
        if (live_w) tfmt_store_step(tp.ED, ptile_w, bd.e_tiles, sl, lane, x);
        if (sl < bd.emb_rows / 3) {
          f32x4 q0, q1, q2;
          split3x8(x, q0, q1, q2);
          ldsi[(E0 + 3 * sl) * 64 + lane] = q0; ldsi[(E0 + 3 * sl + 1) * 64 + lane] = q1; ldsi[(E0 + 3 * sl + 2) * 64 + lane] = q2;
        }
      }
    }
    __syncthreads();
    for (int l = 0; l < nL; ++l) {
      const KSegs ks = (l == 0) ? KSegs{E0, bd.emb_rows, 0, 0} : KSegs{X0, 6 * bd.ts[l - 1], E0, (l == bd.skip) ? bd.emb_rows : 0};
      const int n_ot = bd.ts[l];
      const float* const t_u = tp.U[l + 1];
      const float* const t_gh = tp.GH[l];
      float* const t_ud = tp.UD[l + 1];
      GC(wx + bd.offT[l], ks, n_ot,
        [&](int ot, auto im_c, f32x16& acc) __attribute__((always_inline)) {
          constexpr int im = decltype(im_c)::value; (void)im;
          if (2 * pair + im < n_tiles) {
            tfmt_load_acc(t_u, 2 * pair + im, n_ot, ot, lane, au[im]);
            tfmt_load_acc(t_gh, 2 * pair + im, n_ot, ot, lane, ab[im]);
          } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) { au[im][i] = 0.f; ab[im][i] = 0.f; }
          }
          init_zero(acc);
        },
        [&](int ot, auto im_c, const f32x16& acc) __attribute__((always_inline)) {
          constexpr int im = decltype(im_c)::value; (void)im;
          f32x4* sv = save0 + (size_t)im * per_img + (size_t)l * 4 * MT * 64;
          float v[16], s[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float a = acc[i];
            const float e = fast_exp(-100.f * au[im][i]);
            v[i] = a * (1.f - e);
            s[i] = ab[im][i] * a * (100.f * e);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) st_stream(sv + (ot * 4 + q) * 64 + lane, (f32x4){s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]});
          if (2 * pair + im < n_tiles) tfmt_store_acc(t_ud, 2 * pair + im, n_ot, ot, lane, v);
          store_tile_x3(lds + (size_t)im * IS, X0 + 6 * ot, lane, v);
        });
    }

    // ---------------- reverse sweep ----------------
    {                                                       // g_feat back from the stash (accumulator order) -> piece rows of X
      const f32x4* sv = save0 + (size_t)img * per_img + (size_t)feat_slot * 64;
      for (int t = w4; t < bd.feat_tiles; t += 4) {
        f32x4 q4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) q4[q] = ld_stream(sv + (t * 4 + q) * 64 + lane);
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = q4[i >> 2][i & 3];
        store_tile_x3(ldsi, X0 + 6 * t, lane, v);
      }
    }
    __syncthreads();
    for (int l = nL; l >= 1; --l) {
      const bool top = l == nL;
      const KSegs ks = top ? KSegs{X0, 6 * bd.feat_tiles, 0, 0} : KSegs{X0, 6 * bd.ts[l], 0, 0};
      const int n_ot = bd.ts[l - 1];
      const float* const t_u = tp.U[l];
      float* const t_ab = tp.AB[l - 1];
      const f32x4* const wrow = wf + bd.offWrow;
      GC(wx + (top ? bd.offBtop : bd.offB[l]), ks, n_ot,
        [&](int ot, auto im_c, f32x16& acc) __attribute__((always_inline)) {
          constexpr int im = decltype(im_c)::value; (void)im;
          const f32x4* sv = save0 + (size_t)im * per_img + (size_t)(l - 1) * 4 * MT * 64;
          if (2 * pair + im < n_tiles) tfmt_load_acc(t_u, 2 * pair + im, n_ot, ot, lane, au[im]);
          else {
#pragma unroll
            for (int i = 0; i < 16; ++i) au[im][i] = 0.f;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 t = ld_stream(sv + (ot * 4 + q) * 64 + lane);
            ab[im][4 * q] = t[0]; ab[im][4 * q + 1] = t[1]; ab[im][4 * q + 2] = t[2]; ab[im][4 * q + 3] = t[3];
          }
          if (top) {                                        // the sdf row of the last layer as the rank-1 start value
            init_bias_f16s(wrow, ot, lane, acc);
            const float gs = sm->gs[im][p];
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] *= gs;
          } else init_zero(acc);
        },
        [&](int ot, auto im_c, const f32x16& acc) __attribute__((always_inline)) {
          constexpr int im = decltype(im_c)::value; (void)im;
          float v[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) v[i] = acc[i] * act_bwd_from_out<ACT_SOFTPLUS100>(au[im][i]) + ab[im][i];
          if (2 * pair + im < n_tiles) tfmt_store_acc(t_ab, 2 * pair + im, n_ot, ot, lane, v);
          store_tile_x3(lds + (size_t)im * IS, X0 + 6 * ot, lane, v);
        });
    }
  }
}

size_t lds_bytes_b(int MT) { return (size_t)2 * (E_ROWS + 6 * MT) * 1024 + sizeof(SmallsB); }

// this engine's descriptor rules (the shared ones: train_bwd_load_desc, neus_launch.h); emb_rows counts x3 rows, offT / offB / offCB /
// offBtop / offCBfeat index the piece pack and offWrow / offCBnrm the f32 image buffer
int engine_rules(const TrainBwdDesc& bd) {
  if (bd.max_tiles < 1 || bd.max_tiles > NW || lds_bytes_b(bd.max_tiles) > 160 * 1024) return 2;
  if (bd.emb_feats < 3 || bd.emb_feats > 64 || bd.emb_rows != x3_rows(bd.emb_feats) || bd.emb_rows > E_ROWS || 2 * bd.e_tiles * 3 < bd.emb_rows || bd.e_tiles > 2) return 3;
  if (2 * bd.nL + bd.nC + 2 > MAX_CALLS) return 9;
  return 0;
}

// accumulators per image, as in the forward (csrc/neus_mlp_x3.hip): 2 = a0 w0 apart from the five smaller terms, joined by one rounded add
// per tile; VQN_X3_BWD_NACC=1 selects one.  With one, the small terms meet the large accumulator inside the MFMA, which loses them with a
// one-signed error: the pass is then not odd in its adjoints, and the sums over points of a loss on the colours alone carry a bias that
// grows with the point count (scripts/probe_neus_bwd_x3_bias.py, profiles/neus_train_bwd_x3_bias.json)
int bwd_nacc() {
  static const int n = [] { const char* e = getenv("VQN_X3_BWD_NACC"); return (e && e[0] == '1') ? 1 : 2; }();
  return n;
}

// out[t][q][lane][k] (bf16) = piece q of flat[gidx[t][lane][k]]: t over (tile, K step) of every matrix, 64 lanes x 8 slots per step
// (blocks beyond the piece pack's: the plain f32 gather out_f[i] = flat[fidx[i]] of the thin images -- biases in accumulator order, row-dot
//  images -- that every caller of this pack needs from the same flat vector: one launch for both)
__global__ __launch_bounds__(256) void pack_x3_gather_kernel(const float* __restrict__ flat, const int32_t* __restrict__ gidx, const long n_steps,
                                                             unsigned short* __restrict__ out, const int32_t* __restrict__ fidx, const long n_f,
                                                             float* __restrict__ out_f) {
  const long pack_blocks = (n_steps + 3) / 4;
  if ((long)blockIdx.x >= pack_blocks) {
    const long i = ((long)blockIdx.x - pack_blocks) * 256 + threadIdx.x;
    if (i < n_f) out_f[i] = flat[fidx[i]];
    return;
  }
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= n_steps) return;
  const int32_t* ip = gidx + (t * 64 + lane) * 8;
  unsigned short pc[3][8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = flat[ip[k]];
    const float p0 = __uint_as_float(__float_as_uint(x) & 0xffff0000u);
    const float r1 = x - p0;
    const float p1 = __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
    const float p2 = __uint_as_float(__float_as_uint(r1 - p1) & 0xffff0000u);
    pc[0][k] = (unsigned short)(__float_as_uint(p0) >> 16);
    pc[1][k] = (unsigned short)(__float_as_uint(p1) >> 16);
    pc[2][k] = (unsigned short)(__float_as_uint(p2) >> 16);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    unsigned short* op = out + ((t * 3 + q) * 64 + lane) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) op[k] = pc[q][k];
  }
}

}  // namespace

extern "C" int vqn_pack_x3_gather2(const float* flat, const int32_t* gidx, int64_t n_steps, void* out, const int32_t* fidx, int64_t n_f32,
                                   float* out_f32, void* stream) {
  VQN_CHECK_ARG(flat && gidx && out, "null pointer");
  VQN_CHECK_ARG(n_steps >= 1, "n_steps >= 1");
  VQN_CHECK_ARG(n_f32 >= 0 && (n_f32 == 0 || (fidx && out_f32)), "fidx / out_f32 with n_f32 > 0");
  const long blocks = (n_steps + 3) / 4 + (n_f32 + 255) / 256;
  hipLaunchKernelGGL(pack_x3_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flat, gidx, (long)n_steps,
                     reinterpret_cast<unsigned short*>(out), fidx, (long)n_f32, out_f32);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_pack_x3_gather(const float* flat, const int32_t* gidx, int64_t n_steps, void* out, void* stream) {
  return vqn_pack_x3_gather2(flat, gidx, n_steps, out, nullptr, 0, nullptr, stream);
}

extern "C" int64_t vqn_neus_train_bwd_x3_scratch_bytes(const int32_t* desc) { return train_bwd_scratch_bytes(desc, engine_rules); }

extern "C" int vqn_neus_train_bwd_x3(const int32_t* desc, const void* wbuf_pieces, const float* wbuf_f32, const float* pts, const float* g_rgb,
                                     const float* rgb, const float* g_n, const float* g_sdf, int64_t P, void* scratch, int64_t scratch_bytes,
                                     const float* const* saved, int n_saved, float* const* outs, int n_outs, void* stream) {
  TrainBwdDesc bd;
  TrainBwdPtrs tp;
  long grid;
  const int rc = train_bwd_args(__func__, desc, wbuf_pieces, wbuf_f32, pts, g_rgb, rgb, g_n, g_sdf, P, scratch, scratch_bytes, saved, n_saved,
                                outs, n_outs, engine_rules, "invalid backward descriptor for the x3 engine (layers of at most 256 outputs)",
                                &bd, &tp, &grid);
  if (rc != VQN_OK) return rc;
  return vqn_launch(__func__, bwd_nacc() == 2 ? neus_train_bwd_x3_kernel<2> : neus_train_bwd_x3_kernel<1>, grid, 512,
                    lds_bytes_b(bd.max_tiles), stream, bd, reinterpret_cast<const f32x4*>(wbuf_pieces),
                    reinterpret_cast<const f32x4*>(wbuf_f32), tp, (long)P, reinterpret_cast<f32x4*>(scratch));
}
