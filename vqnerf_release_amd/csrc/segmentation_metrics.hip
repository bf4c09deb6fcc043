// Material segmentation scores on the device: the contingency table of two label images and the scores the reference's
// decomp/nerfvq_nfr3/cluster_eval.py takes from it -- purity, micro / macro F1, macro precision, macro recall
// (decomp/nerfactor/util/segmentation.py; the float64 statement is tests/segmentation_model.py).
//
// Two launches per call.
//  * seg_count_kernel: n pixels (the views of a scene, flattened and concatenated) -> coo[g][p], the number of counted pixels with
//    ground-truth label g and predicted label p, R = n_gt + 1 <= 65 rows, C = n_pd + 1 <= 65 columns.  Two input forms, one body:
//      colour  gt_rgb, pd_rgb uint8 [n][3]; a pixel's label is 1 + the index of the first palette row it equals, 0 when it equals
//              none (class 0 takes part); counted when alpha > alpha_thres (strict; every pixel when alpha is NULL).  The palettes
//              are kernel arguments (packed 24-bit words in scalar registers).
//      label   gt, pd int32 [n] in [0, n_gt] x [0, n_pd]; counted when mask != 0 (every pixel when mask is NULL); a counted pixel
//              with a label outside the range does not enter the table but the `invalid` counter.
//    A workgroup of 256 threads takes passes of kPass = 4096 pixels, 16 CONSECUTIVE pixels per lane (16-byte loads when the three
//    base pointers are 16-byte aligned: 3 per colour image, 4 per label image, 4 of alpha, 1 of mask; the ragged last lane and
//    unaligned inputs read pixel by pixel), passes blockIdx.x, blockIdx.x + gridDim.x, ...; the grid is min(kGridCap, passes),
//    kGridCap = 512 = 2 workgroups per CU of the 256-CU chip.  Each workgroup keeps a private table of R * C + 1 32-bit counters in
//    LDS (<= 16.9 KB; the last one is `invalid`).  Label images are flat: all 64 lanes of a wave usually hold the same (g, p), and
//    one ds_add per pixel would serialise on one counter.  So counts are combined BEFORE they touch LDS:
//      1. a lane run-length merges its 16 pixels in registers: it presents (key, run length) only where a run ends;
//      2. per pixel slot the wave merges equal keys and ONE lane adds their sum to LDS (wave_add<kMinMerge>, csrc/wave.h).
//    A flat wave costs one LDS add per 1024 pixels.  Nothing is accumulated across workgroups with atomics: each workgroup writes
//    its table as plain words to its own slot of the scratch buffer.
//  * seg_finalize_kernel: one workgroup.  Sums the slots in slot order into int64 cells, then (float64, fixed order of operations):
//      present rows / columns: those with a non-zero sum (the reference's `resort`);
//      label_map[p] = the row with the largest count in column p, ties to the lowest row (np.argmax), -1 for an absent column;
//      purity = sum_p max_g coo[g][p] / total;   merged confusion M[g][g'] = sum of coo[g][p] over p with label_map[p] = g';
//      per present row g: tp = M[g][g], pred = sum_r M[r][g], true = sum_c M[g][c]; precision = tp / pred (0 when pred = 0),
//      recall = tp / true, f1 = 2 tp / (2 tp + (pred - tp) + (true - tp));
//      p_macro, r_macro, f1_macro = the sums over present rows in ascending order / their number;  f1_micro = sum tp / total.
//    total = 0: the five scores are NaN.
// Integer LDS adds commute, the slots are summed in order: two calls on the same input return the same bits.
//
// out: (kHeadWords + R * C) 8-byte words
//   0..4   float64  purity, f1_micro, f1_macro, p_macro, r_macro
//   5..8   int64    total (counted pixels in the table), invalid, number of present rows, number of present columns
//   9..41  int32    label_map[65] (entries >= C are -1) and one zero word of padding
//   42..   int64    coo[R][C]
#include "common.h"
#include "wave.h"
#include "vqn_eval.h"

// every quotient and sum below is rounded on its own, as the statement's are
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPass = VQN_SEG_PIXELS_PER_PASS;   // 4096 pixels per workgroup pass
constexpr int kPix = kPass / kThreads;       // consecutive pixels per lane and pass: 16
constexpr int kGridCap = VQN_SEG_GRID_CAP;   // workgroups at most: 2 per CU of a 256-CU MI355X
constexpr int kMaxSide = VQN_SEG_MAX_SIDE;   // R, C <= 65: the K = 64 codebook plus class 0
static_assert(kPix * kThreads == kPass, "a pass is whole lanes");
constexpr int kMinMerge = 8;                 // keep merging across the wave while a round absorbed this many lanes
constexpr int kFinThreads = 1024;
constexpr int kHeadWords = VQN_SEG_HEAD_WORDS;   // 8-byte words of `out` ahead of the table
constexpr int kSkip = -1;                    // key of a pixel that is not counted

struct SegArgs {
  const void* gt;
  const void* pd;
  const void* sel;                           // colour form: float alpha [n]; label form: uint8 mask [n]; may be NULL
  float thres;
  int64_t n;
  int R, C;
  uint32_t pal_gt[kMaxSide - 1], pal_pd[kMaxSide - 1];      // R | G << 8 | B << 16, rows 0 .. R - 2 / C - 2 (colour form)
};

// pixel j of 48 bytes held as 12 words: its three bytes as R | G << 8 | B << 16
__device__ __forceinline__ uint32_t pixel_of(const uint32_t (&w)[12], const int j) {
  const int o = 3 * j, d = o >> 2, s = (o & 3) * 8;
  uint32_t v = w[d] >> s;
  if (s > 8) v |= w[d + 1] << (32 - s);
  return v & 0xffffffu;
}

__device__ __forceinline__ int palette_label(const uint32_t v, const uint32_t* pal, const int rows) {
  int label = 0;
  for (int i = rows - 1; i >= 0; --i)        // descending: the first row that matches is the one left standing
    if (v == pal[i]) label = i + 1;
  return label;
}

template <bool RGB, bool VEC>
__global__ __launch_bounds__(kThreads) void seg_count_kernel(const SegArgs a, unsigned* __restrict__ slots) {
  __shared__ unsigned table[kMaxSide * kMaxSide + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int words = a.R * a.C + 1, invalid_key = a.R * a.C;
  for (int i = tid; i < words; i += kThreads) table[i] = 0u;
  __syncthreads();

  const int64_t passes = (a.n + kPass - 1) / kPass;
  for (int64_t pass = blockIdx.x; pass < passes; pass += gridDim.x) {       // the same trip count for every lane of the workgroup
    const int64_t i0 = pass * kPass + (int64_t)tid * kPix;
    int key[kPix];
    if (VEC && i0 + kPix <= a.n) {
      // ---- 16 whole pixels: 16-byte loads ----
      bool keep[kPix];
      if (RGB) {
        if (a.sel) {
          const f32x4* ap = (const f32x4*)((const float*)a.sel + i0);
#pragma unroll
          for (int q = 0; q < kPix / 4; ++q) {
            const f32x4 v = ap[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) keep[4 * q + j] = v[j] > a.thres;
          }
        } else {
#pragma unroll
          for (int j = 0; j < kPix; ++j) keep[j] = true;
        }
        uint32_t wg[12], wp[12];
        const uint4* gp = (const uint4*)((const uint8_t*)a.gt + i0 * 3);
        const uint4* pp = (const uint4*)((const uint8_t*)a.pd + i0 * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const uint4 x = gp[q], y = pp[q];
          wg[4 * q] = x.x, wg[4 * q + 1] = x.y, wg[4 * q + 2] = x.z, wg[4 * q + 3] = x.w;
          wp[4 * q] = y.x, wp[4 * q + 1] = y.y, wp[4 * q + 2] = y.z, wp[4 * q + 3] = y.w;
        }
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
          const int g = palette_label(pixel_of(wg, j), a.pal_gt, a.R - 1), p = palette_label(pixel_of(wp, j), a.pal_pd, a.C - 1);
          key[j] = keep[j] ? g * a.C + p : kSkip;
        }
      } else {
        if (a.sel) {
          const uint4 mv = *(const uint4*)((const uint8_t*)a.sel + i0);
          const uint32_t mw[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
          for (int j = 0; j < kPix; ++j) keep[j] = ((mw[j >> 2] >> (8 * (j & 3))) & 255u) != 0u;
        } else {
#pragma unroll
          for (int j = 0; j < kPix; ++j) keep[j] = true;
        }
        const uint4* gp = (const uint4*)((const int32_t*)a.gt + i0);
        const uint4* pp = (const uint4*)((const int32_t*)a.pd + i0);
#pragma unroll
        for (int q = 0; q < kPix / 4; ++q) {
          const uint4 x = gp[q], y = pp[q];
          const uint32_t gs[4] = {x.x, x.y, x.z, x.w}, ps[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool ok = gs[j] < (uint32_t)a.R && ps[j] < (uint32_t)a.C;          // negative labels wrap to large values
            key[4 * q + j] = !keep[4 * q + j] ? kSkip : ok ? (int)(gs[j] * (uint32_t)a.C + ps[j]) : invalid_key;
          }
        }
      }
    } else {
      // ---- the ragged end of the image, or unaligned inputs: pixel by pixel ----
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        const int64_t i = i0 + j;
        key[j] = kSkip;
        if (i < a.n) {
          if (RGB) {
            const bool keep = a.sel ? ((const float*)a.sel)[i] > a.thres : true;
            const uint8_t* gb = (const uint8_t*)a.gt + i * 3;
            const uint8_t* pb = (const uint8_t*)a.pd + i * 3;
            const uint32_t cg = (uint32_t)gb[0] | (uint32_t)gb[1] << 8 | (uint32_t)gb[2] << 16;
            const uint32_t cp = (uint32_t)pb[0] | (uint32_t)pb[1] << 8 | (uint32_t)pb[2] << 16;
            const int g = palette_label(cg, a.pal_gt, a.R - 1), p = palette_label(cp, a.pal_pd, a.C - 1);
            if (keep) key[j] = g * a.C + p;
          } else {
            const bool keep = a.sel ? ((const uint8_t*)a.sel)[i] != 0 : true;
            const uint32_t g = (uint32_t)((const int32_t*)a.gt)[i], p = (uint32_t)((const int32_t*)a.pd)[i];
            if (keep) key[j] = g < (uint32_t)a.R && p < (uint32_t)a.C ? (int)(g * (uint32_t)a.C + p) : invalid_key;
          }
        }
      }
    }
    // ---- run-length merge in the lane, equal keys across the wave, then LDS ----
    unsigned run = 0u;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      run += 1u;
      const bool ends = j == kPix - 1 || key[j + 1] != key[j];
      wave_add<kMinMerge>(table, ends && key[j] != kSkip, key[j], run, lane);
      if (ends) run = 0u;
    }
  }
  __syncthreads();
  unsigned* dst = slots + (int64_t)blockIdx.x * words;
  for (int i = tid; i < words; i += kThreads) dst[i] = table[i];
}

__global__ __launch_bounds__(kFinThreads) void seg_finalize_kernel(const unsigned* __restrict__ slots, const int blocks, const int R, const int C,
                                                                   long long* __restrict__ out) {
  __shared__ long long tab[kMaxSide * kMaxSide];
  __shared__ long long rowsum[kMaxSide], colsum[kMaxSide], colmax[kMaxSide], tp[kMaxSide], pred[kMaxSide];
  __shared__ int lmap[kMaxSide];
  __shared__ long long invalid;
  const int tid = threadIdx.x;
  const int cells = R * C, words = cells + 1;
  for (int i = tid; i < words; i += kFinThreads) {
    long long s = 0;
    for (int b = 0; b < blocks; ++b) s += (long long)slots[(int64_t)b * words + i];          // slot order
    if (i < cells) {
      tab[i] = s;
      out[kHeadWords + i] = s;
    } else {
      invalid = s;
    }
  }
  __syncthreads();
  if (tid < R) {
    long long s = 0;
    for (int p = 0; p < C; ++p) s += tab[tid * C + p];
    rowsum[tid] = s;
  } else if (tid >= 128 && tid < 128 + kMaxSide) {
    const int p = tid - 128;
    long long s = 0, best = 0;
    int arg = -1;
    if (p < C) {
      for (int g = 0; g < R; ++g) {
        const long long v = tab[g * C + p];
        s += v;
        if (v > best) best = v, arg = g;                                     // strict: a tie stays with the lowest row
      }
    }
    colsum[p] = s, colmax[p] = best, lmap[p] = arg;
  }
  __syncthreads();
  if (tid < R) {
    long long t = 0, q = 0;
    for (int p = 0; p < C; ++p) {
      if (lmap[p] == tid) {
        t += tab[tid * C + p];
        q += colsum[p];
      }
    }
    tp[tid] = t, pred[tid] = q;
  } else if (tid >= 128 && tid < 128 + 33) {                                 // label_map: 65 int32 and a zero, as 33 words
    const int w = tid - 128;
    const unsigned lo = (unsigned)lmap[2 * w], hi = 2 * w + 1 < kMaxSide ? (unsigned)lmap[2 * w + 1] : 0u;
    out[9 + w] = (long long)((unsigned long long)lo | (unsigned long long)hi << 32);
  }
  __syncthreads();
  if (tid != 0) return;
  long long total = 0, max_sum = 0, tp_sum = 0;
  int rows = 0, cols = 0;
  for (int g = 0; g < R; ++g) total += rowsum[g], rows += rowsum[g] > 0;
  for (int p = 0; p < C; ++p) max_sum += colmax[p], cols += colsum[p] > 0;
  double ps = 0.0, rs = 0.0, fs = 0.0;
  for (int g = 0; g < R; ++g) {                                              // present rows, ascending
    if (rowsum[g] == 0) continue;
    const long long t = tp[g], fp = pred[g] - t, fn = rowsum[g] - t;
    tp_sum += t;
    ps += pred[g] == 0 ? 0.0 : (double)t / (double)pred[g];
    rs += (double)t / (double)rowsum[g];
    fs += (double)(2 * t) / (double)(2 * t + fp + fn);
  }
  double* o = (double*)out;
  if (total == 0) {
    for (int s = 0; s < 5; ++s) o[s] = __builtin_nan("");
  } else {
    o[0] = (double)max_sum / (double)total;
    o[1] = (double)tp_sum / (double)total;
    o[2] = fs / (double)rows;
    o[3] = ps / (double)rows;
    o[4] = rs / (double)rows;
  }
  out[5] = total;
  out[6] = invalid;
  out[7] = rows;
  out[8] = cols;
}

int64_t blocks_of(const int64_t n) {
  const int64_t passes = (n + kPass - 1) / kPass;
  return passes < 1 ? 1 : passes < kGridCap ? passes : kGridCap;             // n = 0 still runs one workgroup: an empty table
}

bool shape_ok(const int64_t n, const int R, const int C) {
  return n >= 0 && n < ((int64_t)1 << 31) && R >= 1 && R <= kMaxSide && C >= 1 && C <= kMaxSide;
}

template <bool RGB>
int seg_contingency(const char* fn, SegArgs& a, const int n_gt, const int n_pd, void* scratch, const int64_t scratch_bytes, void* out, void* stream) {
  a.R = n_gt + 1, a.C = n_pd + 1;
  if (n_gt < 0 || n_pd < 0 || a.R > kMaxSide || a.C > kMaxSide) {
    vqn_set_error("%s: unsupported shape: table sides R = n_gt + 1 and C = n_pd + 1 must lie in 1 .. %d, got R = %d, C = %d", fn, kMaxSide, a.R, a.C);
    return VQN_ESHAPE;
  }
  if (a.n < 0 || a.n >= ((int64_t)1 << 31)) {
    vqn_set_error("%s: unsupported shape: 0 <= n < 2^31 pixels, got n = %lld", fn, (long long)a.n);
    return VQN_ESHAPE;
  }
  const int64_t need = vqn_seg_scratch_bytes(a.n, a.R, a.C);
  if ((a.n > 0 && (!a.gt || !a.pd)) || !scratch || !out || scratch_bytes < need) {
    vqn_set_error("%s: bad argument: null pointer, or scratch smaller than vqn_seg_scratch_bytes (%lld bytes)", fn, (long long)need);
    return VQN_EARG;
  }
  const unsigned blocks = (unsigned)blocks_of(a.n);
  const bool vec = (((uintptr_t)a.gt | (uintptr_t)a.pd | (uintptr_t)a.sel) & 15u) == 0u;
  if (vec)
    hipLaunchKernelGGL((seg_count_kernel<RGB, true>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a, (unsigned*)scratch);
  else
    hipLaunchKernelGGL((seg_count_kernel<RGB, false>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a, (unsigned*)scratch);
  VQN_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_finalize_kernel, dim3(1), dim3(kFinThreads), 0, (hipStream_t)stream, (const unsigned*)scratch, (int)blocks, a.R, a.C,
                     (long long*)out);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

}  // namespace

extern "C" int64_t vqn_seg_scratch_bytes(int64_t n, int R, int C) {
  if (!shape_ok(n, R, C)) return 0;
  return blocks_of(n) * ((int64_t)R * C + 1) * (int64_t)sizeof(unsigned);
}

extern "C" int vqn_seg_contingency_rgb(const uint8_t* gt_rgb, const uint8_t* pd_rgb, const float* alpha, float alpha_thres, int64_t n,
                                       const uint8_t* gt_palette, int n_gt, const uint8_t* pd_palette, int n_pd, void* scratch, int64_t scratch_bytes,
                                       void* out, void* stream) {
  SegArgs a;
  memset(&a, 0, sizeof(a));
  a.gt = gt_rgb, a.pd = pd_rgb, a.sel = alpha, a.thres = alpha_thres, a.n = n;
  if ((n_gt > 0 && !gt_palette) || (n_pd > 0 && !pd_palette)) {
    vqn_set_error("%s: bad argument: null palette", __func__);
    return VQN_EARG;
  }
  for (int i = 0; i < n_gt && i < kMaxSide - 1; ++i)
    a.pal_gt[i] = (uint32_t)gt_palette[3 * i] | (uint32_t)gt_palette[3 * i + 1] << 8 | (uint32_t)gt_palette[3 * i + 2] << 16;
  for (int i = 0; i < n_pd && i < kMaxSide - 1; ++i)
    a.pal_pd[i] = (uint32_t)pd_palette[3 * i] | (uint32_t)pd_palette[3 * i + 1] << 8 | (uint32_t)pd_palette[3 * i + 2] << 16;
  return seg_contingency<true>(__func__, a, n_gt, n_pd, scratch, scratch_bytes, out, stream);
}

extern "C" int vqn_seg_contingency_labels(const int32_t* gt, const int32_t* pd, const uint8_t* mask, int64_t n, int n_gt, int n_pd, void* scratch,
                                          int64_t scratch_bytes, void* out, void* stream) {
  SegArgs a;
  memset(&a, 0, sizeof(a));
  a.gt = gt, a.pd = pd, a.sel = mask, a.thres = 0.f, a.n = n;
  return seg_contingency<false>(__func__, a, n_gt, n_pd, scratch, scratch_bytes, out, stream);
}
