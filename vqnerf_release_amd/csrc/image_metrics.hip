// Image metrics on the device: PSNR, MSE, SSIM and their luma forms for a batch of B image pairs [H][W][C], C in {1, 3}
// (decomp/nerfactor/util/metric.py; the float64 statement is tests/image_metrics_model.py).  SSIM is tf.image.ssim with its defaults:
// 11x11 Gaussian window (sigma 1.5, the outer product of the normalised 1-D window the caller passes in), 'VALID' positions,
// c1 = (0.01 * 255)^2, c2 = (0.03 * 255)^2 on 8-bit data.
//
// Two launches per call.
//  * image_metrics_kernel: one workgroup per (32 x 32 tile of window positions, pair).  Its 42 x 42 pixels (tile + 10-pixel halo) are
//    read ONCE, quantised to bytes (the f32 form clips, scales and truncates as the writer's to_uint8 does; the optional alpha plane
//    turns every pixel that is not alpha > thres white first) and kept packed in registers, 7 pixels per thread.  Then per plane
//    (R, G, B, luma): the two planes go to LDS as doubles, the horizontal pass writes the four moment rows conv_h(x), conv_h(y),
//    conv_h(xy), conv_h(x^2 + y^2) to LDS, the vertical pass finishes the four windows of each position and adds luminance * cs to
//    the thread's sum.  Squared differences (exact integers) are taken from the same registers, each pixel by the tile that owns it.
//    The workgroup's sums go to its own 64-byte slot of the scratch buffer: no atomics.
//  * image_metrics_finalize_kernel: one wave per pair adds the slots in a fixed order and writes sums, counts and the five scores.
// Two calls on the same input therefore return the same bits.
//
// Arithmetic: the moments, the SSIM quotient and all sums are float64.  The variance terms conv(x^2 + y^2) - mx^2 - my^2 cancel to
// ~1e-7 relative in f32, against c2 = 58.5 on numbers up to 1.3e5: up to 2e-4 per position in flat bright regions (a white
// background), a systematic part of it from the f32 window not summing to 1 -- more than the 5e-5 a four-decimal score allows.  Byte
// data makes x, y, xy, x^2 + y^2 exact in either format, so float64 accumulation leaves ~1e-13.  gfx950 issues v_fma_f64 at the rate
// of unpacked v_fma_f32; the price is LDS (the doubles), not ALU time.
//
// LDS per workgroup: 2 x 42 x 42 doubles (planes) + 4 x 42 x 32 doubles (moment rows) + reduction = 71.9 KB -> 2 workgroups per CU.
// All LDS accesses of the two passes are lane-consecutive 8-byte words (ds_read_b64 / ds_write_b64: conflict-free within each
// 32-lane half whatever the row stride).
#include "common.h"
#include "wave.h"
#include "vqn_eval.h"

// every product and sum below is rounded on its own (the statement's PSNR is matched bit for bit); fma() is written where wanted
#pragma clang fp contract(off)

namespace {

constexpr int kWin = VQN_IMAGE_METRICS_WINDOW, kHalo = kWin - 1;
constexpr int kTile = 32;                    // window positions per tile edge
constexpr int kIn = kTile + kHalo;           // 42 pixels per tile edge
constexpr int kThreads = 256;
constexpr int kPix = (kIn * kIn + kThreads - 1) / kThreads;      // 7 pixels per thread
constexpr int kSlots = 8;                    // 8-byte words per tile in scratch: ssim[4], luma se, sse[3]
constexpr int kOutWords = VQN_IMAGE_METRICS_OUT_WORDS;   // 8-byte words per pair in `out`

struct ImArgs {
  const void* a;
  const void* b;
  const float* alpha;
  int64_t alpha_stride;
  float thres;
  int H, W, C;
  int tiles_x, tiles_y;
  double w[kWin];
};

__device__ __forceinline__ unsigned quantise(const float f) { return (unsigned)(int)(fminf(fmaxf(f, 0.f), 1.f) * 255.f); }

// the pixel (y, x) of pair b as packed bytes R | G << 8 | B << 16 (C == 1: the value in byte 0)
template <bool F32>
__device__ __forceinline__ unsigned load_pixel(const void* img, const ImArgs& g, const int64_t b, const int y, const int x, const bool keep) {
  const int64_t at = ((b * g.H + y) * (int64_t)g.W + x) * g.C;
  unsigned v = 0;
  for (int c = 0; c < g.C; ++c) {
    unsigned q;
    if (F32) {
      const float f = ((const float*)img)[at + c];
      q = quantise(keep ? f : 1.f);
    } else {
      q = keep ? (unsigned)((const uint8_t*)img)[at + c] : 255u;
    }
    v |= q << (8 * c);
  }
  return v;
}

__device__ __forceinline__ double plane_value(const unsigned v, const int p) {
  if (p < 3) return (double)((v >> (8 * p)) & 255u);
  return 0.2126 * (double)(v & 255u) + 0.7152 * (double)((v >> 8) & 255u) + 0.0722 * (double)((v >> 16) & 255u);
}

template <bool F32>
__global__ __launch_bounds__(kThreads) void image_metrics_kernel(const ImArgs g, double* __restrict__ partials) {
  __shared__ double sx[kIn * kIn], sy[kIn * kIn];
  __shared__ double hb[4][kIn][kTile];
  __shared__ double red[kThreads / 64][kSlots];

  const int tid = threadIdx.x;
  const int64_t b = blockIdx.z;
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const int in_w = min(kIn, g.W - x0), in_h = min(kIn, g.H - y0);          // >= 11 each: the grid has ceil((W - 10) / 32) columns
  const int out_w = in_w - kHalo, out_h = in_h - kHalo;
  const int own_w = (int)blockIdx.x == g.tiles_x - 1 ? in_w : kTile;         // every pixel has one owner: the last tile takes the halo
  const int own_h = (int)blockIdx.y == g.tiles_y - 1 ? in_h : kTile;
  const int P = g.C == 3 ? 4 : 1;

  // ---- the tile's pixels, once: bytes in registers; squared differences of the owned ones ----
  unsigned pa[kPix], pb[kPix];
  unsigned sse[3] = {0u, 0u, 0u};                                            // <= 7 * 255^2 per thread
  double luma_se = 0.0;
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    const int idx = tid + i * kThreads;
    const int iy = idx / kIn, ix = idx - iy * kIn;
    pa[i] = pb[i] = 0u;
    if (iy < in_h && ix < in_w) {
      const int y = y0 + iy, x = x0 + ix;
      bool keep = true;
      if (g.alpha) keep = g.alpha[b * g.alpha_stride + (int64_t)y * g.W + x] > g.thres;
      pa[i] = load_pixel<F32>(g.a, g, b, y, x, keep);
      pb[i] = load_pixel<F32>(g.b, g, b, y, x, keep);
      if (iy < own_h && ix < own_w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int d = (int)((pa[i] >> (8 * c)) & 255u) - (int)((pb[i] >> (8 * c)) & 255u);
          sse[c] += (unsigned)(d * d);
        }
        if (P == 4) {
          const double dl = plane_value(pa[i], 3) - plane_value(pb[i], 3);
          luma_se += dl * dl;
        }
      }
    }
  }

  const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
  double ssim[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < P; ++p) {
    // (the previous plane's vertical pass reads hb only; its horizontal pass, which read sx / sy, ended at a barrier)
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const int idx = tid + i * kThreads;
      if (idx < kIn * kIn) {
        sx[idx] = plane_value(pa[i], p);
        sy[idx] = plane_value(pb[i], p);
      }
    }
    __syncthreads();
    // ---- horizontal pass: four moment rows per input row ----
    for (int idx = tid; idx < in_h * kTile; idx += kThreads) {
      const int r = idx / kTile, c = idx % kTile;
      if (c < out_w) {
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
          const double x = sx[r * kIn + c + k], y = sy[r * kIn + c + k], w = g.w[k];
          m0 = fma(w, x, m0);
          m1 = fma(w, y, m1);
          m2 = fma(w, x * y, m2);
          m3 = fma(w, fma(x, x, y * y), m3);
        }
        hb[0][r][c] = m0;
        hb[1][r][c] = m1;
        hb[2][r][c] = m2;
        hb[3][r][c] = m3;
      }
    }
    __syncthreads();
    // ---- vertical pass + the SSIM quotient ----
    double acc = 0.0;
    for (int idx = tid; idx < out_h * kTile; idx += kThreads) {
      const int r = idx / kTile, c = idx % kTile;
      if (c < out_w) {
        double mx = 0.0, my = 0.0, sxy = 0.0, sxx = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
          const double w = g.w[k];
          mx = fma(w, hb[0][r + k][c], mx);
          my = fma(w, hb[1][r + k][c], my);
          sxy = fma(w, hb[2][r + k][c], sxy);
          sxx = fma(w, hb[3][r + k][c], sxx);
        }
        const double mxy2 = 2.0 * mx * my, msq = mx * mx + my * my;
        acc += ((mxy2 + c1) * (2.0 * sxy - mxy2 + c2)) / ((msq + c1) * (sxx - msq + c2));
      }
    }
    ssim[p] = acc;
  }

  // ---- the workgroup's sums, in a fixed order: butterfly inside each wave, then wave 0..3 ----
  double vals[kSlots];
  for (int p = 0; p < 4; ++p) vals[p] = wave_sum(ssim[p]);
  vals[4] = wave_sum(luma_se);
  unsigned long long isum[3];
  for (int c = 0; c < 3; ++c) isum[c] = wave_sum((unsigned long long)sse[c]);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    for (int s = 0; s < 5; ++s) red[wave][s] = vals[s];
    for (int c = 0; c < 3; ++c) red[wave][5 + c] = __longlong_as_double((long long)isum[c]);
  }
  __syncthreads();
  if (tid < kSlots) {
    const int64_t tile = ((int64_t)b * g.tiles_y + blockIdx.y) * g.tiles_x + blockIdx.x;
    double* dst = partials + tile * kSlots + tid;
    if (tid < 5) {
      double s = red[0][tid];
      for (int w = 1; w < kThreads / 64; ++w) s += red[w][tid];
      *dst = s;
    } else {
      long long s = 0;
      for (int w = 0; w < kThreads / 64; ++w) s += __double_as_longlong(red[w][tid]);
      *dst = __longlong_as_double(s);
    }
  }
}

// log10 in a fixed order of IEEE operations (tests/image_metrics_model.py: log10_det), r > 0 finite
__device__ double log10_det(const double r) {
  int e;
  double m = frexp(r, &e);
  if (m < 0x1.6a09e667f3bcdp-1) {
    m = m * 2.0;
    e -= 1;
  }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double q = 1.0 / 25.0;
  for (int k = 11; k >= 0; --k) q = q * z + 1.0 / (double)(2 * k + 1);
  const double ln_m = (2.0 * s) * q;
  return (double)e * 0x1.34413509f79ffp-2 + ln_m * 0x1.bcb7b1526e50ep-2;
}

__device__ double psnr_of_mse(const double mse) { return mse == 0.0 ? __builtin_inf() : 10.0 * log10_det((255.0 * 255.0) / mse); }

// out[b]: words 0..4 psnr, mse, psnr_luma, ssim, ssim_luma (f64); 5..9 the SSIM sums of R, G, B and luma and the luma squared
// error (f64); 10..14 sse of R, G, B, pixels H W, positions (H - 10)(W - 10) (int64); 15 zero
__global__ __launch_bounds__(64) void image_metrics_finalize_kernel(const double* __restrict__ partials, const int tiles, const int H, const int W,
                                                                    const int C, double* __restrict__ out) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  double fs[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  long long is[3] = {0, 0, 0};
  for (int t = lane; t < tiles; t += 64) {                                   // lane l: tiles l, l + 64, ... in order
    const double* src = partials + (b * tiles + t) * kSlots;
    for (int s = 0; s < 5; ++s) fs[s] += src[s];
    for (int c = 0; c < 3; ++c) is[c] += __double_as_longlong(src[5 + c]);
  }
  for (int s = 0; s < 5; ++s) fs[s] = wave_sum(fs[s]);
  for (int c = 0; c < 3; ++c) is[c] = (long long)wave_sum((unsigned long long)is[c]);
  if (lane != 0) return;
  const long long npix = (long long)H * W, npos = (long long)(H - kHalo) * (W - kHalo);
  if (C == 1) {                                                              // luma of a one-channel image is the channel
    fs[3] = fs[0];
    fs[4] = (double)is[0];
  }
  const double mse = (double)(is[0] + is[1] + is[2]) / (double)(npix * C);
  const double mse_l = fs[4] / (double)npix;
  const double n = (double)npos;
  const double ssim = C == 1 ? fs[0] / n : ((fs[0] / n + fs[1] / n) + fs[2] / n) / 3.0;
  double* o = out + b * kOutWords;
  o[0] = psnr_of_mse(mse);
  o[1] = mse;
  o[2] = psnr_of_mse(mse_l);
  o[3] = ssim;
  o[4] = fs[3] / n;
  for (int s = 0; s < 5; ++s) o[5 + s] = fs[s];
  for (int c = 0; c < 3; ++c) o[10 + c] = __longlong_as_double(is[c]);
  o[13] = __longlong_as_double(npix);
  o[14] = __longlong_as_double(npos);
  o[15] = 0.0;
}

int64_t tiles_of(const int n) { return (n - kHalo + kTile - 1) / kTile; }

template <bool F32>
int image_metrics(const char* fn, const void* a, const void* b, const float* alpha, int64_t alpha_stride, float alpha_thres, int64_t B, int H, int W,
                  int C, const double* window, void* scratch, int64_t scratch_bytes, void* out, void* stream) {
  if (H < kWin || W < kWin) {
    vqn_set_error("%s: unsupported shape: image %dx%d is smaller than the %dx%d SSIM window", fn, H, W, kWin, kWin);
    return VQN_ESHAPE;
  }
  if (C != 1 && C != 3) {
    vqn_set_error("%s: unsupported shape: %d channels (1 or 3)", fn, C);
    return VQN_ESHAPE;
  }
  if (B < 0 || B > 65535 || (int64_t)H * W >= ((int64_t)1 << 31)) {
    vqn_set_error("%s: unsupported shape: 0 <= B <= 65535 pairs of fewer than 2^31 pixels, got B = %lld, %dx%d", fn, (long long)B, H, W);
    return VQN_ESHAPE;
  }
  if (B == 0) return VQN_OK;
  const int64_t need = vqn_image_metrics_scratch_bytes(B, H, W);
  if (!a || !b || !window || !scratch || !out || scratch_bytes < need || (alpha && alpha_stride != 0 && alpha_stride != (int64_t)H * W)) {
    vqn_set_error("%s: bad argument: null pointer, scratch smaller than vqn_image_metrics_scratch_bytes, or alpha_stride not 0 / H W", fn);
    return VQN_EARG;
  }
  ImArgs g;
  g.a = a, g.b = b, g.alpha = alpha, g.alpha_stride = alpha_stride, g.thres = alpha_thres;
  g.H = H, g.W = W, g.C = C;
  g.tiles_x = (int)tiles_of(W), g.tiles_y = (int)tiles_of(H);
  if (g.tiles_y > 65535) {
    vqn_set_error("%s: unsupported shape: more than 65535 tile rows (H = %d)", fn, H);
    return VQN_ESHAPE;
  }
  for (int k = 0; k < kWin; ++k) g.w[k] = window[k];
  hipLaunchKernelGGL(image_metrics_kernel<F32>, dim3(g.tiles_x, g.tiles_y, (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, g, (double*)scratch);
  VQN_LAUNCH_CHECK();
  hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (const double*)scratch,
                     g.tiles_x * g.tiles_y, H, W, C, (double*)out);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

}  // namespace

extern "C" int64_t vqn_image_metrics_scratch_bytes(int64_t B, int H, int W) {
  if (B < 0 || H < kWin || W < kWin) return 0;
  return B * tiles_of(H) * tiles_of(W) * kSlots * (int64_t)sizeof(double);
}

extern "C" int vqn_image_metrics_u8(const uint8_t* a, const uint8_t* b, const float* alpha, int64_t alpha_stride, float alpha_thres, int64_t B, int H,
                                    int W, int C, const double* window, void* scratch, int64_t scratch_bytes, void* out, void* stream) {
  return image_metrics<false>(__func__, a, b, alpha, alpha_stride, alpha_thres, B, H, W, C, window, scratch, scratch_bytes, out, stream);
}

extern "C" int vqn_image_metrics_f32(const float* a, const float* b, const float* alpha, int64_t alpha_stride, float alpha_thres, int64_t B, int H,
                                     int W, int C, const double* window, void* scratch, int64_t scratch_bytes, void* out, void* stream) {
  return image_metrics<true>(__func__, a, b, alpha, alpha_stride, alpha_thres, B, H, W, C, window, scratch, scratch_bytes, out, stream);
}
