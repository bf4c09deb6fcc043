// Baseline JPEG on the device: uint8 [N, H, W, 3] RGB frames -> one contiguous byte stream per frame, the bytes between SOS and EOI of a
// file whose header csrc/jpeg_plan.h writes (decomp/nerfactor/util/mjpeg.py puts the two together; the float64 statement is
// tests/jpeg_model.py).  Five launches and no host read:
//
//   1. jpeg_dct_kernel: pixels -> quantised coefficients.  A workgroup of 256 threads takes a tile of 16 rows x 64 columns of the
//      padded frame (rows and columns past the frame repeat its last ones): every thread reads 4 pixels of a column, so that the 64
//      lanes of a wave read 192 consecutive bytes of a row, converts them with the JFIF full-range BT.601 matrix in f32 and puts Y,
//      Cb, Cr into LDS planes whose rows are 65 floats apart (the column pass below then reads 32 different banks).  '420' averages the
//      chroma of each 2 x 2 square into planes of 8 x 32 (rows 33 apart).  The 8 x 8 blocks of the planes (48 for '444', 24 for '420')
//      are transformed in place, rows first (one thread per row of a block), then columns (one thread per column of a block, lanes on
//      consecutive columns), as plain 8 x 8 products with the orthonormal DCT-II matrix; the column pass divides by the table entry,
//      rounds half away from zero and puts the int16 at its zigzag position of an LDS image of the blocks, which goes to memory as
//      whole 32-bit words, a run of consecutive blocks of a block row at a time.
//      Coefficients: three planes, Y [N][by_y][bx_y][64], Cb and Cr [N][by_c][bx_c][64], int16 in zigzag order (by, bx: JpegGeom).
//   2. jpeg_entropy_kernel: one wave per (frame, restart interval), lane k on zigzag coefficient k of the block at hand.  The non-zero
//      lanes of a block are a ballot; from it a lane knows the run of zeros in front of it, so it forms all of its bits alone (up to
//      three ZRL codes, its run / size code and its magnitude bits, 59 bits at most; lane 0 the DC difference, the lane behind the last
//      non-zero coefficient the EOB), a wave prefix sum of the lengths places them, and LDS atomic ORs on disjoint bits assemble the
//      block.  Whole bytes are then flushed into the interval's slot with FF -> FF 00 stuffing (a ballot of the FF bytes gives every
//      byte its place) and the 0 .. 7 bits left over start the next block.  An interval begins with predictors 0 and ends padded
//      with 1-bits; it depends on nothing outside itself.  The slot is sized by the worst case (kJpegBlockBytes per block), every
//      store is guarded by the slot size all the same, and values are clamped to what baseline JPEG can code, so that no coefficient
//      buffer whatever makes a wave write outside its slot.
//   3. jpeg_scan_kernel: one workgroup turns the interval lengths into the place of every interval in the output (frames back to
//      back, two bytes of RSTm between the intervals of a frame) and writes the [N][2] offsets and ends of the frames, which
//      jpeg_meta_kernel turns into offsets and lengths.
//   4. jpeg_compact_kernel: one workgroup per (interval, frame) copies the slot to its place and appends its RST marker.
// Everything is integer work or f32 arithmetic in a fixed order: equal frames give equal bytes.
#include "codec_stream.h"
#include "common.h"
#include "jpeg_plan.h"
#include "wave.h"
#include "vqn_image_codec.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTileH = 16, kTileW = 64;
constexpr int kLd = kTileW + 1;              // floats between the rows of a full-resolution LDS plane
constexpr int kLdHalf = kTileW / 2 + 1;      // ... of a subsampled chroma plane

// orthonormal DCT-II matrix [u][x] = c(u) cos((2 x + 1) u pi / 16), c(0) = sqrt(1/8), else 1/2
__constant__ float c_dct[64] = {
    0.35355339059327379f, 0.35355339059327379f,  0.35355339059327379f,  0.35355339059327379f,  0.35355339059327379f,  0.35355339059327379f,
    0.35355339059327379f, 0.35355339059327379f,  0.49039264020161522f,  0.41573480615127262f,  0.27778511650980114f,  0.09754516100806417f,
    -0.09754516100806417f, -0.27778511650980114f, -0.41573480615127262f, -0.49039264020161522f, 0.46193976625564337f,  0.19134171618254492f,
    -0.19134171618254492f, -0.46193976625564337f, -0.46193976625564337f, -0.19134171618254492f, 0.19134171618254492f,  0.46193976625564337f,
    0.41573480615127262f, -0.09754516100806417f, -0.49039264020161522f, -0.27778511650980114f, 0.27778511650980114f,  0.49039264020161522f,
    0.09754516100806417f, -0.41573480615127262f, 0.35355339059327379f,  -0.35355339059327379f, -0.35355339059327379f, 0.35355339059327379f,
    0.35355339059327379f, -0.35355339059327379f, -0.35355339059327379f, 0.35355339059327379f,  0.27778511650980114f,  -0.49039264020161522f,
    0.09754516100806417f, 0.41573480615127262f,  -0.41573480615127262f, -0.09754516100806417f, 0.49039264020161522f,  -0.27778511650980114f,
    0.19134171618254492f, -0.46193976625564337f, 0.46193976625564337f,  -0.19134171618254492f, -0.19134171618254492f, 0.46193976625564337f,
    -0.46193976625564337f, 0.19134171618254492f, 0.09754516100806417f,  -0.27778511650980114f, 0.41573480615127262f,  -0.49039264020161522f,
    0.49039264020161522f, -0.41573480615127262f, 0.27778511650980114f,  -0.09754516100806417f};
// natural index (row * 8 + column) -> zigzag position
__constant__ uint8_t c_zigzag_of[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                        41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                        46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct DctArgs {
  const uint8_t* rgb;
  int16_t* coef[3];                          // Y, Cb, Cr
  int h, w;
  int by_y, bx_y, by_c, bx_c;
  uint16_t q[2][64];                         // luma, chroma; natural order
};

// the 8-point transform of v[0 .. 7] (contraction is off: products and sums are rounded one by one, left to right)
__device__ __forceinline__ void dct8(const float (&v)[8], float (&o)[8]) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    float s = c_dct[u * 8] * v[0];
#pragma unroll
    for (int x = 1; x < 8; ++x) s += c_dct[u * 8 + x] * v[x];
    o[u] = s;
  }
}

// rows of the blocks of a plane of R rows x C columns (LD floats between rows), in place: one task per (row, block column)
template <int R, int C, int LD>
__device__ __forceinline__ void row_pass(float* p, const int tid) {
  constexpr int kTasks = R * (C / 8);
  for (int t = tid; t < kTasks; t += kThreads) {
    float* row = p + (t / (C / 8)) * LD + (t % (C / 8)) * 8;
    float v[8], o[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) v[x] = row[x];
    dct8(v, o);
#pragma unroll
    for (int x = 0; x < 8; ++x) row[x] = o[x];
  }
}

// columns of the blocks, quantised into the LDS image of the blocks: qout[(block row * (C / 8) + block column) * 64 + zigzag position]
template <int R, int C, int LD>
__device__ __forceinline__ void col_pass(const float* p, const float* q, int16_t* qout, const int tid) {
  constexpr int kTasks = (R / 8) * C;
  for (int t = tid; t < kTasks; t += kThreads) {
    const int br = t / C, c = t % C, v8 = c & 7;
    const float* col = p + br * 8 * LD + c;
    float v[8], o[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) v[y] = col[y * LD];
    dct8(v, o);
    int16_t* dst = qout + (br * (C / 8) + c / 8) * 64;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float r = o[u] / q[u * 8 + v8];
      const int k = (int)(r + (r < 0.f ? -0.5f : 0.5f));                 // half away from zero (the cast truncates)
      dst[c_zigzag_of[u * 8 + v8]] = (int16_t)(k < -1024 ? -1024 : k > 1023 ? 1023 : k);
    }
  }
}

// the blocks of the LDS image (R8 x C8 of them) -> plane [by][bx][64] at block (by0, bx0), whole 32-bit words, blocks past the plane dropped
template <int R8, int C8>
__device__ __forceinline__ void store_blocks(const int16_t* qout, int16_t* plane, const int by0, const int bx0, const int by, const int bx,
                                             const int tid) {
  const uint32_t* src = (const uint32_t*)qout;
  for (int i = tid; i < R8 * C8 * 32; i += kThreads) {
    const int b = i >> 5, r = b / C8, c = b % C8;
    if (by0 + r < by && bx0 + c < bx) ((uint32_t*)plane)[((int64_t)(by0 + r) * bx + (bx0 + c)) * 32 + (i & 31)] = src[i];
  }
}

template <bool SUB420>
__global__ __launch_bounds__(kThreads) void jpeg_dct_kernel(const DctArgs a) {
  __shared__ float plane[3][kTileH * kLd];
  __shared__ float half[2][(kTileH / 2) * kLdHalf];
  __shared__ float q[2][64];
  __shared__ __attribute__((aligned(4))) int16_t qout[3 * (kTileH / 8) * (kTileW / 8) * 64];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const int64_t frame = blockIdx.z;
  if (tid < 128) q[tid >> 6][tid & 63] = (float)a.q[tid >> 6][tid & 63];
  const uint8_t* img = a.rgb + frame * a.h * a.w * 3;
  {
    const int cx = tid & 63, x = min(x0 + cx, a.w - 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cy = (tid >> 6) + 4 * k, y = min(y0 + cy, a.h - 1);
      const uint8_t* px = img + ((int64_t)y * a.w + x) * 3;
      const float R = (float)px[0], G = (float)px[1], B = (float)px[2];
      plane[0][cy * kLd + cx] = (0.299f * R + 0.587f * G + 0.114f * B) - 128.f;
      plane[1][cy * kLd + cx] = -0.168735892f * R - 0.331264108f * G + 0.5f * B;            // (+ 128 - 128: the level shift)
      plane[2][cy * kLd + cx] = 0.5f * R - 0.418687589f * G - 0.081312411f * B;
    }
  }
  __syncthreads();
  if (SUB420) {
    const int cx = tid & 31, cy = tid >> 5;                                                 // 8 x 32 chroma samples
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float* p = plane[1 + c] + 2 * cy * kLd + 2 * cx;
      half[c][cy * kLdHalf + cx] = ((p[0] + p[1]) + (p[kLd] + p[kLd + 1])) * 0.25f;
    }
    __syncthreads();
  }
  row_pass<kTileH, kTileW, kLd>(plane[0], tid);
  if (SUB420) {
    row_pass<kTileH / 2, kTileW / 2, kLdHalf>(half[0], tid);
    row_pass<kTileH / 2, kTileW / 2, kLdHalf>(half[1], tid);
  } else {
    row_pass<kTileH, kTileW, kLd>(plane[1], tid);
    row_pass<kTileH, kTileW, kLd>(plane[2], tid);
  }
  __syncthreads();
  constexpr int kYBlocks = (kTileH / 8) * (kTileW / 8);
  constexpr int kCBlocks = SUB420 ? kYBlocks / 4 : kYBlocks;
  col_pass<kTileH, kTileW, kLd>(plane[0], q[0], qout, tid);
  if (SUB420) {
    col_pass<kTileH / 2, kTileW / 2, kLdHalf>(half[0], q[1], qout + kYBlocks * 64, tid);
    col_pass<kTileH / 2, kTileW / 2, kLdHalf>(half[1], q[1], qout + (kYBlocks + kCBlocks) * 64, tid);
  } else {
    col_pass<kTileH, kTileW, kLd>(plane[1], q[1], qout + kYBlocks * 64, tid);
    col_pass<kTileH, kTileW, kLd>(plane[2], q[1], qout + (kYBlocks + kCBlocks) * 64, tid);
  }
  __syncthreads();
  int16_t* y = a.coef[0] + frame * a.by_y * a.bx_y * 64;
  int16_t* cb = a.coef[1] + frame * a.by_c * a.bx_c * 64;
  int16_t* cr = a.coef[2] + frame * a.by_c * a.bx_c * 64;
  store_blocks<kTileH / 8, kTileW / 8>(qout, y, y0 / 8, x0 / 8, a.by_y, a.bx_y, tid);
  if (SUB420) {
    store_blocks<kTileH / 16, kTileW / 16>(qout + kYBlocks * 64, cb, y0 / 16, x0 / 16, a.by_c, a.bx_c, tid);
    store_blocks<kTileH / 16, kTileW / 16>(qout + (kYBlocks + kCBlocks) * 64, cr, y0 / 16, x0 / 16, a.by_c, a.bx_c, tid);
  } else {
    store_blocks<kTileH / 8, kTileW / 8>(qout + kYBlocks * 64, cb, y0 / 8, x0 / 8, a.by_c, a.bx_c, tid);
    store_blocks<kTileH / 8, kTileW / 8>(qout + (kYBlocks + kCBlocks) * 64, cr, y0 / 8, x0 / 8, a.by_c, a.bx_c, tid);
  }
}

// ---- 2. entropy coding ----------------------------------------------------------------------------------------------------------------
struct EntropyArgs {
  const int16_t* coef[3];
  uint8_t* slots;                            // [N][intervals][slot_bytes]
  uint32_t* lens;                            // [N][intervals]
  int by_y, bx_y, by_c, bx_c;
  int mcus_x, mcus, ri, intervals, sub420;
  int64_t slot_bytes;
  JpegHuff huff;
};

constexpr int kBitWords = 64;                // LDS words of a wave's bit buffer: 7 bits left over + kJpegBlockBits, and two words of slack
static_assert((7 + kJpegBlockBits + 31) / 32 + 2 <= kBitWords, "a block fits the bit buffer");
constexpr int kHuffWords = sizeof(JpegHuff) / 4;

// byte i of the bit buffer (bits run from the top of word 0)
__device__ __forceinline__ uint32_t bit_byte(const uint32_t* words, const int i) { return (words[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const EntropyArgs a) {
  __shared__ uint32_t huff[kHuffWords];
  __shared__ uint32_t words[kBitWords];
  const int lane = threadIdx.x;
  const int interval = blockIdx.x;
  const int64_t frame = blockIdx.y;
  for (int i = lane; i < kHuffWords; i += 64) huff[i] = ((const uint32_t*)&a.huff)[i];
  words[lane] = 0u;
  __syncthreads();
  uint8_t* slot = a.slots + (frame * a.intervals + interval) * a.slot_bytes;
  const int64_t cap = a.slot_bytes;
  const int16_t* plane_y = a.coef[0] + frame * a.by_y * a.bx_y * 64;
  const int16_t* plane_cb = a.coef[1] + frame * a.by_c * a.bx_c * 64;
  const int16_t* plane_cr = a.coef[2] + frame * a.by_c * a.bx_c * 64;
  const int per_mcu = a.sub420 ? 6 : 3;
  const int m0 = interval * a.ri, m1 = min(m0 + a.ri, a.mcus);
  int pred_y = 0, pred_cb = 0, pred_cr = 0;      // (three names, not an array: the component is a runtime value)
  int bitpos = 0;                            // bits waiting in `words`
  int64_t outpos = 0;                        // bytes of the slot written
  for (int m = m0; m < m1; ++m) {            // (everything that steers the loops is the same in every lane)
    const int my = m / a.mcus_x, mx = m % a.mcus_x;
    for (int b = 0; b < per_mcu; ++b) {
      const int comp = b < per_mcu - 2 ? 0 : b - (per_mcu - 2) + 1, cls = comp ? 1 : 0;
      int64_t block;
      if (comp)
        block = (int64_t)my * a.bx_c + mx;
      else if (a.sub420)
        block = (int64_t)(2 * my + (b >> 1)) * a.bx_y + 2 * mx + (b & 1);
      else
        block = (int64_t)my * a.bx_y + mx;
      const uint32_t* dc_tab = huff + 12 * cls;
      const uint32_t* ac_tab = huff + 24 + 256 * cls;
      int v = (comp == 0 ? plane_y : comp == 1 ? plane_cb : plane_cr)[block * 64 + lane];
      const int dc = __shfl(v, 0, 64);
      const int pred = comp == 0 ? pred_y : comp == 1 ? pred_cb : pred_cr;
      if (lane == 0) v = max(-2047, min(2047, dc - pred));
      else v = max(-1023, min(1023, v));
      if (comp == 0) pred_y = dc;
      else if (comp == 1) pred_cb = dc;
      else pred_cr = dc;
      // ---- the bits of this lane ----
      const unsigned long long nz = __ballot(v != 0) & ~1ull;            // the non-zero AC lanes
      const int last = 63 - __clzll((long long)(nz | 1ull));             // the last of them, 0: none
      const int mag = v < 0 ? -v : v;
      const int cat = 32 - __clz(mag);                                   // (__clz(0) = 32)
      const uint32_t magbits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
      unsigned long long acc = 0ull;
      int n = 0;
      if (lane == 0) {
        const uint32_t e = dc_tab[cat];
        acc = (unsigned long long)(e & 0xffffu) << cat | magbits;
        n = (int)(e >> 16) + cat;
      } else if (v != 0) {
        const unsigned long long below = nz & ((1ull << lane) - 1ull);
        const int prev = 63 - __clzll((long long)(below | 1ull));
        const int run = lane - prev - 1;
        const uint32_t zrl = ac_tab[0xf0], e = ac_tab[(run & 15) << 4 | cat];
        for (int i = 0; i < (run >> 4); ++i) acc = acc << (zrl >> 16) | (zrl & 0xffffu), n += (int)(zrl >> 16);
        acc = (acc << (e >> 16) | (e & 0xffffu)) << cat | magbits;
        n += (int)(e >> 16) + cat;
      } else if (lane == last + 1) {                                     // zeros up to the end of the block: EOB
        const uint32_t e = ac_tab[0];
        acc = e & 0xffffu, n = (int)(e >> 16);
      }
      int total;
      const int p = bitpos + wave_exclusive_sum(n, lane, &total);
      if (n > 0) {
        const int w = p >> 5, s = p & 31;
        const unsigned long long x = acc << (64 - n);                    // the bits at the top of 64
        const unsigned long long hi = x >> s;
        const uint32_t lo = s ? (uint32_t)((x << (64 - s)) >> 32) : 0u;
        if (hi >> 32) atomicOr(&words[w], (uint32_t)(hi >> 32));
        if ((uint32_t)hi) atomicOr(&words[w + 1], (uint32_t)hi);
        if (lo) atomicOr(&words[w + 2], lo);
      }
      bitpos += total;
      __syncthreads();
      // ---- whole bytes -> the slot, stuffed ----
      const int n_bytes = bitpos >> 3;
      for (int base = 0; base < n_bytes; base += 64) {
        const int i = base + lane;
        const bool have = i < n_bytes;
        const uint32_t byte = have ? bit_byte(words, i) : 0u;
        const unsigned long long ff = __ballot(have && byte == 255u);
        const int64_t at = outpos + lane + __popcll(ff & ((1ull << lane) - 1ull));
        if (have) {
          if (at < cap) slot[at] = (uint8_t)byte;
          if (byte == 255u && at + 1 < cap) slot[at + 1] = 0;
        }
        outpos += min(64, n_bytes - base) + __popcll(ff);
      }
      const uint32_t rest = (bitpos & 7) ? bit_byte(words, n_bytes) : 0u;      // the bits left over (the low ones of the byte are zero)
      __syncthreads();
      words[lane] = lane == 0 ? rest << 24 : 0u;
      bitpos &= 7;
      __syncthreads();
    }
  }
  if (lane == 0) {
    if (bitpos) {                                                        // pad with 1-bits
      const uint32_t byte = (words[0] >> 24) | (0xffu >> bitpos);
      if (outpos < cap) slot[outpos] = (uint8_t)byte;
      ++outpos;
      if (byte == 255u) {
        if (outpos < cap) slot[outpos] = 0;
        ++outpos;
      }
    }
    a.lens[frame * a.intervals + interval] = (uint32_t)(outpos < cap ? outpos : cap);
  }
}

// ---- 3. places of the intervals -------------------------------------------------------------------------------------------------------
// dst[f][i] = bytes in front of interval i of frame f in the output: every interval of a frame but its last is followed by two bytes of
// RST.  meta[f] = {offset, length} of frame f.  One workgroup; the runs of the threads and their scan: csrc/codec_stream.h.
__global__ __launch_bounds__(kThreads) void jpeg_scan_kernel(const uint32_t* lens, int64_t* dst, int64_t* meta, const int64_t n_frames,
                                                             const int64_t intervals) {
  const int tid = threadIdx.x;
  int64_t i0, i1;
  codec_run<kThreads>(n_frames * intervals, tid, &i0, &i1);
  int64_t s = 0;
  for (int64_t i = i0; i < i1; ++i) s += (int64_t)lens[i] + ((i % intervals) + 1 < intervals ? 2 : 0);
  s = codec_scan_runs<kThreads>(s, tid);
  for (int64_t i = i0; i < i1; ++i) {
    dst[i] = s;
    s += (int64_t)lens[i] + ((i % intervals) + 1 < intervals ? 2 : 0);
    if ((i % intervals) + 1 == intervals) meta[2 * (i / intervals) + 1] = s;              // the end of the frame, for now
    if (i % intervals == 0) meta[2 * (i / intervals)] = dst[i];
  }
}

// meta[f][1]: end -> length (after the scan, so that no thread reads what another one is writing)
__global__ void jpeg_meta_kernel(int64_t* meta, const int64_t n_frames) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n_frames) meta[2 * f + 1] -= meta[2 * f];
}

// ---- 4. compaction --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void jpeg_compact_kernel(const uint8_t* slots, const uint32_t* lens, const int64_t* dst, uint8_t* out,
                                                                const int64_t slot_bytes, const int64_t intervals, const int64_t out_bytes) {
  const int64_t item = (int64_t)blockIdx.y * intervals + blockIdx.x;
  const uint8_t* src = slots + item * slot_bytes;
  const int64_t n = lens[item], at = dst[item];
  if (at + n + 2 > out_bytes) return;                                    // (the planner sized `out` by the worst case: never taken)
  codec_copy_slot<kThreads>(src, out, at, n, threadIdx.x);
  if (threadIdx.x == 0 && blockIdx.x + 1 < intervals) {
    out[at + n] = 0xff;
    out[at + n + 1] = (uint8_t)(0xd0 + (blockIdx.x & 7));
  }
}

int plan_or_refuse(const char* fn, int64_t n, int64_t h, int64_t w, int quality, int sub, int64_t ri, JpegGeom* g) {
  const int rc = codec_refuse(fn, [&](char* why, size_t len) { return jpeg_plan(n, h, w, quality, sub, ri, g, why, len); });
  if (rc != VQN_OK) return rc;
  uint8_t header[kJpegHeaderCap];
  g->header_bytes = jpeg_header(*g, header, sizeof(header));
  return VQN_OK;
}

}  // namespace

static_assert(kJpegGeomWords == 24, "include/vqn_image_codec.h documents VqnJpegGeom as 24 words");

extern "C" int vqn_jpeg_plan(int64_t n, int64_t h, int64_t w, int quality, int subsampling, int64_t restart_interval, int64_t* geom,
                             uint8_t* header, int header_cap) {
  JpegGeom g;
  const int rc = plan_or_refuse(__func__, n, h, w, quality, subsampling, restart_interval, &g);
  if (rc != VQN_OK) return rc;
  if (geom) memcpy(geom, &g, sizeof(g));
  if (header) {
    VQN_CHECK_ARG(jpeg_header(g, header, header_cap) > 0, "the header does not fit header_cap bytes");
  }
  return VQN_OK;
}

extern "C" int vqn_jpeg_encode(const uint8_t* rgb, int64_t n, int64_t h, int64_t w, int quality, int subsampling, int64_t restart_interval,
                               void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_bytes, int64_t* meta, int coefficients_only,
                               void* stream) {
  JpegGeom g;
  const int rc = plan_or_refuse(__func__, n, h, w, quality, subsampling, restart_interval, &g);
  if (rc != VQN_OK) return rc;
  VQN_CHECK_ARG(rgb && scratch, "null frames or scratch");
  VQN_CHECK_ARG(((uintptr_t)scratch & 15u) == 0u, "scratch is not 16-byte aligned");
  const auto fits = [&](char* why, size_t len) { return jpeg_check_buffers(g, scratch_bytes, out_bytes, coefficients_only, why, len); };
  if (const int fit = codec_refuse(__func__, fits); fit != VQN_OK) return fit;
  VQN_CHECK_ARG(coefficients_only || (out && meta), "null out or meta");
  VQN_CHECK_SHAPE(n <= 65535 && g.intervals <= 0x7fffffff && g.mcus_x * g.mcus_y <= 0x7fffffff, "at most 65535 frames in a batch");
  uint8_t* base = (uint8_t*)scratch;
  hipStream_t s = (hipStream_t)stream;
  DctArgs d;
  d.rgb = rgb;
  d.coef[0] = (int16_t*)base, d.coef[1] = (int16_t*)(base + g.off_cb), d.coef[2] = (int16_t*)(base + g.off_cr);
  d.h = (int)h, d.w = (int)w;
  d.by_y = (int)g.by_y, d.bx_y = (int)g.bx_y, d.by_c = (int)g.by_c, d.bx_c = (int)g.bx_c;
  jpeg_quant_table(kJpegLumaBase, quality, d.q[0]);
  jpeg_quant_table(kJpegChromaBase, quality, d.q[1]);
  const int64_t wp = g.mcus_x * g.mcu, hp = g.mcus_y * g.mcu;
  const dim3 tiles((unsigned)((wp + kTileW - 1) / kTileW), (unsigned)((hp + kTileH - 1) / kTileH), (unsigned)n);
  if (subsampling == 420)
    hipLaunchKernelGGL((jpeg_dct_kernel<true>), tiles, dim3(kThreads), 0, s, d);
  else
    hipLaunchKernelGGL((jpeg_dct_kernel<false>), tiles, dim3(kThreads), 0, s, d);
  VQN_LAUNCH_CHECK();
  if (coefficients_only) return VQN_OK;
  EntropyArgs e;
  for (int i = 0; i < 3; ++i) e.coef[i] = d.coef[i];
  e.slots = base + g.off_slots, e.lens = (uint32_t*)(base + g.off_lens);
  e.by_y = d.by_y, e.bx_y = d.bx_y, e.by_c = d.by_c, e.bx_c = d.bx_c;
  e.mcus_x = (int)g.mcus_x, e.mcus = (int)(g.mcus_x * g.mcus_y), e.ri = (int)g.ri, e.intervals = (int)g.intervals, e.sub420 = subsampling == 420;
  e.slot_bytes = g.slot_bytes;
  jpeg_huff_tables(&e.huff);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)g.intervals, (unsigned)n), dim3(64), 0, s, e);
  VQN_LAUNCH_CHECK();
  int64_t* dst = (int64_t*)(base + g.off_dst);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kThreads), 0, s, e.lens, dst, meta, n, g.intervals);
  VQN_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_meta_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, meta, n);
  VQN_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)g.intervals, (unsigned)n), dim3(kThreads), 0, s, e.slots, e.lens, dst, out,
                     g.slot_bytes, g.intervals, out_bytes);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}
