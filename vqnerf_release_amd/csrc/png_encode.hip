// PNG on the device: uint8 [N, H, W, C] images -> one zlib stream per image, the data of the IDAT chunk of a file whose other bytes
// csrc/png_plan.h and decomp/nerfactor/util/png.py write (the statement of the format is tests/png_model.py).  Four launches and no
// host read:
//
//   1. png_filter_kernel: pixels -> the filtered stream [N][H][stride] (stride = 1 + W C: the filter type, then the row).  One wave per
//      row.  A lane takes four consecutive bytes of the row at a time: with rows of whole, aligned 32-bit words it reads them, the four
//      in front of them and the two words above as four 32-bit loads (byte loads otherwise); the left and upper-left neighbours are
//      C bytes back in the pair of words.  In adaptive mode the sums of |residual as int8| of the five types are wave reductions, the
//      smallest (the lower type on a tie) is written in a second pass over the row.
//   2. png_deflate_kernel: one wave per (image, segment).  64 positions of the segment at a time: for each of the nine candidate
//      distances a ballot of b[p] == b[p - d] -- the ballots of this window and of the five behind it are carried in registers, 258
//      positions ahead -- gives every lane its match length by bit scans; the greedy parse of the window is a pointer-jumping pass
//      over next[p] = p + max(1, length) from the position the previous window's last token ran to.  A first pass over the segment
//      adds up the bits of the tokens under every coding (the dynamic tables, fixed Huffman) and the Adler-32 sums, the smallest byte
//      size (stored included) is chosen, and a second pass re-runs the same tokeniser and emits: every token lane forms its own bits,
//      a wave prefix sum places them, LDS ORs on disjoint bits assemble them and whole bytes go to the segment's slot.  Every store is
//      guarded by the slot size and every loop bounded by the segment length; no workgroup waits for another.
//   3. png_scan_kernel: one workgroup: the place of every segment in the output (images back to back, 78 01 in front of and the
//      Adler-32 behind the segments of an image), the [N][2] offset and length of every stream, and the Adler-32 of every image from
//      the pairs of its segments, combined in order by zlib's adler32_combine rule.
//   4. png_compact_kernel: one workgroup per (segment, image) copies the slot to its place; the first and the last of an image add
//      the two bytes in front and the four behind.
// Integer work throughout: equal images give equal bytes.
#include "codec_stream.h"
#include "common.h"
#include "png_plan.h"
#include "wave.h"
#include "vqn_image_codec.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerGroup = kThreads / 64;
constexpr uint32_t kAdlerBase = 65521u;

__constant__ PngTables c_tables = png_make_tables();

// ---- 1. filtering ---------------------------------------------------------------------------------------------------------------------
struct FilterArgs {
  const uint8_t* pix;                        // [N][H][W C]
  uint8_t* filtered;                         // [N][H][1 + W C]
  int h, row_bytes, c, mode, wide;
};

// bytes i .. i + 3 of a row of n bytes, byte i in the low bits; zero in front of the row, behind it and for a missing row
__device__ __forceinline__ uint32_t row_word(const uint8_t* row, const int i, const int n, const bool wide) {
  if (row == nullptr || i < 0 || i >= n) return 0u;
  if (wide) return *(const uint32_t*)(row + i);          // (n and the row's address are multiples of 4)
  uint32_t v = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (i + j < n) v |= (uint32_t)row[i + j] << (8 * j);
  return v;
}

__device__ __forceinline__ int byte_of(const unsigned long long pair, const int i) { return (int)((pair >> (8 * i)) & 255ull); }

// the residual of type t for x with neighbours a (left), b (up), c (up-left), as a byte
__device__ __forceinline__ int residual(const int t, const int x, const int a, const int b, const int c) {
  int pred = 0;
  if (t == 1) pred = a;
  else if (t == 2) pred = b;
  else if (t == 3) pred = (a + b) >> 1;
  else if (t == 4) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (x - pred) & 255;
}

__device__ __forceinline__ int abs_int8(const int r) { return r < 128 ? r : 256 - r; }

__global__ __launch_bounds__(kThreads) void png_filter_kernel(const FilterArgs a) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6);
  if (y >= a.h) return;                                   // (whole waves leave: no barrier below)
  const int64_t image = blockIdx.y;
  const int n = a.row_bytes;
  const uint8_t* row = a.pix + (image * a.h + y) * n;
  const uint8_t* above = y ? row - n : nullptr;
  uint8_t* out = a.filtered + (image * a.h + y) * (n + 1);
  const bool wide = a.wide != 0;
  int type = a.mode;
  if (a.mode == kPngFilterAdaptive) {
    int sums[5] = {0, 0, 0, 0, 0};
    for (int i = lane * 4; i < n; i += 256) {
      const unsigned long long cur = (unsigned long long)row_word(row, i, n, wide) << 32 | row_word(row, i - 4, n, wide);
      const unsigned long long up = (unsigned long long)row_word(above, i, n, wide) << 32 | row_word(above, i - 4, n, wide);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i + j >= n) continue;
        const int x = byte_of(cur, 4 + j), l = byte_of(cur, 4 + j - a.c), u = byte_of(up, 4 + j), ul = byte_of(up, 4 + j - a.c);
#pragma unroll
        for (int t = 0; t < 5; ++t) sums[t] += abs_int8(residual(t, x, l, u, ul));
      }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) sums[t] += __shfl_xor(sums[t], d, 64);
    type = 0;
#pragma unroll
    for (int t = 1; t < 5; ++t)
      if (sums[t] < sums[type]) type = t;
  }
  if (lane == 0) out[0] = (uint8_t)type;
  for (int i = lane * 4; i < n; i += 256) {
    const unsigned long long cur = (unsigned long long)row_word(row, i, n, wide) << 32 | row_word(row, i - 4, n, wide);
    const unsigned long long up = (unsigned long long)row_word(above, i, n, wide) << 32 | row_word(above, i - 4, n, wide);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j >= n) continue;
      out[1 + i + j] = (uint8_t)residual(type, byte_of(cur, 4 + j), byte_of(cur, 4 + j - a.c), byte_of(up, 4 + j), byte_of(up, 4 + j - a.c));
    }
  }
}

// ---- 2. deflate -----------------------------------------------------------------------------------------------------------------------
struct DeflateArgs {
  const uint8_t* filtered;                   // [N][image_bytes]
  uint8_t* slots;                            // [N][segments][slot_bytes]
  uint32_t* lens;                            // [N][segments]: bytes of the segment's slot that are used
  uint32_t* adler;                           // [N][segments][2]: s1, s2 of the segment's bytes alone
  int64_t image_bytes, slot_bytes;
  int segments, segment_bytes;
  PngCandidate cand[kPngCandidates];
};

constexpr int kAhead = 6;                    // windows of ballots a lane looks through: 64 - lane + 5 * 64 >= 258 positions
constexpr int kBitWords = 104;               // LDS words of the bit buffer: 7 bits left over + 64 tokens of 48 bits, and slack
static_assert((7 + 64 * 48 + 31) / 32 + 3 <= kBitWords, "a window's tokens fit the bit buffer");
static_assert(kPngHeaderWords + 2 <= kBitWords, "a block header fits the bit buffer");
static_assert(64 + (kAhead - 1) * 64 - 63 >= kPngMaxMatch, "the carried ballots cover the longest match from the last lane");

// length 3 .. 258 -> its symbol less 257, with the number and the value of its extra bits
__device__ __forceinline__ int len_symbol(const int len, int* extra_bits, int* extra) {
  *extra_bits = 0, *extra = 0;
  if (len == kPngMaxMatch) return 28;
  const int l = len - kPngMinMatch;
  if (l < 8) return l;
  const int e = 29 - __clz(l);
  *extra_bits = e, *extra = l & ((1 << e) - 1);
  return 4 + 4 * e + ((l >> e) & 3);
}

// The tokeniser of a segment: b[0 .. L) are its bytes, s0 bytes of the image's stream lie in front of b.  window() hands every lane
// what stands at its position of the window at hand; advance() moves on by 64 positions.
struct Tokeniser {
  const uint8_t* b;
  int64_t s0;
  int L, lane;
  int d[kPngCandidates];
  unsigned long long eq[kPngCandidates][kAhead];         // eq[k][j]: the ballot of b[q] == b[q - d[k]] over window (at hand + j)
  int at;                                    // the window at hand
  int start;                                 // where its first token begins, from the window's first position (>= 64: in a later one)

  template <int J>
  __device__ __forceinline__ void fill(const int w) {
    const int q = w * 64 + lane;
    const bool in = q < L;
    const int x = in ? (int)b[q] : -1;
#pragma unroll
    for (int k = 0; k < kPngCandidates; ++k) {
      const bool ok = in && d[k] > 0 && s0 + q - d[k] >= 0;
      const int y = ok ? (int)b[q - d[k]] : -2;
      eq[k][J] = __ballot(x == y);
    }
  }

  __device__ __forceinline__ void begin(const DeflateArgs& a, const uint8_t* bytes, const int64_t in_front, const int len, const int ln) {
    b = bytes, s0 = in_front, L = len, lane = ln, at = 0, start = 0;
#pragma unroll
    for (int k = 0; k < kPngCandidates; ++k) d[k] = a.cand[k].d;
    fill<0>(0), fill<1>(1), fill<2>(2), fill<3>(3), fill<4>(4), fill<5>(5);
  }

  __device__ __forceinline__ void advance() {
    ++at;
#pragma unroll
    for (int k = 0; k < kPngCandidates; ++k)
#pragma unroll
      for (int j = 0; j + 1 < kAhead; ++j) eq[k][j] = eq[k][j + 1];
    fill<kAhead - 1>(at + kAhead - 1);
  }

  // -> whether a token begins at this lane's position; *len its length (1: a literal), *k the candidate of a match, *x the byte at
  // the position (-1 behind the segment's end).  mark: two LDS words.
  __device__ __forceinline__ bool window(uint32_t* mark, int* len, int* k, int* x) {
    const int q = at * 64 + lane;
    *x = q < L ? (int)b[q] : -1;
    *len = 1, *k = 0;
    if (start >= 64) {                                     // a match of an earlier window covers this one
      start -= 64;
      return false;
    }
    int best = 0, best_k = 0;
#pragma unroll
    for (int c = 0; c < kPngCandidates; ++c) {
      int tail = 0;                                        // matching positions from the next window's first on (the same in every lane)
#pragma unroll
      for (int j = 1; j < kAhead; ++j) {
        const unsigned long long miss = ~eq[c][j];
        if (tail == 64 * (j - 1)) tail += miss ? __ffsll((long long)miss) - 1 : 64;
      }
      const unsigned long long miss = ~eq[c][0] >> lane;   // (the zeros shifted in at the top are no misses: handled below)
      const int here = miss ? __ffsll((long long)miss) - 1 : 64;
      int n = here < 64 - lane ? here : 64 - lane + tail;
      n = min(n, kPngMaxMatch);
      if (n > best) best = n, best_k = c;
    }
    const int step = best >= kPngMinMatch ? best : 1;
    // the positions the parse visits: pointer jumping over next = lane + step from `start`
    if (lane < 2) mark[lane] = 0u;
    __syncthreads();
    if (lane == start) atomicOr(&mark[lane >> 5], 1u << (lane & 31));
    __syncthreads();
    int jump = min(lane + step, 64);                       // 64: out of the window
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const bool marked = (mark[lane >> 5] >> (lane & 31)) & 1u;
      __syncthreads();
      if (marked && jump < 64) atomicOr(&mark[jump >> 5], 1u << (jump & 31));
      const int further = __shfl(jump, min(jump, 63), 64);
      jump = jump < 64 ? further : 64;
      __syncthreads();
    }
    const unsigned long long visited = (unsigned long long)mark[1] << 32 | mark[0];
    const int valid = min(64, L - at * 64);                // positions of the window inside the segment (>= 1)
    const unsigned long long tokens = valid == 64 ? visited : visited & ((1ull << valid) - 1ull);
    const int last = 63 - __clzll((long long)tokens);      // (`start` is a token: never empty)
    start = __shfl(lane + step, last, 64) - 64;
    __syncthreads();                                       // (mark is free again)
    *len = step, *k = best_k;
    return (tokens >> lane) & 1ull;
  }
};

__global__ __launch_bounds__(64) void png_deflate_kernel(const DeflateArgs a) {
  __shared__ uint8_t lit_len[kPngCodings][288];
  __shared__ uint8_t dist_len[kPngCodings][16];            // by candidate
  __shared__ uint32_t codes[288];                          // of the chosen coding
  __shared__ uint32_t dist_code[16];                       // ... by candidate
  __shared__ int cand_extra_bits[16], cand_extra[16];
  __shared__ uint32_t words[kBitWords];
  __shared__ uint32_t mark[2];
  const int lane = threadIdx.x;
  const int seg = blockIdx.x;
  const int64_t image = blockIdx.y;
  const int64_t s0 = (int64_t)seg * a.segment_bytes;
  const int L = (int)min((int64_t)a.segment_bytes, a.image_bytes - s0);
  const uint8_t* b = a.filtered + image * a.image_bytes + s0;
  const int64_t item = image * a.segments + seg;
  uint8_t* slot = a.slots + item * a.slot_bytes;
  const int64_t cap = a.slot_bytes;
  const bool final_block = seg + 1 == a.segments;
  const int n_windows = (L + 63) / 64;

  for (int i = lane; i < kPngCodings * 288; i += 64) lit_len[i / 288][i % 288] = (uint8_t)(c_tables.lit[i / 288][i % 288] >> 16);
  if (lane < kPngCandidates) {
    cand_extra_bits[lane] = a.cand[lane].extra_bits, cand_extra[lane] = a.cand[lane].extra;
    for (int t = 0; t < kPngCodings; ++t) dist_len[t][lane] = (uint8_t)(c_tables.dist[t][a.cand[lane].symbol] >> 16);
  }
  __syncthreads();

  // ---- pass 1: the bits of the tokens under every coding, the Adler-32 sums ----
  Tokeniser tk;
  tk.begin(a, b, s0, L, lane);
  int cost[kPngCodings];
#pragma unroll
  for (int t = 0; t < kPngCodings; ++t) cost[t] = 0;
  int extra_bits = 0;
  unsigned long long sum = 0ull, weighted = 0ull;
  for (int w = 0; w < n_windows; ++w) {
    int len, k, x;
    const bool token = tk.window(mark, &len, &k, &x);
    if (x >= 0) sum += (unsigned)x, weighted += (unsigned long long)(L - (w * 64 + lane)) * (unsigned)x;
    if (token) {
      if (len >= kPngMinMatch) {
        int eb, ev;
        const int s = 257 + len_symbol(len, &eb, &ev);
        extra_bits += eb + cand_extra_bits[k];
#pragma unroll
        for (int t = 0; t < kPngCodings; ++t) cost[t] += lit_len[t][s] + dist_len[t][k];
      } else {
#pragma unroll
        for (int t = 0; t < kPngCodings; ++t) cost[t] += lit_len[t][x];
      }
    }
    tk.advance();
  }
  extra_bits = wave_sum(extra_bits);
  int choice = kPngCodings;                                // stored
  int64_t best_bytes = 5 + (int64_t)L;
#pragma unroll
  for (int t = kPngCodings - 1; t >= 0; --t) {             // (backwards with <=: the earlier candidate on a tie)
    const int64_t bits = (int64_t)c_tables.header_bits[t] + wave_sum(cost[t]) + extra_bits + lit_len[t][256];
    const int64_t bytes = (bits + 3 + 7) / 8 + 4;          // + the empty stored block: 3 bits, padding, 00 00 FF FF
    if (bytes <= best_bytes) best_bytes = bytes, choice = t;
  }
  {
    const unsigned long long all_weighted = wave_sum(weighted), all = wave_sum(sum);
    if (lane == 0) {
      a.adler[2 * item] = (uint32_t)((1ull + all) % kAdlerBase);
      a.adler[2 * item + 1] = (uint32_t)(((unsigned long long)L + all_weighted) % kAdlerBase);
    }
  }

  // ---- stored ----
  if (choice == kPngCodings) {
    if (lane == 0 && cap >= 5) {
      slot[0] = final_block ? 1 : 0;
      slot[1] = (uint8_t)(L & 255), slot[2] = (uint8_t)(L >> 8);
      slot[3] = (uint8_t)(~L & 255), slot[4] = (uint8_t)((~L >> 8) & 255);
    }
    for (int i = lane; i < L; i += 64)
      if (5 + (int64_t)i < cap) slot[5 + i] = b[i];
    if (lane == 0) a.lens[item] = (uint32_t)min((int64_t)L + 5, cap);
    return;
  }

  // ---- pass 2: the same tokens again, emitted under the chosen coding ----
  for (int i = lane; i < 288; i += 64) codes[i] = c_tables.lit[choice][i];
  if (lane < kPngCandidates) dist_code[lane] = c_tables.dist[choice][a.cand[lane].symbol];
  for (int i = lane; i < kBitWords; i += 64) words[i] = i < kPngHeaderWords ? c_tables.header[choice][i] : 0u;
  __syncthreads();
  int bitpos = (int)c_tables.header_bits[choice];          // bits waiting in `words`
  int64_t outpos = 0;                                      // bytes of the slot written
  // whole bytes of `words` -> the slot; the bits left over start the buffer again.  all: the last, padded byte too.
  auto flush = [&](const bool all) {
    const int n_bytes = all ? (bitpos + 7) >> 3 : bitpos >> 3;
    for (int base = 0; base < n_bytes; base += 64) {
      const int i = base + lane;
      if (i < n_bytes && outpos + i < cap) slot[outpos + i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
    }
    outpos += n_bytes;
    const uint32_t rest = (!all && (bitpos & 7)) ? (words[n_bytes >> 2] >> (8 * (n_bytes & 3))) & 255u : 0u;
    __syncthreads();
    for (int i = lane; i < kBitWords; i += 64) words[i] = i == 0 ? rest : 0u;
    bitpos = all ? 0 : bitpos & 7;
    __syncthreads();
  };
  auto place = [&](const unsigned long long acc, const int n, const int p) {      // n <= 48 bits of acc at bit p of `words`
    if (n > 0) {
      const int w = p >> 5, s = p & 31;
      const unsigned long long lo = acc << s;
      const uint32_t hi = s ? (uint32_t)(acc >> (64 - s)) : 0u;
      if ((uint32_t)lo) atomicOr(&words[w], (uint32_t)lo);
      if ((uint32_t)(lo >> 32)) atomicOr(&words[w + 1], (uint32_t)(lo >> 32));
      if (hi) atomicOr(&words[w + 2], hi);
    }
  };
  flush(false);
  tk.begin(a, b, s0, L, lane);
  for (int w = 0; w < n_windows; ++w) {
    int len, k, x;
    const bool token = tk.window(mark, &len, &k, &x);
    unsigned long long acc = 0ull;
    int n = 0;
    if (token) {
      if (len >= kPngMinMatch) {
        int eb, ev;
        const uint32_t e = codes[257 + len_symbol(len, &eb, &ev)], de = dist_code[k];
        acc = e & 0xffffu, n = (int)(e >> 16);
        acc |= (unsigned long long)ev << n, n += eb;
        acc |= (unsigned long long)(de & 0xffffu) << n, n += (int)(de >> 16);
        acc |= (unsigned long long)cand_extra[k] << n, n += cand_extra_bits[k];
      } else {
        const uint32_t e = codes[x];
        acc = e & 0xffffu, n = (int)(e >> 16);
      }
    }
    int total;
    const int p = bitpos + wave_exclusive_sum(n, lane, &total);
    place(acc, n, p);
    bitpos += total;
    __syncthreads();
    flush(false);
    tk.advance();
  }
  {                                                        // end of block, then the empty stored block: BFINAL, 00, padding
    const uint32_t e = codes[256];
    const int n = (int)(e >> 16);
    if (lane == 0) place((unsigned long long)(e & 0xffffu) | (unsigned long long)(final_block ? 1 : 0) << n, n + 3, bitpos);
    bitpos += n + 3;
    __syncthreads();
    flush(true);
  }
  if (lane < 4 && outpos + lane < cap) slot[outpos + lane] = lane < 2 ? 0x00 : 0xff;
  outpos += 4;
  if (lane == 0) a.lens[item] = (uint32_t)min(outpos, cap);
}

// ---- 3. places of the segments, the Adler-32 of the images ----------------------------------------------------------------------------
// Thread t takes a run of the images (codec_run): the length of each stream (2 + its segments + 4) and its Adler-32, then, after the
// scan of the runs' totals (codec_scan_runs written out: as a call it costs this kernel two scalar registers), dst and meta.
__global__ __launch_bounds__(kThreads) void png_scan_kernel(const uint32_t* lens, const uint32_t* adler, int64_t* dst, uint32_t* sums,
                                                            int64_t* meta, const int64_t n_images, const int64_t segments,
                                                            const int64_t segment_bytes, const int64_t image_bytes) {
  __shared__ int64_t totals[kThreads];
  const int tid = threadIdx.x;
  int64_t i0, i1;
  codec_run<kThreads>(n_images, tid, &i0, &i1);
  int64_t total = 0;
  for (int64_t i = i0; i < i1; ++i) {
    unsigned long long s1 = 1ull, s2 = 0ull;               // of the bytes so far
    int64_t bytes = 6;
    for (int64_t s = 0; s < segments; ++s) {
      bytes += lens[i * segments + s];
      const unsigned long long len2 = (unsigned long long)min(segment_bytes, image_bytes - s * segment_bytes) % kAdlerBase;
      const unsigned long long a2 = adler[2 * (i * segments + s)], b2 = adler[2 * (i * segments + s) + 1];
      s2 = (s2 + b2 + len2 * ((s1 + kAdlerBase - 1ull) % kAdlerBase)) % kAdlerBase;
      s1 = (s1 + a2 + kAdlerBase - 1ull) % kAdlerBase;
    }
    sums[i] = (uint32_t)(s2 << 16 | s1);
    total += bytes;
  }
  totals[tid] = total;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < kThreads; ++t) {
      const int64_t v = totals[t];
      totals[t] = run;
      run += v;
    }
  }
  __syncthreads();
  int64_t at = totals[tid];
  for (int64_t i = i0; i < i1; ++i) {
    meta[2 * i] = at;
    at += 2;
    for (int64_t s = 0; s < segments; ++s) {
      dst[i * segments + s] = at;
      at += lens[i * segments + s];
    }
    at += 4;
    meta[2 * i + 1] = at - meta[2 * i];
  }
}

// ---- 4. compaction --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void png_compact_kernel(const uint8_t* slots, const uint32_t* lens, const int64_t* dst,
                                                               const uint32_t* sums, uint8_t* out, const int64_t slot_bytes,
                                                               const int64_t segments, const int64_t out_bytes) {
  const int64_t image = blockIdx.y, item = image * segments + blockIdx.x;
  const uint8_t* src = slots + item * slot_bytes;
  const int64_t n = min((int64_t)lens[item], slot_bytes), at = dst[item];
  if (at < 2 || at + n + 4 > out_bytes) return;            // (the planner sized `out` by the worst case: never taken)
  codec_copy_slot<kThreads>(src, out, at, n, threadIdx.x);
  if (threadIdx.x == 0 && blockIdx.x == 0) out[at - 2] = 0x78, out[at - 1] = 0x01;
  if (threadIdx.x < 4 && blockIdx.x + 1 == segments) out[at + n + threadIdx.x] = (uint8_t)(sums[image] >> (24 - 8 * threadIdx.x));
}

int plan_or_refuse(const char* fn, int64_t n, int64_t h, int64_t w, int64_t c, int filter_mode, int64_t rows_per_segment, PngGeom* g) {
  return codec_refuse(fn, [&](char* why, size_t len) { return png_plan(n, h, w, c, filter_mode, rows_per_segment, g, why, len); });
}

}  // namespace

static_assert(kPngGeomWords == 17, "include/vqn_image_codec.h documents VqnPngGeom as 17 words");

extern "C" int vqn_png_plan(int64_t n, int64_t h, int64_t w, int64_t c, int filter_mode, int64_t rows_per_segment, int64_t* geom,
                            uint8_t* head, int head_cap) {
  PngGeom g;
  const int rc = plan_or_refuse(__func__, n, h, w, c, filter_mode, rows_per_segment, &g);
  if (rc != VQN_OK) return rc;
  if (geom) memcpy(geom, &g, sizeof(g));
  if (head) {
    VQN_CHECK_ARG(png_head(g, head, head_cap) > 0, "the head does not fit head_cap bytes");
  }
  return VQN_OK;
}

extern "C" int vqn_png_encode(const uint8_t* pix, int64_t n, int64_t h, int64_t w, int64_t c, int filter_mode, int64_t rows_per_segment,
                              void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_bytes, int64_t* meta, int filtered_only,
                              void* stream) {
  PngGeom g;
  const int rc = plan_or_refuse(__func__, n, h, w, c, filter_mode, rows_per_segment, &g);
  if (rc != VQN_OK) return rc;
  VQN_CHECK_ARG(pix && scratch, "null images or scratch");
  VQN_CHECK_ARG(((uintptr_t)scratch & 15u) == 0u, "scratch is not 16-byte aligned");
  const auto fits = [&](char* why, size_t len) { return png_check_buffers(g, scratch_bytes, out_bytes, filtered_only, why, len); };
  if (const int fit = codec_refuse(__func__, fits); fit != VQN_OK) return fit;
  VQN_CHECK_ARG(filtered_only || (out && meta), "null out or meta");
  uint8_t* base = (uint8_t*)scratch;
  hipStream_t s = (hipStream_t)stream;
  FilterArgs f;
  f.pix = pix, f.filtered = base;
  f.h = (int)h, f.row_bytes = (int)(w * c), f.c = (int)c, f.mode = filter_mode;
  f.wide = (f.row_bytes % 4 == 0 && ((uintptr_t)pix & 3u) == 0u) ? 1 : 0;
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((h + kRowsPerGroup - 1) / kRowsPerGroup), (unsigned)n), dim3(kThreads), 0, s, f);
  VQN_LAUNCH_CHECK();
  if (filtered_only) return VQN_OK;
  DeflateArgs d;
  d.filtered = base, d.slots = base + g.off_slots;
  d.lens = (uint32_t*)(base + g.off_lens), d.adler = (uint32_t*)(base + g.off_adler);
  d.image_bytes = h * g.stride, d.slot_bytes = g.slot_bytes;
  d.segments = (int)g.segments, d.segment_bytes = (int)g.segment_bytes;
  png_candidates(g.stride, c, d.cand);
  hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)g.segments, (unsigned)n), dim3(64), 0, s, d);
  VQN_LAUNCH_CHECK();
  int64_t* dst = (int64_t*)(base + g.off_dst);
  uint32_t* sums = (uint32_t*)(base + g.off_sums);
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(kThreads), 0, s, d.lens, d.adler, dst, sums, meta, n, g.segments, g.segment_bytes,
                     d.image_bytes);
  VQN_LAUNCH_CHECK();
  hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)g.segments, (unsigned)n), dim3(kThreads), 0, s, d.slots, d.lens, dst, sums, out,
                     g.slot_bytes, g.segments, out_bytes);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}
