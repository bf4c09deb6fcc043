// AddressSanitizer / UBSan check of the host-only C++ of the device PNG encoder (csrc/png_plan.h): the 33 bytes in front of IDAT of two
// geometries and the pre-encoded block headers of two tables against bytes written by the numpy model (tests/png_model.py:
// head(17, 23, 3), head(800, 640, 2), the headers of tables 0 and 13 behind a BFINAL bit of 0), the header lengths of every coding,
// canonical codes, the geometry at its bounds, the candidate distances, and every refusal with its reason.  Built and run by
// tests/test_png_plan_native.py:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Ivqnerf_release_amd/csrc tests/native/png_plan_host.cpp
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "png_plan.h"

static const uint8_t kHeadA[33] = {0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a, 0x00, 0x00, 0x00, 0x0d, 0x49, 0x48, 0x44, 0x52, 0x00,
                                   0x00, 0x00, 0x17, 0x00, 0x00, 0x00, 0x11, 0x08, 0x02, 0x00, 0x00, 0x00, 0xb9, 0x11, 0xa0, 0xea};
static const uint8_t kHeadB[33] = {0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a, 0x00, 0x00, 0x00, 0x0d, 0x49, 0x48, 0x44, 0x52, 0x00,
                                   0x00, 0x02, 0x80, 0x00, 0x00, 0x03, 0x20, 0x08, 0x04, 0x00, 0x00, 0x00, 0x19, 0xaf, 0x1b, 0xf2};
static const int kHeaderBits[15] = {419, 404, 487, 462, 536, 534, 409, 412, 411, 395, 355, 355, 327, 328, 3};
static const uint8_t kTableHeader0[53] = {0xec, 0xfd, 0x03, 0xa0, 0x6c, 0xd9, 0x96, 0xad, 0x8d, 0x7e, 0xad, 0xf7, 0x11, 0x6b, 0x67, 0x56, 0xdd, 0x67,
                                          0xdb, 0xb6, 0x6d, 0xdb, 0xb6, 0x6d, 0xdb, 0xb6, 0x6d, 0xdb, 0xb6, 0x6d, 0xdb, 0xf6, 0xfb, 0x6f, 0x9d, 0xdc,
                                          0x2b, 0xe6, 0xe8, 0xad, 0x9d, 0x88, 0xa5, 0xad, 0xe4, 0x51, 0x69, 0x7e, 0x5d, 0xd3, 0xf6, 0x1c, 0x00};
static const uint8_t kTableHeader13[41] = {0xec, 0x9d, 0x03, 0x80, 0x5d, 0xd7, 0x16, 0x86, 0xc7, 0xb6, 0x19, 0xdb, 0xb6, 0x9d,
                                           0xda, 0xb6, 0xed, 0xf6, 0xd9, 0xae, 0x6d, 0xdb, 0x6e, 0x6c, 0xdb, 0x76, 0x32, 0xb6,
                                           0xad, 0xb7, 0xb6, 0x8e, 0x2e, 0x47, 0x51, 0xff, 0x6f, 0xe9, 0xd8, 0x3e, 0x1b};

static int failures = 0;
static void expect(bool ok, const char* what, const char* msg) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s (%s)\n", what, msg);
    ++failures;
  }
}

static void head_equals(int64_t h, int64_t w, int64_t c, const uint8_t* want, const char* what) {
  PngGeom g;
  char msg[256] = "";
  expect(png_plan(1, h, w, c, kPngFilterAdaptive, 1, &g, msg, sizeof(msg)) == 0, what, msg);
  std::vector<uint8_t> exact((size_t)kPngHeadBytes);           // exact-size heap buffer: a byte past it is an ASan report
  expect(png_head(g, exact.data(), kPngHeadBytes) == kPngHeadBytes && memcmp(exact.data(), want, kPngHeadBytes) == 0, what,
         "the bytes in front of IDAT differ from the table");
  std::vector<uint8_t> small((size_t)kPngHeadBytes - 1);
  expect(png_head(g, small.data(), kPngHeadBytes - 1) == -1, what, "a buffer one byte short is refused");
}

static void header_equals(const PngTables& t, int k, const uint8_t* want, int want_len, const char* what) {
  const int bits = (int)t.header_bits[k];
  expect((bits + 7) / 8 == want_len, what, "header length");
  bool same = true;
  for (int i = 0; i < want_len; ++i) same = same && (uint8_t)(t.header[k][i >> 2] >> (8 * (i & 3))) == want[i];
  expect(same, what, "header bytes differ from the table");
  for (int i = bits; i < kPngHeaderWords * 32; ++i) same = same && !(t.header[k][i >> 5] >> (i & 31) & 1u);
  expect(same, what, "bits behind the header are zero");
}

static int refusals = 0;
static void refused(int64_t n, int64_t h, int64_t w, int64_t c, int mode, int64_t rows, int want_rc, const char* reason) {
  PngGeom g;
  char msg[256] = "";
  const int rc = png_plan(n, h, w, c, mode, rows, &g, msg, sizeof(msg));
  expect(rc == want_rc && strstr(msg, reason) != nullptr, reason, msg);
  expect(g.scratch_bytes == 0 && g.segments == 0, "a refused plan is left zeroed", msg);
  ++refusals;
}

int main() {
  head_equals(17, 23, 3, kHeadA, "head of 17 x 23, 3 channels");
  head_equals(800, 640, 2, kHeadB, "head of 800 x 640, 2 channels");

  const PngTables& t = png_tables();
  for (int k = 0; k < kPngCodings; ++k) expect((int)t.header_bits[k] == kHeaderBits[k] && kHeaderBits[k] <= kPngHeaderWords * 32, "header bits", "");
  header_equals(t, 0, kTableHeader0, (int)sizeof(kTableHeader0), "block header of table 0");
  header_equals(t, 13, kTableHeader13, (int)sizeof(kTableHeader13), "block header of table 13");
  expect(t.header[kPngTables][0] == 2u, "fixed Huffman: BFINAL 0, BTYPE 01", "");
  // canonical codes, bit-reversed: table 3 and fixed Huffman against the model's (code, length)
  expect(t.lit[3][0] == (3u << 16 | png_reverse_bits(0x0u, 3)) && t.lit[3][256] == (11u << 16 | png_reverse_bits(0x7eeu, 11)) &&
             t.lit[3][285] == (3u << 16 | png_reverse_bits(0x1u, 3)) && t.dist[3][29] == (5u << 16 | png_reverse_bits(0x15u, 5)),
         "codes of table 3", "");
  expect(t.lit[14][0] == (8u << 16 | png_reverse_bits(0x30u, 8)) && t.lit[14][144] == (9u << 16 | png_reverse_bits(0x190u, 9)) &&
             t.lit[14][256] == (7u << 16) && t.lit[14][280] == (8u << 16 | png_reverse_bits(0xc0u, 8)) &&
             t.dist[14][29] == (5u << 16 | png_reverse_bits(0x1du, 5)),
         "codes of fixed Huffman", "");
  expect(png_reverse_bits(0x1u, 15) == 0x4000u && png_reverse_bits(0x6u, 3) == 0x3u, "bit reversal", "");
  for (int k = 0; k < kPngCodings; ++k) {                      // every set complete, every symbol coded, no code over 15 bits
    uint32_t kraft_lit = 0, kraft_dist = 0;
    bool all = true;
    for (int s = 0; s < (k < kPngTables ? 286 : 288); ++s) {
      const uint32_t n = t.lit[k][s] >> 16;
      all = all && n >= 1 && n <= 15;
      if (n >= 1 && n <= 15) kraft_lit += 1u << (15 - n);
    }
    for (int s = 0; s < 30; ++s) {
      const uint32_t n = t.dist[k][s] >> 16;
      all = all && n >= 1 && n <= 15;
      if (n >= 1 && n <= 15) kraft_dist += 1u << (15 - n);
    }
    expect(all && kraft_lit == 1u << 15 && (k < kPngTables ? kraft_dist == 1u << 15 : kraft_dist == 30u << 10), "Kraft sums", "");
  }

  PngGeom g;
  char msg[256] = "";
  // geometry: 3 images of 33 x 17 x 3 in segments of 2 rows
  expect(png_plan(3, 33, 17, 3, 0, 2, &g, msg, sizeof(msg)) == 0, "plan", msg);
  expect(g.stride == 52 && g.segments == 17 && g.segment_bytes == 104 && g.slot_bytes == 112 && g.rows_per_segment == 2, "geometry", msg);
  expect(g.off_slots == 5152 && g.off_lens == g.off_slots + 3 * 17 * 112 && g.off_adler == g.off_lens + 208 &&
             g.off_dst == g.off_adler + 416 && g.off_sums == g.off_dst + 3 * 17 * 8 && g.scratch_bytes == g.off_sums + 16,
         "scratch regions", msg);
  expect(g.out_bytes == 3 * (2 + 33 * 52 + 5 * 17 + 4), "the output holds every segment stored", msg);
  // more rows than the image: one segment; the default; the bounds
  expect(png_plan(1, 5, 7, 4, 5, 1000, &g, msg, sizeof(msg)) == 0 && g.rows_per_segment == 5 && g.segments == 1 && g.segment_bytes == 145, "rows past the image", msg);
  expect(png_default_rows(800, 3) == 3 && png_default_rows(64, 3) == 42 && png_default_rows(65534, 1) == 1, "default rows", "");
  expect(png_plan(1, 1, 1, 1, 0, 1, &g, msg, sizeof(msg)) == 0 && g.stride == 2 && g.slot_bytes == 16, "1 x 1", msg);
  expect(png_plan(65535, 2, 65534, 1, 5, 1, &g, msg, sizeof(msg)) == 0 && g.stride == 65535 && g.segments == 2 && g.slot_bytes == 65552, "the limits", msg);
  expect(png_plan(1, 1 << 24, 16383, 4, 5, 1, &g, msg, sizeof(msg)) == 0 && g.stride == 65533 && g.scratch_bytes > g.off_slots, "2^24 rows", msg);

  // buffers against the plan
  expect(png_plan(2, 16, 16, 3, 5, 2, &g, msg, sizeof(msg)) == 0, "plan", msg);
  expect(png_check_buffers(g, g.scratch_bytes, g.out_bytes, 0, msg, sizeof(msg)) == 0, "exact buffers pass", msg);
  expect(png_check_buffers(g, 2 * 16 * 49, 0, 1, msg, sizeof(msg)) == 0, "filtered only: the stream suffices", msg);
  expect(png_check_buffers(g, g.scratch_bytes, g.out_bytes - 1, 0, msg, sizeof(msg)) == -1 && strstr(msg, "byte total of up to") &&
             strstr(msg, "over the buffer"), "a byte total over the buffer", msg);
  ++refusals;
  expect(png_check_buffers(g, g.scratch_bytes - 1, g.out_bytes, 0, msg, sizeof(msg)) == -1 && strstr(msg, "the scratch holds"), "a small scratch", msg);
  ++refusals;
  expect(png_check_buffers(g, 2 * 16 * 49 - 1, 0, 1, msg, sizeof(msg)) == -1 && strstr(msg, "the scratch holds"), "a small scratch, filtered only", msg);
  ++refusals;

  // candidate distances: 1, 2, 3, 4, 6, 8, stride - c, stride, stride + c with their distance symbols; over 32768: dropped
  PngCandidate cand[kPngCandidates];
  png_candidates(2401, 3, cand);
  expect(cand[0].d == 1 && cand[0].symbol == 0 && cand[4].d == 6 && cand[4].symbol == 4 && cand[4].extra_bits == 1 && cand[4].extra == 1 &&
             cand[5].d == 8 && cand[5].symbol == 5 && cand[5].extra == 1, "short candidates", "");
  expect(cand[6].d == 2398 && cand[6].symbol == 22 && cand[6].extra_bits == 10 && cand[6].extra == 2398 - 2049 && cand[8].d == 2404, "stride candidates", "");
  png_candidates(32768, 4, cand);
  expect(cand[6].d == 32764 && cand[7].d == 32768 && cand[7].symbol == 29 && cand[7].extra_bits == 13 && cand[7].extra == 32768 - 24577 &&
             cand[8].d == 0, "a candidate over 32768 is dropped", "");
  png_candidates(2, 1, cand);
  expect(cand[6].d == 1 && cand[7].d == 2 && cand[8].d == 3, "the smallest stride", "");

  refused(0, 8, 8, 3, 5, 1, -1, "at least one image, got N = 0");
  refused(-1, 8, 8, 3, 5, 1, -1, "at least one image");
  refused(1, 0, 8, 3, 5, 1, -1, "has a zero side");
  refused(1, 8, 0, 3, 5, 1, -1, "has a zero side");
  refused(1, 8, 8, 0, 5, 1, -1, "1 .. 4 channels, got 0");
  refused(1, 8, 8, 5, 5, 1, -1, "1 .. 4 channels, got 5");
  refused(1, 8, 8, 3, 6, 1, -1, "unknown filter mode 6");
  refused(1, 8, 8, 3, -1, 1, -1, "unknown filter mode -1");
  refused(1, 8, 8, 3, 5, 0, -1, "at least one row, got rows_per_segment = 0");
  refused(1, 8, 8, 3, 5, -4, -1, "at least one row");
  refused(1, 2, 65535, 1, 5, 1, -2, "a row of 65536 bytes");
  refused(1, 2, 16384, 4, 5, 1, -2, "a row of 65537 bytes");
  refused(1, 4, 30000, 1, 5, 3, -2, "a segment of 3 rows is 90003 bytes");
  refused(1, (1 << 24) + 1, 8, 3, 5, 1, -2, "at most 16777216 rows");
  refused(65536, 8, 8, 3, 5, 1, -2, "at most 65535 images");

  if (failures) return 1;
  printf("png plan ok: 2 heads, 2 table headers, %d refusals\n", refusals);
  return 0;
}
