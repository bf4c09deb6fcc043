// Host side of the device JPEG encoder (csrc/jpeg_encode.hip): the quantisation tables of a quality, the Huffman code tables from
// BITS / HUFFVAL, the geometry of a batch (MCU counts, restart intervals, slot and buffer sizes) and the header bytes of a file, with
// every refusal.  Plain C++, no HIP: tests/native/jpeg_plan_host.cpp builds it into a stand-alone program under ASan / UBSan.
//
// Baseline sequential JPEG (SOF0), 8 bit, three components Y Cb Cr, JFIF; '420' (MCU 16x16: Y00 Y01 Y10 Y11 Cb Cr) or '444' (MCU 8x8:
// Y Cb Cr); the Annex K tables; a restart interval of Ri MCUs, always.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vqn_image_codec.h"  // (by path: the stand-alone build of this header names no include directory)
#include "codec_plan.h"

constexpr int kJpegMaxSide = 65535;
constexpr int kJpegBlockBits = 64 * 26;                  // the most a block codes to: 64 coefficients of a 16-bit code + 10 bits
constexpr int kJpegBlockBytes = kJpegBlockBits / 8 * 2;  // ... in bytes, doubled: every byte may be an FF that is stuffed
constexpr int kJpegHeaderCap = VQN_JPEG_HEADER_CAP;      // bytes a header never reaches (it has 629)

// zigzag position -> natural index (row * 8 + column)
static const uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 / K.2, natural order
static const uint8_t kJpegLumaBase[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                          69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                          81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72,  92,  95,  98,  112, 100, 103, 99};
static const uint8_t kJpegChromaBase[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                            99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                            99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3 - K.6: BITS (codes of length 1 .. 16) and HUFFVAL
static const uint8_t kJpegDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kJpegDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kJpegDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kJpegAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t kJpegAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
static const uint8_t kJpegAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t kJpegAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// What the entropy kernel reads: a code and its length as len << 16 | code, 0 for a symbol without a code.  Class 0 luma, 1 chroma.
struct JpegHuff {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};

// The geometry of a batch is the public struct VqnJpegGeom (include/vqn_image_codec.h): vqn_jpeg_plan hands its words to the caller
// as they lie.
using JpegGeom = VqnJpegGeom;
constexpr int kJpegGeomWords = sizeof(JpegGeom) / sizeof(int64_t);

// IJG scaling of a base table: s = 5000 / q below 50, else 200 - 2 q; entry clamp((base s + 50) / 100, 1, 255).  Natural order.
inline void jpeg_quant_table(const uint8_t* base, int quality, uint16_t* out) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    int v = (base[i] * s + 50) / 100;
    out[i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
  }
}

// Annex C: the codes of a table in the order of HUFFVAL -> table[symbol] = len << 16 | code.
inline void jpeg_huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* table, int table_len) {
  for (int i = 0; i < table_len; ++i) table[i] = 0u;
  uint32_t code = 0u;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i, ++k) table[vals[k]] = (uint32_t)len << 16 | code++;
    code <<= 1;
  }
}

inline void jpeg_huff_tables(JpegHuff* h) {
  jpeg_huff_codes(kJpegDcLumaBits, kJpegDcVals, h->dc[0], 12);
  jpeg_huff_codes(kJpegDcChromaBits, kJpegDcVals, h->dc[1], 12);
  jpeg_huff_codes(kJpegAcLumaBits, kJpegAcLumaVals, h->ac[0], 256);
  jpeg_huff_codes(kJpegAcChromaBits, kJpegAcChromaVals, h->ac[1], 256);
}

// -> 0, or -1 (bad argument) / -2 (unsupported shape) with the reason in msg.  sub: 420 or 444.
inline int jpeg_plan(int64_t n, int64_t h, int64_t w, int quality, int sub, int64_t ri, JpegGeom* g, char* msg, size_t msg_len) {
  memset(g, 0, sizeof(*g));
  if (n < 1) {
    snprintf(msg, msg_len, "bad argument: a batch has at least one frame, got N = %lld", (long long)n);
    return -1;
  }
  if (h < 1 || w < 1) {
    snprintf(msg, msg_len, "bad argument: a frame of %lld x %lld pixels has a zero side", (long long)h, (long long)w);
    return -1;
  }
  if (h > kJpegMaxSide || w > kJpegMaxSide) {
    snprintf(msg, msg_len, "unsupported shape: a JPEG side is at most %d pixels, got %lld x %lld", kJpegMaxSide, (long long)h, (long long)w);
    return -2;
  }
  if (quality < 1 || quality > 100) {
    snprintf(msg, msg_len, "bad argument: quality is 1 .. 100, got %d", quality);
    return -1;
  }
  if (sub != 420 && sub != 444) {
    snprintf(msg, msg_len, "bad argument: unknown subsampling %d, '420' and '444' are supported", sub);
    return -1;
  }
  if (ri < 1 || ri > 65535) {
    snprintf(msg, msg_len, "bad argument: the restart interval is 1 .. 65535 MCUs, got %lld", (long long)ri);
    return -1;
  }
  g->n = n, g->h = h, g->w = w, g->quality = quality, g->sub = sub, g->ri = ri;
  g->mcu = sub == 420 ? 16 : 8;
  g->blocks_per_mcu = sub == 420 ? 6 : 3;
  g->mcus_x = (w + g->mcu - 1) / g->mcu, g->mcus_y = (h + g->mcu - 1) / g->mcu;
  const int64_t mcus = g->mcus_x * g->mcus_y;
  g->intervals = (mcus + ri - 1) / ri;
  const int64_t per_slot = ri < mcus ? ri : mcus;        // MCUs an interval holds at most
  g->slot_bytes = (per_slot * g->blocks_per_mcu * kJpegBlockBytes + 2 + 15) / 16 * 16;      // + the padded last byte, stuffed
  g->by_c = g->mcus_y, g->bx_c = g->mcus_x;
  g->by_y = sub == 420 ? 2 * g->mcus_y : g->mcus_y, g->bx_y = sub == 420 ? 2 * g->mcus_x : g->mcus_x;
  const int64_t y_bytes = n * g->by_y * g->bx_y * 128, c_bytes = n * g->by_c * g->bx_c * 128;   // 64 int16 per block
  g->off_cb = y_bytes, g->off_cr = y_bytes + c_bytes, g->off_slots = y_bytes + 2 * c_bytes;
  g->off_lens = g->off_slots + n * g->intervals * g->slot_bytes;
  g->off_dst = g->off_lens + (n * g->intervals * 4 + 15) / 16 * 16;
  g->scratch_bytes = g->off_dst + n * g->intervals * 8;
  g->out_bytes = n * g->intervals * (g->slot_bytes + 2);                                    // + an RST marker per interval
  return 0;
}

// codec_check_buffers for this plan.  coefficients_only: the first kernel alone runs, which needs the coefficient planes and no output.
inline int jpeg_check_buffers(const JpegGeom& g, int64_t scratch_bytes, int64_t out_bytes, int coefficients_only, char* msg, size_t msg_len) {
  return codec_check_buffers(g.off_slots, g.scratch_bytes, g.out_bytes, scratch_bytes, out_bytes, coefficients_only, msg, msg_len);
}

// The header of a file: SOI, APP0 (JFIF 1.01, no density), DQT x 2, SOF0, DHT x 4, DRI, SOS -> its length, or -1 when cap is too small.
inline int jpeg_header(const JpegGeom& g, uint8_t* out, int cap) {
  uint8_t b[kJpegHeaderCap];
  int n = 0;
  auto put = [&](int v) { b[n++] = (uint8_t)v; };
  auto put16 = [&](int v) { put(v >> 8), put(v & 255); };
  put16(0xffd8);
  put16(0xffe0), put16(16);
  for (const char c : {'J', 'F', 'I', 'F', '\0'}) put(c);
  put16(0x0101), put(0), put16(1), put16(1), put(0), put(0);
  for (int t = 0; t < 2; ++t) {
    uint16_t q[64];
    jpeg_quant_table(t ? kJpegChromaBase : kJpegLumaBase, (int)g.quality, q);
    put16(0xffdb), put16(67), put(t);
    for (int k = 0; k < 64; ++k) put(q[kJpegZigzag[k]]);
  }
  put16(0xffc0), put16(17), put(8), put16((int)g.h), put16((int)g.w), put(3);
  put(1), put(g.sub == 420 ? 0x22 : 0x11), put(0);
  put(2), put(0x11), put(1);
  put(3), put(0x11), put(1);
  const uint8_t* bits[4] = {kJpegDcLumaBits, kJpegAcLumaBits, kJpegDcChromaBits, kJpegAcChromaBits};
  const uint8_t* vals[4] = {kJpegDcVals, kJpegAcLumaVals, kJpegDcVals, kJpegAcChromaVals};
  const int ids[4] = {0x00, 0x10, 0x01, 0x11}, counts[4] = {12, 162, 12, 162};
  for (int t = 0; t < 4; ++t) {
    put16(0xffc4), put16(19 + counts[t]), put(ids[t]);
    for (int i = 0; i < 16; ++i) put(bits[t][i]);
    for (int i = 0; i < counts[t]; ++i) put(vals[t][i]);
  }
  put16(0xffdd), put16(4), put16((int)g.ri);
  put16(0xffda), put16(12), put(3), put(1), put(0x00), put(2), put(0x11), put(3), put(0x11), put(0), put(63), put(0);
  if (n > cap) return -1;
  memcpy(out, b, (size_t)n);
  return n;
}
