// Host side of the material selection kernel (csrc/material_edit.hip): the selection program as the caller states it -> the packed
// form the kernel reads from its arguments, with every refusal.  Plain C++, no HIP: tests/native/material_edit_host.cpp builds it
// into a stand-alone program under ASan / UBSan.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vqn_material_edit.h"  // (by path: the stand-alone build of this header names no include directory)

constexpr int kMatPlanes = VQN_MATEDIT_MAX_PLANES;   // property planes at most
constexpr int kMatMaxCh = VQN_MATEDIT_MAX_CHANNELS;  // channels of a plane at most
constexpr int kMatTerms = VQN_MATEDIT_MAX_TERMS;     // terms of a program at most
constexpr int kMatConds = VQN_MATEDIT_MAX_CONDS;     // conditions of a program at most
constexpr int kMatCodes = VQN_MATEDIT_CODES;         // code labels 0 .. 64
constexpr int kMatNoDen = 255;       // MatEditProgram::den of a term without a denominator

// A term is one channel test lo < v < hi (both strict) of v = plane[ch], or v = plane[ch] / (plane[den] + eps); a condition holds when
// all of its terms hold.  Terms are sorted by plane: plane p owns the terms begin[p] .. begin[p + 1] - 1.
struct MatEditProgram {
  float lo[kMatTerms], hi[kMatTerms];
  uint8_t ch[kMatTerms], den[kMatTerms], cond[kMatTerms];
  uint8_t begin[kMatPlanes + 1];
  uint8_t plane_ch[kMatPlanes];
  uint32_t plane_word[kMatPlanes];   // begin[p] | begin[p + 1] << 8 | plane_ch[p] << 16: what the kernel reads per plane
  uint32_t or_bits;                  // bit i: the op between condition i and condition i + 1 is 'or' (else 'and')
  int32_t n_conds, n_terms;
  uint64_t codes_lo;                 // bit c: code c is in the set, c = 0 .. 63
  uint32_t code64;                   // code 64 is in the set
  int32_t has_codes;
  float eps;
};

// plane_ch [8]: the channel count of each plane (read only where plane_present[p] != 0); terms_i [n_terms][4] = plane, channel,
// denominator channel or -1, condition id; terms_f [n_terms][2] = lo, hi; ops [n_conds - 1]: 0 'and', 1 'or'; codes [65] flags or NULL.
// -> 0, or -1 (bad argument) / -2 (unsupported shape) with the reason in msg.
inline int matedit_pack(const int32_t* plane_ch, const uint8_t* plane_present, const int32_t* terms_i, const float* terms_f, int n_terms,
                        const int32_t* ops, int n_conds, const uint8_t* codes, float eps, MatEditProgram* out, char* msg, size_t msg_len) {
  memset(out, 0, sizeof(*out));
  if (n_conds < 0 || n_conds > kMatConds) {
    snprintf(msg, msg_len, "unsupported shape: a program has at most %d conditions, got %d", kMatConds, n_conds);
    return -2;
  }
  if (n_terms < 0 || n_terms > kMatTerms) {
    snprintf(msg, msg_len, "unsupported shape: a program has at most %d terms, got %d", kMatTerms, n_terms);
    return -2;
  }
  if ((n_terms > 0 && (!terms_i || !terms_f || !plane_ch || !plane_present)) || (n_conds > 1 && !ops)) {
    snprintf(msg, msg_len, "bad argument: null program array");
    return -1;
  }
  if ((n_conds == 0) != (n_terms == 0)) {
    snprintf(msg, msg_len, "bad argument: %d conditions with %d terms", n_conds, n_terms);
    return -1;
  }
  unsigned seen = 0u;
  int per_plane[kMatPlanes] = {0};
  for (int t = 0; t < n_terms; ++t) {
    const int p = terms_i[4 * t], c = terms_i[4 * t + 1], d = terms_i[4 * t + 2], k = terms_i[4 * t + 3];
    if (p < 0 || p >= kMatPlanes) {
      snprintf(msg, msg_len, "bad argument: term %d names plane %d, planes are 0 .. %d", t, p, kMatPlanes - 1);
      return -1;
    }
    if (!plane_present[p]) {
      snprintf(msg, msg_len, "bad argument: term %d names plane %d, which is null", t, p);
      return -1;
    }
    if (plane_ch[p] < 1 || plane_ch[p] > kMatMaxCh) {
      snprintf(msg, msg_len, "unsupported shape: plane %d has %d channels, 1 .. %d are supported", p, plane_ch[p], kMatMaxCh);
      return -2;
    }
    if (c < 0 || c >= plane_ch[p] || d < -1 || d >= plane_ch[p]) {
      snprintf(msg, msg_len, "bad argument: term %d: channel %d / denominator %d out of range for plane %d of %d channels", t, c, d, p, plane_ch[p]);
      return -1;
    }
    if (k < 0 || k >= n_conds) {
      snprintf(msg, msg_len, "bad argument: term %d belongs to condition %d of %d", t, k, n_conds);
      return -1;
    }
    seen |= 1u << k;
    ++per_plane[p];
  }
  if (seen != (n_conds ? (1u << n_conds) - 1u : 0u)) {
    snprintf(msg, msg_len, "bad argument: a condition without a term");
    return -1;
  }
  int at[kMatPlanes];
  for (int p = 0, s = 0; p < kMatPlanes; ++p) {
    out->begin[p] = (uint8_t)s, at[p] = s;
    s += per_plane[p];
    out->begin[p + 1] = (uint8_t)s;
    out->plane_ch[p] = plane_present && plane_present[p] && plane_ch && plane_ch[p] >= 1 && plane_ch[p] <= kMatMaxCh ? (uint8_t)plane_ch[p] : 0;
  }
  for (int p = 0; p < kMatPlanes; ++p) out->plane_word[p] = (uint32_t)out->begin[p] | (uint32_t)out->begin[p + 1] << 8 | (uint32_t)out->plane_ch[p] << 16;
  for (int t = 0; t < n_terms; ++t) {                            // stable counting sort by plane
    const int s = at[terms_i[4 * t]]++;
    out->lo[s] = terms_f[2 * t], out->hi[s] = terms_f[2 * t + 1];
    out->ch[s] = (uint8_t)terms_i[4 * t + 1];
    out->den[s] = terms_i[4 * t + 2] < 0 ? (uint8_t)kMatNoDen : (uint8_t)terms_i[4 * t + 2];
    out->cond[s] = (uint8_t)terms_i[4 * t + 3];
  }
  for (int i = 0; i + 1 < n_conds; ++i) {
    if (ops[i] != 0 && ops[i] != 1) {
      snprintf(msg, msg_len, "bad argument: op %d is %d, 0 ('and') or 1 ('or') expected", i, ops[i]);
      return -1;
    }
    out->or_bits |= (uint32_t)ops[i] << i;
  }
  out->n_conds = n_conds, out->n_terms = n_terms, out->eps = eps;
  if (codes) {
    out->has_codes = 1;
    for (int c = 0; c < 64; ++c) out->codes_lo |= (uint64_t)(codes[c] != 0) << c;
    out->code64 = codes[64] != 0;
  }
  return 0;
}
