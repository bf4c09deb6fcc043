// AddressSanitizer / UBSan check of the host-only C++ of the material selection kernel: the packing and validation of a selection
// program (csrc/material_edit_plan.h), fed the maximal program, a handful of ordinary ones and every refused one.  Built and run by
// tests/test_material_edit_native.py:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Ivqnerf_release_amd/csrc tests/native/material_edit_host.cpp
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "material_edit_plan.h"

struct Term { int plane, ch, den, cond; float lo, hi; };

static int pack(const std::vector<int32_t>& plane_ch, const std::vector<uint8_t>& present, const std::vector<Term>& terms, const std::vector<int32_t>& ops,
                int n_conds, const uint8_t* codes, MatEditProgram* out, char* msg, size_t len) {
  // exact-size heap copies: a read one element past any of them is an ASan report
  std::vector<int32_t> ti;
  std::vector<float> tf;
  for (const Term& t : terms) {
    ti.insert(ti.end(), {t.plane, t.ch, t.den, t.cond});
    tf.insert(tf.end(), {t.lo, t.hi});
  }
  return matedit_pack(plane_ch.data(), present.data(), ti.empty() ? nullptr : ti.data(), tf.empty() ? nullptr : tf.data(), (int)terms.size(),
                      ops.empty() ? nullptr : ops.data(), n_conds, codes, 5e-6f, out, msg, len);
}

static int failures = 0;
static void expect(bool ok, const char* what, const char* msg) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s (%s)\n", what, msg);
    ++failures;
  }
}

int main() {
  const std::vector<int32_t> plane_ch = {3, 3, 3, 3, 1, 0, 0, 0};
  const std::vector<uint8_t> present = {1, 1, 1, 1, 1, 0, 0, 0};
  MatEditProgram prog;
  char msg[256] = "";
  // the maximal program: 8 conditions, 32 terms (mat, mat, mat, rgb, xyz, rgb_scale, spec_scale, rough), given in an order that is NOT by plane
  std::vector<Term> terms;
  for (int k = 0; k < 3; ++k) {
    for (int c = 0; c < 3; ++c) terms.push_back({2, c, -1, k, 0.1f * k, 0.9f});
    for (int c = 0; c < 3; ++c) terms.push_back({3, c, -1, k, 0.2f, 1.f});
    terms.push_back({4, 0, -1, k, 0.f, 1.f});
  }
  for (int c = 0; c < 3; ++c) terms.push_back({0, c, -1, 3, 0.2f, 1.f});
  for (int c = 0; c < 3; ++c) terms.push_back({1, c, -1, 4, -1.f, 1.f});
  for (int c = 0; c < 2; ++c) terms.push_back({0, c, 2, 5, 0.5f, 2.f});
  for (int c = 0; c < 2; ++c) terms.push_back({3, c, 2, 6, 0.5f, 2.f});
  terms.push_back({4, 0, -1, 7, 0.3f, 0.8f});
  const std::vector<int32_t> ops = {1, 1, 0, 1, 0, 1, 0};
  uint8_t codes[kMatCodes] = {0};
  codes[1] = codes[63] = codes[64] = 1;
  int rc = pack(plane_ch, present, terms, ops, 8, codes, &prog, msg, sizeof(msg));
  expect(rc == 0 && terms.size() == 32, "the maximal program packs", msg);
  expect(prog.n_terms == 32 && prog.n_conds == 8 && prog.or_bits == 0x2bu, "counts and ops", msg);
  expect(prog.begin[0] == 0 && prog.begin[1] == 5 && prog.begin[2] == 8 && prog.begin[3] == 17 && prog.begin[4] == 28 && prog.begin[5] == 32 &&
             prog.begin[8] == 32, "terms sorted by plane", msg);
  expect(prog.codes_lo == ((1ull << 1) | (1ull << 63)) && prog.code64 == 1 && prog.has_codes == 1, "the code set", msg);
  int dens = 0;
  for (int p = 0; p < kMatPlanes; ++p) {
    expect(prog.plane_word[p] == ((uint32_t)prog.begin[p] | (uint32_t)prog.begin[p + 1] << 8 | (uint32_t)prog.plane_ch[p] << 16), "plane word", msg);
    for (int t = prog.begin[p]; t < prog.begin[p + 1]; ++t) {
      expect(prog.ch[t] < prog.plane_ch[p] && (prog.den[t] == kMatNoDen || prog.den[t] < prog.plane_ch[p]) && prog.cond[t] < 8, "a packed term", msg);
      dens += prog.den[t] != kMatNoDen;
    }
  }
  expect(dens == 4, "the denominators survive the sort", msg);
  // ordinary ones: codes alone, one condition, no codes
  expect(pack(plane_ch, present, {}, {}, 0, codes, &prog, msg, sizeof(msg)) == 0 && prog.n_terms == 0 && prog.has_codes == 1, "codes alone", msg);
  expect(pack(plane_ch, present, {{4, 0, -1, 0, 0.f, 1.f}}, {}, 1, nullptr, &prog, msg, sizeof(msg)) == 0 && prog.has_codes == 0 && prog.begin[5] == 1,
         "one condition", msg);
  expect(pack(plane_ch, present, {}, {}, 0, nullptr, &prog, msg, sizeof(msg)) == 0, "the empty program (mask_in alone selects)", msg);
  // the refused ones, each with its reason
  struct Bad { std::vector<Term> terms; std::vector<int32_t> ops; int n_conds, rc; const char* why; };
  std::vector<Term> nine, many(33, Term{4, 0, -1, 0, 0.f, 1.f});
  for (int k = 0; k < 9; ++k) nine.push_back({4, 0, -1, k, 0.f, 1.f});
  const std::vector<Bad> bad = {
      {nine, std::vector<int32_t>(8, 0), 9, -2, "at most 8 conditions, got 9"},
      {many, {}, 1, -2, "at most 32 terms, got 33"},
      {{{5, 0, -1, 0, 0.f, 1.f}}, {}, 1, -1, "names plane 5, which is null"},
      {{{8, 0, -1, 0, 0.f, 1.f}}, {}, 1, -1, "names plane 8, planes are 0 .. 7"},
      {{{-1, 0, -1, 0, 0.f, 1.f}}, {}, 1, -1, "names plane -1"},
      {{{4, 1, -1, 0, 0.f, 1.f}}, {}, 1, -1, "channel 1 / denominator -1 out of range"},
      {{{0, 0, 3, 0, 0.f, 1.f}}, {}, 1, -1, "channel 0 / denominator 3 out of range"},
      {{{0, -1, -1, 0, 0.f, 1.f}}, {}, 1, -1, "channel -1"},
      {{{0, 0, -2, 0, 0.f, 1.f}}, {}, 1, -1, "denominator -2"},
      {{{4, 0, -1, 1, 0.f, 1.f}}, {0}, 2, -1, "a condition without a term"},
      {{{4, 0, -1, 2, 0.f, 1.f}}, {}, 1, -1, "belongs to condition 2 of 1"},
      {{{4, 0, -1, 0, 0.f, 1.f}, {4, 0, -1, 1, 0.f, 1.f}}, {2}, 2, -1, "op 0 is 2"},
      {{}, {}, 1, -1, "1 conditions with 0 terms"},
      {{{4, 0, -1, 0, 0.f, 1.f}}, {}, 0, -1, "0 conditions with 1 terms"},
      {{}, {}, -1, -2, "at most 8 conditions, got -1"},
  };
  for (const Bad& b : bad) {
    msg[0] = 0;
    rc = pack(plane_ch, present, b.terms, b.ops, b.n_conds, nullptr, &prog, msg, sizeof(msg));
    expect(rc == b.rc && strstr(msg, b.why) != nullptr, b.why, msg);
  }
  // a plane of too many channels, and a message buffer that is too short for its message
  rc = pack({4, 3, 3, 3, 1, 0, 0, 0}, present, {{0, 0, -1, 0, 0.f, 1.f}}, {}, 1, nullptr, &prog, msg, sizeof(msg));
  expect(rc == -2 && strstr(msg, "plane 0 has 4 channels") != nullptr, "a plane of 4 channels", msg);
  char tiny[8];
  rc = pack(plane_ch, present, nine, std::vector<int32_t>(8, 0), 9, nullptr, &prog, tiny, sizeof(tiny));
  expect(rc == -2 && strlen(tiny) == sizeof(tiny) - 1, "a short message buffer is not overrun", tiny);
  if (failures) return 1;
  printf("material edit plan ok: the maximal program, %d refusals\n", (int)bad.size() + 1);
  return 0;
}
