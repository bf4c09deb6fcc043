// The descriptor rules of the Dense-stack kernels (csrc/chain_launch.h: chain_check_desc), as a stand-alone program under ASan / UBSan.
// Built and run by tests/test_chain_check_native.py:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ivqnerf_release_amd/csrc
//       tests/native/chain_check_host.cpp vqnerf_release_amd/csrc/neus_pack_plan.cpp vqnerf_release_amd/csrc/chain_pack_plan.cpp
//       vqnerf_release_amd/csrc/error.cpp
// 1. the shipped programs, built by the C planner (vqn_chain_pack_plan), are accepted under the f32 rules;
// 2. every rule number 1-6 and 10-22: one field of a valid program broken, that number under each engine's rules;
// 3. the two differences between the engines, one by one;
// 4. descriptors given on the command line as `f32:FILE` / `f16s:FILE` (272 int32 each: the Python packer's) are accepted under
//    that engine's rules.
#include <stdio.h>
#include <string.h>

#include <functional>

#include "chain_launch.h"
#include "vqnerf_hip.h"

static int n_accepted = 0, n_refused = 0;

static bool accept(const char* what, const ChainDesc& d, const ChainEngineRules& r) {
  const int c = chain_check_desc(d, r);
  if (c != 0) {
    fprintf(stderr, "FAIL: %s: check %d, wanted a valid program\n", what, c);
    return false;
  }
  ++n_accepted;
  return true;
}

// A small program both engines take: GEMM layer (rows 0..2 -> tile at rows 4..8, slot 0), the input again at rows 8..10, a two-output
// layer over rows 4..8 and 8..10 (slot 1).
static ChainDesc base_program() {
  ChainDesc d;
  memset(&d, 0, sizeof(d));
  d.n_layers = 3; d.in_mode = 0; d.in_feats = 16; d.in_rows = 2; d.in_row0 = 0; d.total_rows = 16; d.n_waves = 4; d.in_stride = 16;
  d.small_w4 = 2 * 6 * 2;
  ChainLayer& g = d.layers[0];
  g.kind = 0; g.act = 1; g.n_out_tiles = 1; g.kA_row0 = 0; g.kA_rows = 2; g.dst_row0 = 4; g.out_slot = 0; g.out_feats = 32;
  ChainLayer& in2 = d.layers[1];
  in2.kind = 2; in2.dst_row0 = 8; in2.out_slot = -1;
  ChainLayer& s = d.layers[2];
  s.kind = 1; s.act = 3; s.n_out_tiles = 2; s.kA_row0 = 4; s.kA_rows = 4; s.kB_row0 = 8; s.kB_rows = 2; s.dst_row0 = 0; s.out_slot = 1;
  return d;
}

// the base program with `breakit` applied: `f32` / `f16s` are the codes wanted under the two engines' rules
static bool expect(const char* what, const std::function<void(ChainDesc&)>& breakit, const int f32, const int f16s) {
  ChainDesc d = base_program();
  breakit(d);
  const int a = chain_check_desc(d, kChainRulesF32), b = chain_check_desc(d, kChainRulesF16s);
  if (a != f32 || b != f16s) {
    fprintf(stderr, "FAIL: %s: check %d under the f32 rules (wanted %d), %d under the f16s rules (wanted %d)\n", what, a, f32, b, f16s);
    return false;
  }
  n_refused += (f32 != 0) + (f16s != 0);
  n_accepted += (f32 == 0) + (f16s == 0);
  return true;
}

static bool planned(const char* what, const int in_mode, const int in_feats, const int n_freqs, const int n_stacks, const vqn_chain_stack* st) {
  int32_t words[sizeof(ChainDesc) / 4];
  if (vqn_chain_pack_plan(in_mode, in_feats, n_freqs, n_stacks, st, words, nullptr, 0) <= 0) {
    fprintf(stderr, "FAIL: %s: the planner refused it (%s)\n", what, vqn_last_error());
    return false;
  }
  ChainDesc d;
  memcpy(&d, words, sizeof(d));
  return accept(what, d, kChainRulesF32);
}

int main(int argc, char** argv) {
  static_assert(sizeof(ChainDesc) == 272 * 4, "descriptor layout");
  bool ok = true;

  // ---- 1. the shipped networks (vq_nfr.ini: mlp_width 128, z_dim 256, 10 frequencies), planned in C
  vqn_chain_stack enc[5] = {};
  enc[0] = {0, 4, {128, 128, 128, 128}, {1, 1, 1, 1}, 2, -1, -1};
  enc[1] = {0, 3, {128, 256, 256}, {0, 1, 3}, -1, 0, 0};
  const int main_out[3] = {3, 1, 1}, vq_out[3] = {3, 3, 1};
  for (int h = 0; h < 3; ++h) enc[2 + h] = {1, 3, {256, 128, main_out[h]}, {1, 1, 3}, 1, 1, h + 1};
  vqn_chain_stack heads_main[3], heads_vq[3];
  for (int h = 0; h < 3; ++h) {
    heads_main[h] = {1, 3, {256, 128, main_out[h]}, {1, 1, 3}, 1, -1, h};
    heads_vq[h] = {1, 3, {256, 128, vq_out[h]}, {1, 1, 3}, 1, -1, h};
  }
  ok &= planned("encoder", 1, 63, 10, 2, enc);
  ok &= planned("encoder + main heads", 1, 63, 10, 5, enc);
  ok &= planned("main heads", 0, 256, 0, 3, heads_main);
  ok &= planned("vq heads", 0, 256, 0, 3, heads_vq);

  // ---- 2. one broken field per rule
  ok &= accept("base program, f32 rules", base_program(), kChainRulesF32);
  ok &= accept("base program, f16s rules", base_program(), kChainRulesF16s);
  ok &= expect("no layers", [](ChainDesc& d) { d.n_layers = 0; }, 1, 1);
  ok &= expect("17 layers", [](ChainDesc& d) { d.n_layers = VQN_CHAIN_MAX_LAYERS + 1; }, 1, 1);
  ok &= expect("6 waves", [](ChainDesc& d) { d.n_waves = 6; }, 2, 2);
  ok &= expect("no rows", [](ChainDesc& d) { d.total_rows = 0; }, 3, 3);
  ok &= expect("negative small_w4", [](ChainDesc& d) { d.small_w4 = -1; }, 3, 3);
  ok &= expect("more LDS than a CU has", [](ChainDesc& d) { d.total_rows = 160; }, 3, 3);
  ok &= expect("no input rows", [](ChainDesc& d) { d.in_rows = 0; }, 4, 4);
  ok &= expect("input before row 0", [](ChainDesc& d) { d.in_row0 = -1; }, 4, 4);
  ok &= expect("input past the last row", [](ChainDesc& d) { d.in_row0 = 15; }, 4, 4);
  ok &= expect("posenc width", [](ChainDesc& d) { d.in_mode = 1; d.n_freqs = 2; }, 5, 5);
  ok &= expect("17 frequencies", [](ChainDesc& d) { d.in_mode = 1; d.n_freqs = 17; d.in_feats = 105; }, 5, 5);
  ok &= expect("no input features", [](ChainDesc& d) { d.in_feats = 0; }, 6, 6);
  ok &= expect("more features than rows hold", [](ChainDesc& d) { d.in_feats = 17; }, 6, 6);
  ok &= expect("input stride 0", [](ChainDesc& d) { d.in_stride = 0; }, 6, 6);
  ok &= expect("negative K rows", [](ChainDesc& d) { d.layers[0].kA_rows = -1; }, 10, 10);
  ok &= expect("no K rows", [](ChainDesc& d) { d.layers[0].kA_rows = 0; }, 10, 10);
  ok &= expect("segment A before row 0", [](ChainDesc& d) { d.layers[0].kA_row0 = -1; }, 11, 11);
  ok &= expect("segment A past the last row", [](ChainDesc& d) { d.layers[0].kA_row0 = 15; }, 11, 11);
  ok &= expect("segment B before row 0", [](ChainDesc& d) { d.layers[2].kB_row0 = -1; }, 12, 12);
  ok &= expect("segment B past the last row", [](ChainDesc& d) { d.layers[2].kB_row0 = 15; }, 12, 12);
  ok &= expect("output slot 4", [](ChainDesc& d) { d.layers[0].out_slot = VQN_CHAIN_MAX_OUTS; }, 13, 13);
  ok &= expect("no output tiles", [](ChainDesc& d) { d.layers[0].n_out_tiles = 0; }, 14, 14);
  ok &= expect("output before row 0", [](ChainDesc& d) { d.layers[0].dst_row0 = -1; }, 14, 14);
  ok &= expect("output past the last row", [](ChainDesc& d) { d.layers[0].dst_row0 = 14; }, 14, 14);
  ok &= expect("no output features", [](ChainDesc& d) { d.layers[0].out_feats = 0; }, 15, 15);
  ok &= expect("more output features than tiles", [](ChainDesc& d) { d.layers[0].out_feats = 33; }, 15, 15);
  ok &= expect("output over segment A", [](ChainDesc& d) { d.layers[0].dst_row0 = 0; }, 16, 16);
  ok &= expect("output over segment B", [](ChainDesc& d) { d.layers[0].kB_row0 = 6; d.layers[0].kB_rows = 2; }, 17, 17);
  ok &= expect("small layer without outputs", [](ChainDesc& d) { d.layers[2].n_out_tiles = 0; }, 18, 18);
  ok &= expect("small layer with 5 outputs", [](ChainDesc& d) { d.layers[2].n_out_tiles = 5; }, 18, 18);
  ok &= expect("small layer without a slot", [](ChainDesc& d) { d.layers[2].out_slot = -1; }, 18, 18);
  ok &= expect("layer kind 3", [](ChainDesc& d) { d.layers[0].kind = 3; }, 19, 19);
  ok &= expect("input reloaded before row 0", [](ChainDesc& d) { d.layers[1].dst_row0 = -1; }, 20, 20);
  ok &= expect("input reloaded past the last row", [](ChainDesc& d) { d.layers[1].dst_row0 = 15; }, 20, 20);
  ok &= expect("weight image before the region", [](ChainDesc& d) { d.layers[2].dst_row0 = -1; }, 21, 21);
  ok &= expect("weight image past the region", [](ChainDesc& d) { d.layers[2].dst_row0 = 1; }, 21, 21);

  // ---- 3. what the engines differ in: whole K steps of two rows, and layers written in place (bit 8 of act)
  ok &= expect("odd kA_rows", [](ChainDesc& d) { d.layers[0].kA_rows = 3; }, 0, 10);
  ok &= expect("odd kB_rows", [](ChainDesc& d) { d.layers[2].kB_rows = 1; d.small_w4 = 2 * 5 * 2; }, 0, 10);
  ok &= expect("odd in_rows", [](ChainDesc& d) { d.in_rows = 3; }, 0, 4);
  ok &= expect("in place over segment A", [](ChainDesc& d) { d.layers[0].act |= 0x100; d.layers[0].dst_row0 = 0; }, 0, 16);
  ok &= expect("in place over segment B",
               [](ChainDesc& d) { d.layers[0].act |= 0x100; d.layers[0].kB_row0 = 6; d.layers[0].kB_rows = 2; }, 0, 17);
  const auto five_tiles_in_place = [](ChainDesc& d) {
    d.total_rows = 32;
    d.layers[0].act |= 0x100; d.layers[0].dst_row0 = 0; d.layers[0].n_out_tiles = 5;
  };
  ok &= expect("in place, 5 tiles on 4 waves", five_tiles_in_place, 22, 16);
  ok &= expect("in place, 5 tiles on 8 waves", [&](ChainDesc& d) { five_tiles_in_place(d); d.n_waves = 8; }, 0, 16);

  // ---- 4. the Python packer's descriptors
  for (int i = 1; i < argc; ++i) {
    const bool f16s = strncmp(argv[i], "f16s:", 5) == 0;
    if (!f16s && strncmp(argv[i], "f32:", 4) != 0) {
      fprintf(stderr, "FAIL: argument %s: f32:FILE or f16s:FILE\n", argv[i]);
      return 1;
    }
    const char* path = argv[i] + (f16s ? 5 : 4);
    FILE* f = fopen(path, "rb");
    ChainDesc d;
    const size_t n = f ? fread(&d, 1, sizeof(d), f) : 0;
    const bool at_end = f && fgetc(f) == EOF;
    if (f) fclose(f);
    if (n != sizeof(d) || !at_end) {
      fprintf(stderr, "FAIL: %s: not a file of 272 int32\n", path);
      return 1;
    }
    ok &= accept(argv[i], d, f16s ? kChainRulesF16s : kChainRulesF32);
  }
  if (!ok) return 1;
  printf("chain descriptor rules ok: %d descriptors accepted, %d refusals checked\n", n_accepted, n_refused);
  return 0;
}
