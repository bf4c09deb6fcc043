// Host side of the mesh-material kernels (csrc/mesh_materials.hip): the sizes as the caller states them -> the limits, the bitmap
// geometry, the face blocks and the scratch layout of the label clean-up, with every refusal.  Plain C++, no HIP:
// tests/native/mesh_materials_host.cpp builds it into a stand-alone program under ASan / UBSan.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vqn_mesh_materials.h"  // (by path: the stand-alone build of this header names no include directory)

constexpr int kMeshMatMaxCodes = VQN_MESHMAT_MAX_CODES;
constexpr int kMeshMatFacesPerBlock = VQN_MESHMAT_FACES_PER_BLOCK;
constexpr int kMeshMatWordBits = VQN_MESHMAT_WORD_BITS;
constexpr int64_t kMeshMatIndexLimit = (int64_t)1 << 31;   // every index and every flat offset is an int32
constexpr int kMeshMatVoteThreads = 128;                   // vertices per workgroup of the vote kernel: n_codes * 128 counters of LDS
constexpr int kMeshMatScanBlock = 2048;                    // entries one workgroup of the prefix sum takes (256 threads x 8)
static_assert(kMeshMatMaxCodes * kMeshMatVoteThreads * 4 <= 64 * 1024, "the vote tables fit the LDS a kernel gets unasked");
static_assert(kMeshMatWordBits == 32, "bitmap words are uint32");

struct MeshMatPlan {
  int64_t T, V;
  int32_t K;
  int64_t words;          // W = ceil(V / 32): bitmap words per code row
  int64_t bitmap_words;   // K * W
  int64_t blocks;         // B = max(1, ceil(T / 512)): face blocks
  int64_t block_entries;  // K * B
  int64_t vote_lds;       // bytes of LDS of the vote kernel
  // the label clean-up's scratch, in int32 entries from its start (each section a multiple of 4 entries: 16-byte aligned)
  int64_t scan_blocks;    // workgroups of the prefix sum over the V + 1 offsets
  int64_t at_start, at_cursor, at_corners, at_codes, at_sums;
  int64_t scratch_need;   // bytes
};

#define MESHMAT_REFUSE(code, ...)        \
  do {                                   \
    snprintf(msg, msg_len, __VA_ARGS__); \
    return code;                         \
  } while (0)

inline int64_t meshmat_round4(const int64_t n) { return (n + 3) / 4 * 4; }

// -> 0, or -1 (bad argument) / -2 (unsupported shape) with the reason in msg
inline int meshmat_plan(int64_t T, int64_t V, int K, MeshMatPlan* out, char* msg, size_t msg_len) {
  memset(out, 0, sizeof(*out));
  if (T < 0 || V < 0) MESHMAT_REFUSE(-1, "bad argument: negative size: n_tris = %lld, n_verts = %lld", (long long)T, (long long)V);
  if (V >= kMeshMatIndexLimit) MESHMAT_REFUSE(-2, "unsupported shape: n_verts = %lld must be < 2^31", (long long)V);
  if (T >= (kMeshMatIndexLimit + 2) / 3) MESHMAT_REFUSE(-2, "unsupported shape: 3 n_tris must be < 2^31, n_tris = %lld", (long long)T);
  if (K < 1 || K > kMeshMatMaxCodes) MESHMAT_REFUSE(-2, "unsupported shape: 1 .. %d codes, got %d", kMeshMatMaxCodes, K);
  out->T = T, out->V = V, out->K = K;
  out->words = (V + kMeshMatWordBits - 1) / kMeshMatWordBits;
  out->bitmap_words = out->words * K;
  if (out->bitmap_words >= kMeshMatIndexLimit)
    MESHMAT_REFUSE(-2, "unsupported shape: n_codes * ceil(n_verts / 32) = %lld must be < 2^31", (long long)out->bitmap_words);
  out->blocks = T > 0 ? (T + kMeshMatFacesPerBlock - 1) / kMeshMatFacesPerBlock : 1;
  out->block_entries = out->blocks * K;        // (<= 128 * 2^31 / 3 / 512 < 2^31)
  out->vote_lds = (int64_t)K * kMeshMatVoteThreads * 4;
  out->scan_blocks = (V + 1 + kMeshMatScanBlock - 1) / kMeshMatScanBlock;
  out->at_start = 0;
  out->at_cursor = out->at_start + meshmat_round4(V + 1);
  out->at_corners = out->at_cursor + meshmat_round4(V);
  out->at_codes = out->at_corners + meshmat_round4(3 * T);
  out->at_sums = out->at_codes + meshmat_round4(V);
  out->scratch_need = (out->at_sums + meshmat_round4(out->scan_blocks)) * 4;
  return 0;
}

// which buffer round i of `iters` writes: the last one writes codes_out, the ones before alternate with the scratch's code array
inline bool meshmat_round_writes_out(const int i, const int iters) { return (iters - 1 - i) % 2 == 0; }
