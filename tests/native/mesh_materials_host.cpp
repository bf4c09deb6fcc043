// Stand-alone check of the host side of the mesh-material kernels (csrc/mesh_materials_plan.h) under ASan / UBSan: the limits, the
// bitmap geometry at its word edges, the face blocks, the scratch layout of the label clean-up, which buffer a round writes, and
// every refusal with its reason.  Run by tests/test_mesh_materials_native.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mesh_materials_plan.h"

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                \
    }                                                            \
  } while (0)

static int refusals = 0;
static void refused(int64_t T, int64_t V, int K, int code, const char* word) {
  MeshMatPlan g;
  char msg[256];
  msg[0] = 0;
  const int rc = meshmat_plan(T, V, K, &g, msg, sizeof(msg));
  ++refusals;
  if (rc != code || !strstr(msg, word) || !strstr(msg, code == -2 ? "unsupported shape" : "bad argument")) {
    printf("FAILED refusal %d: rc %d (want %d), reason '%s' (want '%s')\n", refusals, rc, code, msg, word);
    ++failures;
  }
}

int main() {
  MeshMatPlan g;
  char msg[256];
  const int64_t two31 = (int64_t)1 << 31;
  int shapes = 0;

  // ---- the limits as the header states them ----
  CHECK(kMeshMatMaxCodes == 128 && kMeshMatFacesPerBlock == 512 && kMeshMatWordBits == 32);

  // ---- an export-sized mesh: 2 * 10^6 vertices, 4 * 10^6 triangles, 128 codes ----
  msg[0] = 0;
  CHECK(meshmat_plan(4000000, 2000000, 128, &g, msg, sizeof(msg)) == 0 && msg[0] == 0);
  CHECK(g.words == 62500 && g.bitmap_words == 8000000 && g.blocks == 7813 && g.block_entries == 7813 * 128);
  CHECK(g.vote_lds == 128 * 128 * 4 && g.scan_blocks == 977);
  CHECK(g.at_start == 0 && g.at_cursor == 2000004 && g.at_corners == 4000004 && g.at_codes == 16000004 && g.at_sums == 18000004);
  CHECK(g.scratch_need == (18000004 + 980) * 4);
  // (far below a V x K vote table: 2 * 10^6 * 128 * 4 bytes)
  CHECK(g.scratch_need < (int64_t)2000000 * 128 * 4 / 10);

  // ---- the bitmap and the blocks at their edges ----
  const int64_t Vs[] = {0, 1, 31, 32, 33, 63, 64, 65, 5000, two31 - 1};
  const int64_t Ts[] = {0, 1, 511, 512, 513, 1024, 1025, (two31 - 1) / 3};
  const int Ks[] = {1, 2, 64, 65, 128};
  for (int64_t V : Vs)
    for (int64_t T : Ts)
      for (int K : Ks) {
        msg[0] = 0;
        const int rc = meshmat_plan(T, V, K, &g, msg, sizeof(msg));
        const int64_t W = (V + 31) / 32;
        if (W * K >= two31) {
          CHECK(rc == -2 && strstr(msg, "ceil(n_verts / 32)"));
          continue;
        }
        ++shapes;
        CHECK(rc == 0 && msg[0] == 0);
        CHECK(g.words == W && g.words * 32 >= V && (g.words - 1) * 32 < V + (V == 0));
        CHECK(g.bitmap_words == W * K && g.bitmap_words < two31);
        CHECK(g.blocks >= 1 && g.blocks * 512 >= T && (g.blocks - 1) * 512 < T + (T == 0) && g.block_entries == g.blocks * K);
        CHECK(g.block_entries < two31);
        CHECK(g.vote_lds == (int64_t)K * 128 * 4 && g.vote_lds <= 64 * 1024);
        CHECK(g.scan_blocks * kMeshMatScanBlock >= V + 1 && (g.scan_blocks - 1) * kMeshMatScanBlock < V + 1);
        // the sections follow each other, hold what they are for, and start at multiples of 16 bytes
        CHECK(g.at_start == 0 && g.at_cursor - g.at_start >= V + 1 && g.at_corners - g.at_cursor >= V && g.at_codes - g.at_corners >= 3 * T &&
              g.at_sums - g.at_codes >= V && g.scratch_need / 4 - g.at_sums >= g.scan_blocks);
        CHECK(g.at_cursor % 4 == 0 && g.at_corners % 4 == 0 && g.at_codes % 4 == 0 && g.at_sums % 4 == 0 && g.scratch_need % 16 == 0);
        // the scratch does not depend on K
        MeshMatPlan g1;
        CHECK(meshmat_plan(T, V, 1, &g1, msg, sizeof(msg)) == 0 && g1.scratch_need == g.scratch_need);
      }
  // the largest bitmap that passes and the first that does not: K * W = 2^31 - 128 at W = 2^24 - 1, 2^31 at W = 2^24
  CHECK(meshmat_plan(0, ((int64_t)1 << 29) - 32, 128, &g, msg, sizeof(msg)) == 0 && g.bitmap_words == two31 - 128);
  refused(0, (int64_t)1 << 29, 128, -2, "ceil(n_verts / 32)");
  refused(0, ((int64_t)1 << 29) - 31, 128, -2, "ceil(n_verts / 32)");
  CHECK(meshmat_plan(0, two31 - 1, 31, &g, msg, sizeof(msg)) == 0);
  refused(0, two31 - 1, 32, -2, "ceil(n_verts / 32)");

  // ---- refusals ----
  refused(-1, 10, 4, -1, "negative size");
  refused(10, -1, 4, -1, "negative size");
  refused(-1, two31, 0, -1, "negative size");               // a negative size is reported before any shape
  refused(10, two31, 4, -2, "n_verts");
  refused(10, two31 + 5, 4, -2, "n_verts");
  refused((two31 - 1) / 3 + 1, 10, 4, -2, "3 n_tris");
  refused(two31, 10, 4, -2, "3 n_tris");
  refused(10, 10, 0, -2, "codes");
  refused(10, 10, -3, -2, "codes");
  refused(10, 10, 129, -2, "codes");
  CHECK(3 * ((two31 - 1) / 3) < two31 && 3 * ((two31 - 1) / 3 + 1) >= two31);

  // ---- which buffer a round writes: the last one the caller's, alternating before it, never the one it reads ----
  for (int iters = 1; iters <= 7; ++iters) {
    CHECK(meshmat_round_writes_out(iters - 1, iters));
    for (int i = 1; i < iters; ++i) CHECK(meshmat_round_writes_out(i, iters) != meshmat_round_writes_out(i - 1, iters));
  }

  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("mesh materials plan ok: %d shapes, %d refusals\n", shapes, refusals);
  return 0;
}
