// Material codes on a triangle mesh for gfx950 (include/vqn_mesh_materials.h; the host side is csrc/mesh_materials_plan.h, the plain
// statement tests/mesh_materials_model.py): a label clean-up by majority vote over the mesh, one code per face, and the stable split
// of the mesh into one sub-mesh per code (geo/mesh.py: smooth_labels, face_labels, split_by_label; decomp/material_mesh.py).
//
// Everything is integer work, and every output position follows from a prefix sum, so the results do not depend on how the threads
// were scheduled.  Atomics are used only where the result is a sum or an OR (vertex degrees, face histograms, `changed`, usage
// bits) or where the order does not reach the output (the fill of the corner list: votes are sums).  Every array an atomic wrote is
// read by a LATER launch only.
//
// Label clean-up (vqn_mesh_label_mode), the list built once per call:
//   degree:  one thread per triangle, deg[v] += 1 per corner (triangles with an index out of range are skipped here and so
//            everywhere);
//   scan:    exclusive prefix sum of the V + 1 degrees in place, three launches (sums per 2048 entries, their scan by one
//            workgroup, the entries again with their block's offset);
//   fill:    corner 3 t + i goes to slot start[v] + (cursor[v]++);
//   vote:    one round per launch.  One thread per vertex, whatever its valence: its votes are counted in a table of K counters of
//            its own in LDS (counter k of thread j at [k][j]: 32 consecutive threads hit 32 banks).  Three walks over the vertex's
//            corners: count, find the maximum and the smallest code that holds it, and put the touched counters back to 0 -- so a
//            vertex costs O(valence), not O(K), and the table is cleared once per workgroup.  A fan hub with hundreds of triangles
//            takes the same three walks, in one thread.
//
// Split (vqn_mesh_split_count / _emit): faces are cut into blocks of 512, one 64-lane wave per block.
//   count:   face codes, the block's histogram over the codes (LDS), the usage bits (atomicOr, skipped where a plain read already
//            shows the bit: bits are only ever set, so a stale read costs an atomic and nothing else); then popcounts per word.
//   emit:    the block's K running positions start at its row of the scanned histograms; the wave takes 64 faces at a time, in
//            order: lanes with equal codes find each other by ballot, a lane's position is the running position plus the lanes
//            of its code below it -- stable by construction.  A vertex's rank in its group is the scanned popcount of its word
//            plus the set bits below its own; vert_src is the bitmap written out word by word at the same offsets.
#include "common.h"
#include "launch.h"
#include "wave.h"
#include "mesh_materials_plan.h"
#include "vqn_mesh_materials.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerCu = 8;                 // grid-stride above this many workgroups per CU
constexpr int kScanItems = kMeshMatScanBlock / kThreads;
static_assert(kMeshMatScanBlock % kThreads == 0 && kMeshMatFacesPerBlock % 64 == 0, "whole threads, whole waves");

__device__ __forceinline__ bool in_range(const int x, const int n) { return (unsigned)x < (unsigned)n; }

// ---- the corner list --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mm_degree_kernel(const int* __restrict__ tris, const long T, const int V, int* __restrict__ deg) {
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long)gridDim.x * kThreads) {
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (!(in_range(a, V) && in_range(b, V) && in_range(c, V))) continue;
    atomicAdd(deg + a, 1);
    atomicAdd(deg + b, 1);
    atomicAdd(deg + c, 1);
  }
}

// the sum of a workgroup's 256 values in every thread; `red` holds 4 ints
__device__ __forceinline__ int block_sum(const int v, int* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(kThreads) void mm_scan_sums_kernel(const int* __restrict__ x, const long n, int* __restrict__ sums) {
  __shared__ int red[4];
  const long base = (long)blockIdx.x * kMeshMatScanBlock + (long)threadIdx.x * kScanItems;
  int s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) s += base + i < n ? x[base + i] : 0;
  s = block_sum(s, red);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// exclusive prefix sum of a workgroup's 256 values; `red` holds 4 ints; *total: their sum
__device__ __forceinline__ int block_exclusive_sum(const int v, int* red, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int wave_total;
  const int within = wave_exclusive_sum(v, lane, &wave_total);
  __syncthreads();
  if (lane == 0) red[wave] = wave_total;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < 4; ++w) before += w < wave ? red[w] : 0;
  *total = red[0] + red[1] + red[2] + red[3];
  return before + within;
}

// one workgroup: sums[0 .. nb) -> their exclusive prefix sum, in place
__global__ __launch_bounds__(kThreads) void mm_scan_blocks_kernel(int* __restrict__ sums, const long nb) {
  __shared__ int red[4];
  int carry = 0;
  for (long s = 0; s < nb; s += kThreads) {
    const long i = s + threadIdx.x;
    const int v = i < nb ? sums[i] : 0;
    int total;
    const int e = block_exclusive_sum(v, red, &total);
    if (i < nb) sums[i] = carry + e;
    carry += total;
  }
}

__global__ __launch_bounds__(kThreads) void mm_scan_apply_kernel(int* __restrict__ x, const long n, const int* __restrict__ sums) {
  __shared__ int red[4];
  const long base = (long)blockIdx.x * kMeshMatScanBlock + (long)threadIdx.x * kScanItems;
  int v[kScanItems], s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    v[i] = base + i < n ? x[base + i] : 0;
    s += v[i];
  }
  int total;
  int run = sums[blockIdx.x] + block_exclusive_sum(s, red, &total);
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    if (base + i < n) x[base + i] = run;
    run += v[i];
  }
}

__global__ __launch_bounds__(kThreads) void mm_fill_kernel(const int* __restrict__ tris, const long T, const int V, const int* __restrict__ start,
                                                           int* __restrict__ cursor, int* __restrict__ corners) {
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long)gridDim.x * kThreads) {
    const int idx[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
    if (!(in_range(idx[0], V) && in_range(idx[1], V) && in_range(idx[2], V))) continue;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const long slot = (long)start[idx[i]] + atomicAdd(cursor + idx[i], 1);
      if (slot >= 0 && slot < 3 * T) corners[slot] = (int)(3 * t + i);       // (always, while tris is what the degrees were counted from)
    }
  }
}

// ---- one round of votes -----------------------------------------------------------------------------------------------------------
// the codes of the two other corners of the triangle that corner c belongs to (-1: none)
__device__ __forceinline__ void other_codes(const int* __restrict__ tris, const int* __restrict__ src, const int V, const int c, int* c1,
                                            int* c2) {
  const int t = c / 3, i = c - 3 * t;
  const int n1 = tris[3 * (long)t + (i == 2 ? 0 : i + 1)], n2 = tris[3 * (long)t + (i == 0 ? 2 : i - 1)];
  *c1 = in_range(n1, V) ? src[n1] : -1;
  *c2 = in_range(n2, V) ? src[n2] : -1;
}

__global__ __launch_bounds__(kMeshMatVoteThreads) void mm_vote_kernel(const int* __restrict__ tris, const long T, const int* __restrict__ start,
                                                                      const int* __restrict__ corners, const int* __restrict__ src,
                                                                      int* __restrict__ dst, const int V, const int K, const unsigned self_weight,
                                                                      int* __restrict__ changed) {
  extern __shared__ unsigned votes[];                                  // [K][128]; thread j owns column j and nobody else touches it
  constexpr int TPB = kMeshMatVoteThreads;
  unsigned* mine = votes + threadIdx.x;
  for (int k = 0; k < K; ++k) mine[k * TPB] = 0u;
  int n_changed = 0;
  for (long v0 = (long)blockIdx.x * TPB; v0 < V; v0 += (long)gridDim.x * TPB) {
    const long v = v0 + threadIdx.x;
    if (v >= V) continue;
    const int own = src[v];
    const bool own_ok = in_range(own, K);
    long b = start[v], e = start[v + 1];
    if (b < 0 || e > 3 * T || e < b) b = e = 0;                         // (never, for a list this call built)
    if (own_ok) mine[own * TPB] += self_weight;
    for (long j = b; j < e; ++j) {
      int c1, c2;
      other_codes(tris, src, V, corners[j], &c1, &c2);
      if (in_range(c1, K)) mine[c1 * TPB] += 1u;
      if (in_range(c2, K)) mine[c2 * TPB] += 1u;
    }
    unsigned best = own_ok ? mine[own * TPB] : 0u;
    int best_code = own_ok ? own : 0x7fffffff;
    for (long j = b; j < e; ++j) {
      int c[2];
      other_codes(tris, src, V, corners[j], &c[0], &c[1]);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (!in_range(c[s], K)) continue;
        const unsigned n = mine[c[s] * TPB];
        if (n > best || (n == best && c[s] < best_code)) best = n, best_code = c[s];
      }
    }
    int out = own;
    if (best > 0u && !(own_ok && mine[own * TPB] == best)) out = best_code;
    if (own_ok) mine[own * TPB] = 0u;
    for (long j = b; j < e; ++j) {
      int c1, c2;
      other_codes(tris, src, V, corners[j], &c1, &c2);
      if (in_range(c1, K)) mine[c1 * TPB] = 0u;
      if (in_range(c2, K)) mine[c2 * TPB] = 0u;
    }
    dst[v] = out;
    n_changed += out != own;
  }
  n_changed = wave_sum(n_changed);
  if ((threadIdx.x & 63) == 0 && n_changed) atomicAdd(changed, n_changed);
}

// ---- split --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int face_code_of(const int a, const int b, const int c) {
  if (a == b || a == c) return a;
  if (b == c) return b;
  return min(a, min(b, c));
}

__device__ __forceinline__ void use_bit(unsigned* __restrict__ bitmap, const long word, const unsigned bit) {
  if (!(__hip_atomic_load(bitmap + word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(bitmap + word, bit);
}

// one wave per block of 512 faces
__global__ __launch_bounds__(64) void mm_face_count_kernel(const int* __restrict__ tris, const long T, const int* __restrict__ codes, const int V,
                                                           const int K, const long W, const long B, int* __restrict__ face_code,
                                                           int* __restrict__ block_count, unsigned* __restrict__ bitmap) {
  __shared__ unsigned hist[kMeshMatMaxCodes];
  const int lane = threadIdx.x;
  for (long blk = blockIdx.x; blk < B; blk += gridDim.x) {
    for (int k = lane; k < K; k += 64) hist[k] = 0u;
    __syncthreads();
    for (int r = 0; r < kMeshMatFacesPerBlock / 64; ++r) {
      const long t = blk * kMeshMatFacesPerBlock + r * 64 + lane;
      if (t >= T) continue;
      const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
      int fc = -1;
      if (in_range(a, V) && in_range(b, V) && in_range(c, V)) {
        const int ca = codes[a], cb = codes[b], cc = codes[c];
        if (in_range(ca, K) && in_range(cb, K) && in_range(cc, K)) fc = face_code_of(ca, cb, cc);
      }
      face_code[t] = fc;
      if (fc < 0) continue;
      atomicAdd(hist + fc, 1u);
      use_bit(bitmap, (long)fc * W + (a >> 5), 1u << (a & 31));
      use_bit(bitmap, (long)fc * W + (b >> 5), 1u << (b & 31));
      use_bit(bitmap, (long)fc * W + (c >> 5), 1u << (c & 31));
    }
    __syncthreads();
    for (int k = lane; k < K; k += 64) block_count[(long)k * B + blk] = (int)hist[k];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void mm_popcount_kernel(const unsigned* __restrict__ bitmap, const long n, int* __restrict__ word_count) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) word_count[i] = __popc(bitmap[i]);
}

__global__ __launch_bounds__(64) void mm_face_emit_kernel(const int* __restrict__ tris, const long T, const int V, const int K, const long W,
                                                          const long B, const int* __restrict__ face_code, const int* __restrict__ block_offset,
                                                          const unsigned* __restrict__ bitmap, const int* __restrict__ word_offset, const long F,
                                                          int* __restrict__ face_src, int* __restrict__ tris_local) {
  __shared__ int next[kMeshMatMaxCodes];                               // the next output row of each code, for this block
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long blk = blockIdx.x; blk < B; blk += gridDim.x) {
    for (int k = lane; k < K; k += 64) next[k] = block_offset[(long)k * B + blk];
    __syncthreads();
    for (int r = 0; r < kMeshMatFacesPerBlock / 64; ++r) {                // (wave-uniform: every lane takes every round)
      const long t = blk * kMeshMatFacesPerBlock + r * 64 + lane;
      const int fc = t < T ? face_code[t] : -1;
      const bool has = in_range(fc, K);
      long row = -1;
      unsigned long long pending = __ballot(has);
      while (pending) {                                                // wave-uniform
        const int leader = __ffsll((long long)pending) - 1;
        const int k = __builtin_amdgcn_readlane(fc, leader);
        const bool same_code = has && fc == k;
        const unsigned long long same = __ballot(same_code);
        const int first = next[k];
        if (same_code) row = (long)first + __popcll(same & below);
        if (lane == leader) next[k] = first + __popcll(same);
        pending &= ~same;
      }
      __syncthreads();                                                 // the next round reads what this round's leaders wrote
      if (!has || row < 0 || row >= F) continue;
      face_src[row] = (int)t;
      const long krow = (long)fc * W;
      const int group_first = word_offset[krow];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int v = tris[3 * t + i];
        int rank = -1;
        if (in_range(v, V)) {
          const long word = krow + (v >> 5);
          rank = word_offset[word] - group_first + __popc(bitmap[word] & ((1u << (v & 31)) - 1u));
        }
        tris_local[3 * row + i] = rank;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void mm_vert_emit_kernel(const unsigned* __restrict__ bitmap, const long n, const long W,
                                                                const int* __restrict__ word_offset, const long S, int* __restrict__ vert_src) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    unsigned bits = bitmap[i];
    if (!bits) continue;
    long slot = word_offset[i];
    const int first = (int)((i % W) * kMeshMatWordBits);
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1u;
      if (slot >= 0 && slot < S) vert_src[slot] = first + b;
      ++slot;
    }
  }
}

dim3 mm_grid(const int64_t n, const int per_block) { return dim3((unsigned)vqn_grid1((long)((n + per_block - 1) / per_block), kPerCu)); }

int mm_plan(const char* fn, int64_t T, int64_t V, int K, MeshMatPlan* plan) {
  char msg[200];
  const int rc = meshmat_plan(T, V, K, plan, msg, sizeof(msg));
  if (rc) vqn_set_error("%s: %s", fn, msg);
  return rc;
}

}  // namespace

extern "C" int64_t vqn_mesh_label_scratch_bytes(int64_t n_tris, int64_t n_verts) {
  MeshMatPlan g;
  const int rc = mm_plan(__func__, n_tris, n_verts, 1, &g);
  return rc ? rc : g.scratch_need;
}

extern "C" int vqn_mesh_label_mode(const int32_t* tris, int64_t n_tris, const int32_t* codes_in, int64_t n_verts, int n_codes, int self_weight,
                                   int iters, int32_t* codes_out, int32_t* changed, void* scratch, int64_t scratch_bytes, void* stream) {
  VQN_CHECK_ARG(self_weight >= 0 && iters >= 0, "self_weight and iters must not be negative");
  MeshMatPlan g;
  const int rc = mm_plan(__func__, n_tris, n_verts, n_codes, &g);
  if (rc) return rc;
  VQN_CHECK_ARG((codes_in && codes_out) || n_verts == 0, "null codes");
  VQN_CHECK_ARG(tris || n_tris == 0, "null tris");
  VQN_CHECK_ARG(changed || iters == 0, "null changed");
  VQN_CHECK_ARG(codes_in != codes_out || n_verts == 0, "codes_out must not be codes_in");
  VQN_CHECK_ARG(iters == 0 || n_verts == 0 || (scratch && ((uintptr_t)scratch & 15) == 0 && scratch_bytes >= g.scratch_need),
                "scratch is null, misaligned or too small");
  const hipStream_t s = (hipStream_t)stream;
  if (iters > 0) VQN_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)iters, s));
  if (n_verts == 0) return VQN_OK;
  if (iters == 0) {
    VQN_HIP(hipMemcpyAsync(codes_out, codes_in, sizeof(int32_t) * (size_t)n_verts, hipMemcpyDeviceToDevice, s));
    return VQN_OK;
  }
  int* const base = (int*)scratch;
  int *start = base + g.at_start, *cursor = base + g.at_cursor, *corners = base + g.at_corners, *other = base + g.at_codes,
      *sums = base + g.at_sums;
  const int V = (int)n_verts;
  const long T = (long)n_tris, n_scan = (long)n_verts + 1;
  // start and cursor lie next to each other: one memset clears both
  VQN_HIP(hipMemsetAsync(start, 0, sizeof(int) * (size_t)(g.at_corners - g.at_start), s));
  if (T > 0) {
    if (int e = vqn_launch(__func__, mm_degree_kernel, mm_grid(T, kThreads), kThreads, 0, stream, tris, T, V, start)) return e;
    if (int e = vqn_launch(__func__, mm_scan_sums_kernel, dim3((unsigned)g.scan_blocks), kThreads, 0, stream, (const int*)start, n_scan, sums)) return e;
    if (int e = vqn_launch(__func__, mm_scan_blocks_kernel, dim3(1), kThreads, 0, stream, sums, (long)g.scan_blocks)) return e;
    if (int e = vqn_launch(__func__, mm_scan_apply_kernel, dim3((unsigned)g.scan_blocks), kThreads, 0, stream, start, n_scan, (const int*)sums)) return e;
    if (int e = vqn_launch(__func__, mm_fill_kernel, mm_grid(T, kThreads), kThreads, 0, stream, tris, T, V, (const int*)start, cursor, corners)) return e;
  }
  const int32_t* src = codes_in;
  for (int i = 0; i < iters; ++i) {
    int32_t* dst = meshmat_round_writes_out(i, iters) ? codes_out : other;
    if (int e = vqn_launch(__func__, mm_vote_kernel, mm_grid(n_verts, kMeshMatVoteThreads), kMeshMatVoteThreads, (size_t)g.vote_lds, stream, tris,
                           T, (const int*)start, (const int*)corners, src, dst, V, n_codes, (unsigned)self_weight, changed + i))
      return e;
    src = dst;
  }
  return VQN_OK;
}

extern "C" int vqn_mesh_split_count(const int32_t* tris, int64_t n_tris, const int32_t* codes, int64_t n_verts, int n_codes, int32_t* face_code,
                                    int32_t* block_count, uint32_t* bitmap, int32_t* word_count, void* stream) {
  MeshMatPlan g;
  const int rc = mm_plan(__func__, n_tris, n_verts, n_codes, &g);
  if (rc) return rc;
  VQN_CHECK_ARG(block_count && ((tris && face_code) || n_tris == 0) && ((codes && bitmap && word_count) || n_verts == 0), "null pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (g.bitmap_words > 0) VQN_HIP(hipMemsetAsync(bitmap, 0, sizeof(uint32_t) * (size_t)g.bitmap_words, s));
  if (int e = vqn_launch(__func__, mm_face_count_kernel, dim3((unsigned)vqn_grid1((long)g.blocks, 4 * kPerCu)), 64, 0, stream, tris, (long)n_tris,
                         codes, (int)n_verts, n_codes, (long)g.words, (long)g.blocks, face_code, block_count, bitmap))
    return e;
  if (g.bitmap_words > 0)
    if (int e = vqn_launch(__func__, mm_popcount_kernel, mm_grid(g.bitmap_words, kThreads), kThreads, 0, stream, (const unsigned*)bitmap,
                           (long)g.bitmap_words, word_count))
      return e;
  return VQN_OK;
}

extern "C" int vqn_mesh_split_emit(const int32_t* tris, int64_t n_tris, int64_t n_verts, int n_codes, const int32_t* face_code,
                                   const int32_t* block_offset, const uint32_t* bitmap, const int32_t* word_offset, int64_t n_faces,
                                   int64_t n_slots, int32_t* face_src, int32_t* tris_local, int32_t* vert_src, void* stream) {
  MeshMatPlan g;
  const int rc = mm_plan(__func__, n_tris, n_verts, n_codes, &g);
  if (rc) return rc;
  VQN_CHECK_ARG(n_faces >= 0 && n_faces <= n_tris && n_slots >= 0 && n_slots <= 3 * n_faces && n_slots <= (int64_t)n_codes * n_verts,
                "0 <= n_faces <= n_tris and 0 <= n_slots <= 3 n_faces, n_codes * n_verts");
  if (n_faces == 0) return VQN_OK;
  VQN_CHECK_ARG(tris && face_code && block_offset && bitmap && word_offset && face_src && tris_local && (vert_src || n_slots == 0), "null pointer");
  if (int e = vqn_launch(__func__, mm_face_emit_kernel, dim3((unsigned)vqn_grid1((long)g.blocks, 4 * kPerCu)), 64, 0, stream, tris, (long)n_tris,
                         (int)n_verts, n_codes, (long)g.words, (long)g.blocks, face_code, block_offset, (const unsigned*)bitmap, word_offset,
                         (long)n_faces, face_src, tris_local))
    return e;
  if (n_slots > 0)
    if (int e = vqn_launch(__func__, mm_vert_emit_kernel, mm_grid(g.bitmap_words, kThreads), kThreads, 0, stream, (const unsigned*)bitmap,
                           (long)g.bitmap_words, (long)g.words, word_offset, (long)n_slots, vert_src))
      return e;
  return VQN_OK;
}
