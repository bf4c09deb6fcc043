// Mean-shift clustering on the device: the baseline of the paper's segmentation table, which the reference computes on the host with
// sklearn.cluster.MeanShift (decomp/nerfvq_nfr3/meanshift.py: flat kernel, every sample a seed, cluster_all=True) on at most 10,000
// subsampled pixels (decomp/nerfactor/util/meanshift.py, decomp/meanshift.py; the float64 statement is tests/meanshift_model.py).
// Features are float64 [n][D], row-major, 1 <= D <= 8, n * D < 2^31.
//
// The arithmetic is fixed, so that the statement can be followed decision by decision:
//   d2(x, m) = sum over d = 0 .. D-1, in that order, of (x_d - m_d) * (x_d - m_d): product and sum rounded separately (no FMA);
//   x is a neighbour of m when d2 <= b * b;   mean = sum / count (a division, not a reciprocal);
//   a seed stops when sqrt(d2(m', m)) <= 1e-3 * b, or when max_iter iterations are complete.
//
//  * meanshift_seek_kernel<D>: ONE launch takes every seed to convergence.  The points never change, so seeds are independent: a
//    workgroup of kSeekWaves = 8 waves owns kSeekSeeds = 64 seeds, ONE PER LANE, the same 64 in every wave, and loops until all of
//    them have stopped; nothing is exchanged between workgroups and nothing is read back.  Per iteration the points pass through
//    LDS in tiles of kSeekTile = 256 (a straight copy of 256 * D doubles); wave w tests points [32 w, 32 w + 32) of every tile
//    against its lanes' means (all lanes read one LDS address: a broadcast, no bank conflict) and adds the neighbours to D + 1
//    registers.  The eight partial sums of a seed are then added in wave order, by every wave for itself (so every wave holds the
//    new mean and the stop decision, and the loop condition is uniform without another exchange).  A seed's sum is therefore
//    ((p_0 + p_1) + ...) + p_7 with p_w the sum, in ascending index, of its neighbours i with (i mod 256) / 32 = w: the order depends
//    on the point indices alone -- not on the seed, the workgroup or timing; no atomics.  Two seeds with the same last neighbour set
//    end on bit-identical means, which is what lets the merge count them once.
//  * meanshift_merge_kernel<D>: one workgroup walks the candidates (sorted by the caller: descending neighbour count, then
//    descending coordinates; count 0 = dropped seeds, last) in ROUNDS: the first candidate that is neither kept nor suppressed is
//    kept, then all lanes suppress the later candidates within d2 <= b * b of it.  K rounds, not M; the result is the sequential
//    walk's (a kept centre can have no earlier undecided neighbour).  Exact duplicates need no pass of their own: d2 = 0.
//  * meanshift_assign_kernel<D>: one point per lane against the centres held in LDS (chunks of kAssignCentres = 512), nearest by
//    d2 with ties to the lowest index (strict <); optionally the distance sqrt(d2) and, for b > 0, label -1 where it is > b.
#include "common.h"
#include "vqn_eval.h"

// every product, sum and quotient below is rounded on its own, as the statement's are
#pragma clang fp contract(off)

namespace {

constexpr int kMaxD = VQN_MEANSHIFT_MAX_DIM;
constexpr int kSeekWaves = 8;
constexpr int kSeekSeeds = VQN_MEANSHIFT_SEEDS_PER_GROUP;    // seeds per workgroup: one per lane
constexpr int kSeekThreads = kSeekWaves * 64;
constexpr int kSeekTile = VQN_MEANSHIFT_POINTS_PER_TILE;     // 256 points staged per pass
constexpr int kSeekSlice = kSeekTile / kSeekWaves;           // points of a tile per wave: 32
constexpr int kMergeThreads = 1024;
constexpr int kAssignThreads = VQN_MEANSHIFT_ASSIGN_SPAN;    // points per workgroup and pass
constexpr int kAssignCentres = VQN_MEANSHIFT_ASSIGN_CENTRES; // centres staged in LDS at a time
static_assert(kSeekSlice * kSeekWaves == kSeekTile, "a tile is whole slices");
constexpr int kAssignGridCap = 4096;
constexpr int kUndecided = 0, kKept = 1, kSuppressed = 2;

template <int D>
__device__ __forceinline__ double dist2(const double* __restrict__ x, const double (&m)[D]) {
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double t = x[d] - m[d];
    const double q = t * t;
    s = s + q;
  }
  return s;
}

template <int D>
__global__ __launch_bounds__(kSeekThreads) void meanshift_seek_kernel(const double* __restrict__ points, const int64_t n,
                                                                      const double* __restrict__ seeds, const int64_t S, const double bb,
                                                                      const double stop, const int max_iter, double* __restrict__ means,
                                                                      int32_t* __restrict__ counts, int32_t* __restrict__ iters) {
  __shared__ double tile[kSeekTile * D];
  __shared__ double part[kSeekWaves][D][kSeekSeeds];
  __shared__ int part_n[kSeekWaves][kSeekSeeds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t seed = (int64_t)blockIdx.x * kSeekSeeds + lane;
  bool active = seed < S;
  double m[D];
#pragma unroll
  for (int d = 0; d < D; ++d) m[d] = active ? seeds[seed * D + d] : 0.0;
  int count = 0, done = 0;

  while (__ballot(active) != 0ull) {                         // the same 64 seeds in every wave: uniform over the workgroup
    double sum[D];
#pragma unroll
    for (int d = 0; d < D; ++d) sum[d] = 0.0;
    int cnt = 0;
    for (int64_t p0 = 0; p0 < n; p0 += kSeekTile) {
      const int tn = (int)(n - p0 < kSeekTile ? n - p0 : kSeekTile);
      __syncthreads();                                       // the last pass's readers are through
      for (int i = tid; i < tn * D; i += kSeekThreads) tile[i] = points[p0 * D + i];
      __syncthreads();
      const int lo = wave * kSeekSlice, hi = lo + kSeekSlice < tn ? lo + kSeekSlice : tn;
      if (active) {
#pragma unroll 4
        for (int j = lo; j < hi; ++j) {
          const double* x = &tile[j * D];
          if (dist2<D>(x, m) <= bb) {
            cnt += 1;
#pragma unroll
            for (int d = 0; d < D; ++d) sum[d] = sum[d] + x[d];
          }
        }
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) part[wave][d][lane] = sum[d];
    part_n[wave][lane] = cnt;
    __syncthreads();                                         // (the next write to part follows the two barriers of a tile pass: n >= 1)
    double tot[D];
#pragma unroll
    for (int d = 0; d < D; ++d) tot[d] = part[0][d][lane];
    int c = part_n[0][lane];
    for (int w = 1; w < kSeekWaves; ++w) {                   // wave order
#pragma unroll
      for (int d = 0; d < D; ++d) tot[d] = tot[d] + part[w][d][lane];
      c += part_n[w][lane];
    }
    if (active) {
      count = c;
      if (c == 0) {
        active = false;                                      // no neighbour: the seed is dropped, its mean stays
      } else {
        const double cd = (double)c;
        double nm[D];
#pragma unroll
        for (int d = 0; d < D; ++d) nm[d] = tot[d] / cd;
        const double shift = sqrt(dist2<D>(nm, m));
#pragma unroll
        for (int d = 0; d < D; ++d) m[d] = nm[d];
        if (shift <= stop || done == max_iter)
          active = false;
        else
          done += 1;
      }
    }
  }
  if (wave == 0 && seed < S) {
#pragma unroll
    for (int d = 0; d < D; ++d) means[seed * D + d] = m[d];
    counts[seed] = count;
    iters[seed] = done;
  }
}

template <int D>
__global__ __launch_bounds__(kMergeThreads) void meanshift_merge_kernel(const double* __restrict__ cand, const int32_t* __restrict__ cand_count,
                                                                        const int64_t M, const double bb, uint8_t* state,
                                                                        uint8_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  __shared__ int first;                                      // (M * D < 2^31)
  const int tid = threadIdx.x;
  for (int64_t i = tid; i < M; i += kMergeThreads) state[i] = cand_count[i] > 0 ? kUndecided : kSuppressed;
  int K = 0;
  int64_t start = 0;
  for (;;) {
    // ---- the first undecided candidate at or after `start`, a block of 1024 at a time ----
    int64_t found = -1;
    for (int64_t base = start; base < M; base += kMergeThreads) {
      __syncthreads();                                       // the writes to state of the last round; the readers of `first`
      if (tid == 0) first = (int)M;
      __syncthreads();
      const int64_t i = base + tid;
      if (i < M && state[i] == kUndecided) atomicMin(&first, (int)i);
      __syncthreads();
      if (first < M) {
        found = first;
        break;
      }
    }
    if (found < 0) break;                                    // uniform: every thread read the same `first`
    double c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) c[d] = cand[found * D + d];
    for (int64_t i = found + 1 + tid; i < M; i += kMergeThreads)
      if (state[i] == kUndecided && dist2<D>(&cand[i * D], c) <= bb) state[i] = kSuppressed;
    if (tid == 0) state[found] = kKept;
    K += 1;
    start = found + 1;
  }
  __syncthreads();
  for (int64_t i = tid; i < M; i += kMergeThreads) kept[i] = state[i] == kKept ? 1 : 0;
  if (tid == 0) *n_kept = K;
}

template <int D>
__global__ __launch_bounds__(kAssignThreads) void meanshift_assign_kernel(const double* __restrict__ points, const int64_t n,
                                                                          const double* __restrict__ centres, const int K, const double b,
                                                                          int32_t* __restrict__ labels, double* __restrict__ dist) {
  __shared__ double cen[kAssignCentres * D];
  const int tid = threadIdx.x;
  const bool resident = K <= kAssignCentres;                 // staged once; more centres pass through in chunks, per pass
  if (resident) {
    for (int j = tid; j < K * D; j += kAssignThreads) cen[j] = centres[j];
    __syncthreads();
  }
  const int64_t passes = (n + kAssignThreads - 1) / kAssignThreads;
  for (int64_t pass = blockIdx.x; pass < passes; pass += gridDim.x) {        // the same trip count for every lane of the workgroup
    const int64_t i = pass * kAssignThreads + tid;
    const bool live = i < n;
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = live ? points[i * D + d] : 0.0;
    double best = __builtin_inf();
    int arg = 0;
    for (int k0 = 0; k0 < K; k0 += kAssignCentres) {
      const int kn = K - k0 < kAssignCentres ? K - k0 : kAssignCentres;
      if (!resident) {
        __syncthreads();                                     // the last chunk's readers are through
        for (int j = tid; j < kn * D; j += kAssignThreads) cen[j] = centres[(int64_t)k0 * D + j];
        __syncthreads();
      }
      for (int k = 0; k < kn; ++k) {
        const double d2 = dist2<D>(&cen[k * D], x);
        if (d2 < best) best = d2, arg = k0 + k;              // strict: a tie stays with the lowest index
      }
    }
    if (live) {
      const double r = sqrt(best);
      labels[i] = b > 0.0 && r > b ? -1 : arg;
      if (dist) dist[i] = r;
    }
  }
}

bool shape_ok(const char* fn, const int64_t n, const int D) {
  if (D < 1 || D > kMaxD || n < 1 || n * D >= ((int64_t)1 << 31)) {
    vqn_set_error("%s: unsupported shape: 1 <= D <= %d features and 1 <= n, n * D < 2^31, got n = %lld, D = %d", fn, kMaxD, (long long)n, D);
    return false;
  }
  return true;
}

#define VQN_MS_DISPATCH(D, CALL) \
  switch (D) {                   \
    case 1: { constexpr int kD = 1; CALL; } break; \
    case 2: { constexpr int kD = 2; CALL; } break; \
    case 3: { constexpr int kD = 3; CALL; } break; \
    case 4: { constexpr int kD = 4; CALL; } break; \
    case 5: { constexpr int kD = 5; CALL; } break; \
    case 6: { constexpr int kD = 6; CALL; } break; \
    case 7: { constexpr int kD = 7; CALL; } break; \
    default: { constexpr int kD = 8; CALL; } break; \
  }

}  // namespace

extern "C" int vqn_meanshift_seek(const double* points, int64_t n, const double* seeds, int64_t n_seeds, int D, double bandwidth, int max_iter,
                                  double* means, int32_t* counts, int32_t* iters, void* stream) {
  if (!shape_ok(__func__, n, D) || !shape_ok(__func__, n_seeds, D)) return VQN_ESHAPE;
  if (!(bandwidth > 0.0) || max_iter < 0) {
    vqn_set_error("%s: bad argument: bandwidth > 0 and max_iter >= 0, got %g and %d", __func__, bandwidth, max_iter);
    return VQN_EARG;
  }
  if (!points || !seeds || !means || !counts || !iters) {
    vqn_set_error("%s: bad argument: null pointer", __func__);
    return VQN_EARG;
  }
  const double bb = bandwidth * bandwidth, stop = 1e-3 * bandwidth;
  const unsigned blocks = (unsigned)((n_seeds + kSeekSeeds - 1) / kSeekSeeds);
  VQN_MS_DISPATCH(D, hipLaunchKernelGGL((meanshift_seek_kernel<kD>), dim3(blocks), dim3(kSeekThreads), 0, (hipStream_t)stream, points, n, seeds,
                                        n_seeds, bb, stop, max_iter, means, counts, iters));
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int64_t vqn_meanshift_merge_scratch_bytes(int64_t n_candidates, int D) {
  if (D < 1 || D > kMaxD || n_candidates < 1 || n_candidates * D >= ((int64_t)1 << 31)) return 0;
  return (n_candidates + 63) / 64 * 64;                      // one state byte per candidate
}

extern "C" int vqn_meanshift_merge(const double* candidates, const int32_t* cand_counts, int64_t n_candidates, int D, double bandwidth,
                                   void* scratch, int64_t scratch_bytes, uint8_t* kept, int32_t* n_kept, void* stream) {
  if (!shape_ok(__func__, n_candidates, D)) return VQN_ESHAPE;
  const int64_t need = vqn_meanshift_merge_scratch_bytes(n_candidates, D);
  if (!(bandwidth > 0.0) || !candidates || !cand_counts || !kept || !n_kept || !scratch || scratch_bytes < need) {
    vqn_set_error("%s: bad argument: bandwidth <= 0, a null pointer, or scratch smaller than vqn_meanshift_merge_scratch_bytes (%lld bytes)",
                  __func__, (long long)need);
    return VQN_EARG;
  }
  const double bb = bandwidth * bandwidth;
  VQN_MS_DISPATCH(D, hipLaunchKernelGGL((meanshift_merge_kernel<kD>), dim3(1), dim3(kMergeThreads), 0, (hipStream_t)stream, candidates,
                                        cand_counts, n_candidates, bb, (uint8_t*)scratch, kept, n_kept));
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_meanshift_assign(const double* points, int64_t n, const double* centres, int K, int D, double bandwidth, int32_t* labels,
                                    double* dist, void* stream) {
  if (!shape_ok(__func__, n, D) || !shape_ok(__func__, K, D)) return VQN_ESHAPE;
  if (!points || !centres || !labels) {
    vqn_set_error("%s: bad argument: null pointer", __func__);
    return VQN_EARG;
  }
  const int64_t passes = (n + kAssignThreads - 1) / kAssignThreads;
  const unsigned blocks = (unsigned)(passes < kAssignGridCap ? passes : kAssignGridCap);
  VQN_MS_DISPATCH(D, hipLaunchKernelGGL((meanshift_assign_kernel<kD>), dim3(blocks), dim3(kAssignThreads), 0, (hipStream_t)stream, points, n,
                                        centres, K, bandwidth, labels, dist));
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}
