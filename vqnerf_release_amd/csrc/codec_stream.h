// The back end the device codecs share (csrc/jpeg_encode.hip, csrc/png_encode.hip).  A coding kernel leaves every item (a restart
// interval, a deflate segment) in a slot of worst-case size with its length in `lens`; one workgroup then places the items in the
// output and a compaction launch copies the slots there.  Here: the partition of the items over that workgroup's threads, the scan
// of their totals, and the copy.  What an item adds besides its bytes and what goes to `meta` stay with the codec.  Device only.
#pragma once
#include "codec_plan.h"
#include "common.h"

static_assert(VQN_EARG == -1 && VQN_ESHAPE == -2, "codec_refuse hands the planners' codes on as they are");

// The one-workgroup scan: thread tid adds up what the items of its run [*i0, *i1) come to in the stream (ceil(items / THREADS) items
// each, the last runs short or empty), the threads' totals are scanned, every thread walks its run again from its first item's place.
template <int THREADS>
__device__ __forceinline__ void codec_run(const int64_t items, const int tid, int64_t* i0, int64_t* i1) {
  const int64_t per = (items + THREADS - 1) / THREADS;
  *i0 = min(items, tid * per), *i1 = min(items, *i0 + per);
}

// `mine`: the total of this thread's run -> the total of the runs in front of it.  The totals go through THREADS words of LDS, which
// thread 0 scans serially.  Called by the whole workgroup.  (png_scan_kernel keeps this step in its body: profiles/wave_codec_asm.txt.)
template <int THREADS>
__device__ __forceinline__ int64_t codec_scan_runs(const int64_t mine, const int tid) {
  __shared__ int64_t totals[THREADS];
  totals[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < THREADS; ++t) {
      const int64_t v = totals[t];
      totals[t] = run;
      run += v;
    }
  }
  __syncthreads();
  return totals[tid];
}

// the n bytes of a slot -> byte `at` of the output onwards, by the THREADS threads of a workgroup
template <int THREADS>
__device__ __forceinline__ void codec_copy_slot(const uint8_t* src, uint8_t* out, const int64_t at, const int64_t n, const int tid) {
  for (int64_t i = tid; i < n; i += THREADS) out[at + i] = src[i];
}
