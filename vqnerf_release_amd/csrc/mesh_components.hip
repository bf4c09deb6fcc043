// Connected components of an indexed triangle mesh on the device, and the compaction of its triangle list, for the clean-up step
// of the mesh export (geo/mesh.py: components, filter_components).  Two vertices are connected when a triangle uses both;
// labels[v] is the SMALLEST vertex index of v's component, so the result does not depend on how the threads were scheduled.
//
// Lock-free union-find in the caller's label array (no scratch), three launches:
//  * init:    parent[v] = v;
//  * hook:    one thread per triangle (a, b, c), edges (a, b) and (b, c): find both roots, link the LARGER root under the smaller
//             with a compare-and-swap that succeeds only while the larger one is still a root; on failure go on from what the
//             compare-and-swap returned;
//  * flatten: labels[v] = root(v), in place.
//
// INVARIANT: parent[v] <= v at all times, with equality exactly at roots.  Every write keeps it: a hook writes lo < hi into
// parent[hi], path halving writes parent[parent[v]] <= parent[v] < v into parent[v].  Hence
//  * every chase x -> parent[x] strictly decreases and terminates (no cycle can form);
//  * a vertex that has stopped being a root never becomes one again, and its word only ever holds vertices of its own component;
//  * when the hook kernel is done, the root of a tree is smaller than all its members: it is the component's minimum.
// The second point is what makes a STALE read harmless (the eight XCDs' L2s are not coherent with each other inside a kernel; the
// compare-and-swap executes at the memory side and sees the truth): an old value of parent[x] is a former ancestor, still in x's
// component and still < x, so a chase through it ends at a vertex of the right component; if that vertex only looked like a root,
// the compare-and-swap fails and returns its real parent.  The retry takes that returned value, never a re-read of the same word,
// so max(root a, root b) strictly decreases from one attempt to the next and the loop ends.  Loads and stores of parent[] are
// relaxed agent-scope atomics (ordinary vector loads and stores that skip the L1): no data race in the language's sense either.
//
// A vertex index outside [0, n_verts) is a caller error; the kernels skip such an edge (remap: write -1) instead of touching
// memory outside the arrays.
#include "common.h"
#include "vqn_mesh.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;      // grid-stride above this: 8 workgroups of 4 waves per CU keep every SIMD fed

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int* p, const int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with path halving: every vertex on the way is pointed at its grandparent (a value <= the one it replaces)
__device__ __forceinline__ int cc_find(int* __restrict__ parent, int x) {
  int p = cc_load(parent + x);
  while (p != x) {
    const int g = cc_load(parent + p);
    if (g != p) cc_store(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void cc_union(int* __restrict__ parent, int a, int b) {
  a = cc_find(parent, a);
  b = cc_find(parent, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;                 // hi was a root and now hangs under lo
    a = cc_find(parent, old);              // hi had been hooked already: old < hi is its parent, go on from there
    b = cc_find(parent, lo);
  }
}

__global__ __launch_bounds__(kThreads) void cc_init_kernel(int* __restrict__ parent, const int n_verts) {
  for (long v = (long)blockIdx.x * kThreads + threadIdx.x; v < n_verts; v += (long)gridDim.x * kThreads) parent[v] = (int)v;
}

__global__ __launch_bounds__(kThreads) void cc_hook_kernel(const int* __restrict__ tris, const long n_tris, int* __restrict__ parent,
                                                           const int n_verts) {
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < n_tris; t += (long)gridDim.x * kThreads) {
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    const bool oa = (unsigned)a < (unsigned)n_verts, ob = (unsigned)b < (unsigned)n_verts, oc = (unsigned)c < (unsigned)n_verts;
    if (oa && ob && a != b) cc_union(parent, a, b);
    if (ob && oc && b != c) cc_union(parent, b, c);
    if (oa && oc && !ob && a != c) cc_union(parent, a, c);      // (only when b is out of range: a and c are still one triangle's)
  }
}

__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(int* __restrict__ parent, const int n_verts) {
  // in place: a concurrent reader of parent[v] sees the old parent or the root, both on the way to the same root; roots do not change
  for (long v = (long)blockIdx.x * kThreads + threadIdx.x; v < n_verts; v += (long)gridDim.x * kThreads) {
    int x = (int)v, p = cc_load(parent + x);
    while (p != x) {
      x = p;
      p = cc_load(parent + x);
    }
    if (x != (int)v) cc_store(parent + v, x);
  }
}

__global__ __launch_bounds__(kThreads) void remap_tris_kernel(const int* __restrict__ tris_in, const long n_tris,
                                                              const unsigned char* __restrict__ keep_tri, const int* __restrict__ tri_offset,
                                                              const int* __restrict__ new_index, const int n_verts, int* __restrict__ tris_out,
                                                              const long n_out) {
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < n_tris; t += (long)gridDim.x * kThreads) {
    if (!keep_tri[t]) continue;
    const long o = tri_offset[t];
    if (o < 0 || o >= n_out) continue;                        // (offsets that do not belong to this mask: write nothing)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int v = tris_in[3 * t + s];
      tris_out[3 * o + s] = (unsigned)v < (unsigned)n_verts ? new_index[v] : -1;
    }
  }
}

unsigned cc_blocks(const int64_t n) {
  const int64_t b = (n + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

}  // namespace

extern "C" int vqn_mesh_components(const int32_t* tris, int64_t n_tris, int64_t n_verts, int32_t* labels, void* stream) {
  VQN_CHECK_ARG(n_tris >= 0 && n_verts >= 0 && n_verts < ((int64_t)1 << 31) && 3 * n_tris < ((int64_t)1 << 31), "0 <= n_verts, 3 n_tris < 2^31");
  if (n_verts == 0) return VQN_OK;
  VQN_CHECK_ARG(labels && (tris || n_tris == 0), "null pointer");
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_init_kernel, dim3(cc_blocks(n_verts)), dim3(kThreads), 0, s, labels, (int)n_verts);
  VQN_LAUNCH_CHECK();
  if (n_tris == 0) return VQN_OK;                               // every vertex its own component; tris is not read
  hipLaunchKernelGGL(cc_hook_kernel, dim3(cc_blocks(n_tris)), dim3(kThreads), 0, s, tris, (long)n_tris, labels, (int)n_verts);
  VQN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(n_verts)), dim3(kThreads), 0, s, labels, (int)n_verts);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_mesh_remap_tris(const int32_t* tris_in, int64_t n_tris, const uint8_t* keep_tri, const int32_t* tri_offset,
                                   const int32_t* new_index, int64_t n_verts, int32_t* tris_out, int64_t n_out, void* stream) {
  VQN_CHECK_ARG(n_tris >= 0 && n_out >= 0 && n_out <= n_tris && n_verts >= 0 && n_verts < ((int64_t)1 << 31) &&
                    3 * n_tris < ((int64_t)1 << 31), "0 <= n_out <= n_tris, 0 <= n_verts, 3 n_tris < 2^31");
  if (n_tris == 0 || n_out == 0) return VQN_OK;
  VQN_CHECK_ARG(tris_in && keep_tri && tri_offset && tris_out && (new_index || n_verts == 0), "null pointer");
  hipLaunchKernelGGL(remap_tris_kernel, dim3(cc_blocks(n_tris)), dim3(kThreads), 0, (hipStream_t)stream, tris_in, (long)n_tris, keep_tri,
                     tri_offset, new_index, (int)n_verts, tris_out, (long)n_out);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}
