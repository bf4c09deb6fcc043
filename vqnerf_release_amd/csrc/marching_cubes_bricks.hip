// Marching cubes over a sparse set of bricks: the same mesh as marching_cubes.hip gives on the dense field, byte for byte, from the
// field on the bricks the surface passes through alone (geo/mesh.py: marching_cubes_bricks, extract_geometry_sparse).  A brick is
// 8^3 cells = 9^3 stored points (faces shared with its neighbours are stored on both sides); the layout, the ownership rule and the
// leak count are stated in include/vqn_mesh.h, the per-point statements in mc_bricks_core.h.  Same table and conventions as the
// dense kernels: strict u > threshold, t from the _rn intrinsics, one fma per coordinate, vertex id = owner's offset + rank of the axis.
//  * vqn_mc_brick_points: the stored points of a range of brick slots as [x y z] rows, for the SDF kernel;
//  * vqn_mc_brick_classify: per slot of an active brick the owned crossing edges, the triangles of its cell and its dense linear
//    index (int64: the key the caller sorts by to get the dense order), plus the number of leaking faces;
//  * vqn_mc_brick_emit: vertices and triangles at the offsets the caller derived.
// One workgroup per brick: its 729 values go to LDS once (a cell reads 8 of them, an owned point up to 7 more for its edges), four
// waves loop over the points, consecutive lanes along z.  Edges owned by a point of a neighbouring brick (local coordinate 8 on an
// inner face) are resolved through `slot` from that brick's values in global memory: only the outermost layer of cells does that.
#include "common.h"
#include "vqn_mesh.h"

#define VQN_MC_TABLE_QUAL __constant__
#include "mc_table.h"
#include "mc_bricks_core.h"

namespace {

__global__ __launch_bounds__(256) void brick_points_kernel(const float* __restrict__ ax, const float* __restrict__ ay, const float* __restrict__ az,
                                                           const BrickGrid g, const int32_t* __restrict__ brick_ijk, const long first,
                                                           const long count, float* __restrict__ pts) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= count) return;
  const long p = first + r;
  const long s = p / VQN_BRK_N;
  const int l = (int)(p - s * VQN_BRK_N);
  const int lk = l % 9, lj = (l / 9) % 9, li = l / 81;
  Brick k;
  float x = 0.f, y = 0.f, z = 0.f;
  if (brk_brick(g, brick_ijk + 3 * s, &k)) {
    // padding of a clipped brick: the brick's last stored point again (evaluated, never read)
    x = ax[k.x.lo + (li < k.x.ns ? li : k.x.ns - 1)];
    y = ay[k.y.lo + (lj < k.y.ns ? lj : k.y.ns - 1)];
    z = az[k.z.lo + (lk < k.z.ns ? lk : k.z.ns - 1)];
  }
  pts[3 * r + 0] = x;
  pts[3 * r + 1] = y;
  pts[3 * r + 2] = z;
}

__global__ __launch_bounds__(256) void brick_classify_kernel(const float* __restrict__ ub, const int32_t* __restrict__ brick_ijk, const int n_bricks,
                                                             const int32_t* __restrict__ slot, const BrickGrid g, const float thr,
                                                             int32_t* __restrict__ vcount, int32_t* __restrict__ tcount, int64_t* __restrict__ keys,
                                                             int32_t* __restrict__ leaks) {
  __shared__ float u[VQN_BRK_N];
  __shared__ int face[12];                     // [2 f + (0: a point outside seen, 1: a point inside seen)], face f = 2 axis + side
  const int s = blockIdx.x;
  const long base = (long)s * VQN_BRK_N;
  Brick k;
  const bool ok = brk_brick(g, brick_ijk + 3 * (long)s, &k);
  for (int l = threadIdx.x; l < VQN_BRK_N; l += 256) u[l] = ub[base + l];
  if (threadIdx.x < 12) face[threadIdx.x] = 0;
  __syncthreads();
  for (int l = threadIdx.x; l < VQN_BRK_N; l += 256) {
    int nv = 0, nt = 0;
    int64_t key = VQN_BRK_NOKEY;
    if (ok) {
      brk_classify_point(u, g, k, l, thr, &nv, &nt, &key);
      const int lk = l % 9, lj = (l / 9) % 9, li = l / 81;
      if (li < k.x.ns && lj < k.y.ns && lk < k.z.ns) {                      // a stored point: note its side on every face it lies on
        const int in = (int)brk_inside(u[l], thr);
        if (li == 0) face[0 + in] = 1;
        if (li == k.x.ns - 1) face[2 + in] = 1;
        if (lj == 0) face[4 + in] = 1;
        if (lj == k.y.ns - 1) face[6 + in] = 1;
        if (lk == 0) face[8 + in] = 1;
        if (lk == k.z.ns - 1) face[10 + in] = 1;
      }
    }
    vcount[base + l] = nv;
    tcount[base + l] = nt;
    keys[base + l] = key;
  }
  __syncthreads();
  if (ok && threadIdx.x < 6 && face[2 * threadIdx.x] && face[2 * threadIdx.x + 1]) {
    const int a = threadIdx.x >> 1, d = (threadIdx.x & 1) ? 1 : -1;
    const int bi = k.x.b + (a == 0 ? d : 0), bj = k.y.b + (a == 1 ? d : 0), bk = k.z.b + (a == 2 ? d : 0);
    if (bi >= 0 && bi < g.nbx && bj >= 0 && bj < g.nby && bk >= 0 && bk < g.nbz) {
      const int sm = slot[((long)bi * g.nby + bj) * g.nbz + bk];
      if (sm < 0 || sm >= n_bricks) atomicAdd(leaks, 1);                    // the surface runs into a brick that is not in the list
    }
  }
}

__global__ __launch_bounds__(256) void brick_emit_kernel(const float* __restrict__ ub, const int32_t* __restrict__ brick_ijk, const int n_bricks,
                                                         const int32_t* __restrict__ slot, const BrickGrid g, const float thr, const BrickOut o) {
  __shared__ float u[VQN_BRK_N];
  const int s = blockIdx.x;
  Brick k;
  if (!brk_brick(g, brick_ijk + 3 * (long)s, &k)) return;                   // (uniform over the workgroup)
  for (int l = threadIdx.x; l < VQN_BRK_N; l += 256) u[l] = ub[(long)s * VQN_BRK_N + l];
  __syncthreads();
  for (int l = threadIdx.x; l < VQN_BRK_N; l += 256) brk_emit_point(u, ub, slot, n_bricks, g, k, s, l, thr, o);
}

int brick_grid(BrickGrid* g, int nx, int ny, int nz, int64_t n_bricks, const char* who) {
  if (nx < 2 || ny < 2 || nz < 2) {
    vqn_set_error("%s: unsupported shape: every dimension must be >= 2 (got %d x %d x %d)", who, nx, ny, nz);
    return VQN_ESHAPE;
  }
  g->nx = nx; g->ny = ny; g->nz = nz;
  g->nbx = (nx - 1 + VQN_BRK - 1) / VQN_BRK; g->nby = (ny - 1 + VQN_BRK - 1) / VQN_BRK; g->nbz = (nz - 1 + VQN_BRK - 1) / VQN_BRK;
  if ((int64_t)g->nbx * g->nby * g->nbz >= ((int64_t)1 << 31)) {
    vqn_set_error("%s: unsupported shape: the brick grid %d x %d x %d must have < 2^31 entries", who, g->nbx, g->nby, g->nbz);
    return VQN_ESHAPE;
  }
  if (n_bricks < 0) {
    vqn_set_error("%s: bad argument: n_bricks < 0", who);
    return VQN_EARG;
  }
  if (n_bricks * VQN_BRK_N >= ((int64_t)1 << 31)) {
    vqn_set_error("%s: unsupported shape: n_bricks * 729 must be < 2^31 (got %lld bricks)", who, (long long)n_bricks);
    return VQN_ESHAPE;
  }
  return VQN_OK;
}

}  // namespace

extern "C" int vqn_mc_brick_points(const float* ax, const float* ay, const float* az, int nx, int ny, int nz, const int32_t* brick_ijk,
                                   int64_t n_bricks, int64_t first, int64_t count, float* pts, void* stream) {
  BrickGrid g;
  const int rc = brick_grid(&g, nx, ny, nz, n_bricks, __func__);
  if (rc != VQN_OK) return rc;
  VQN_CHECK_ARG(first >= 0 && count >= 0 && first + count <= n_bricks * VQN_BRK_N, "0 <= first, first + count <= n_bricks * 729");
  if (count == 0) return VQN_OK;
  VQN_CHECK_ARG(ax && ay && az && brick_ijk && pts, "null pointer");
  hipLaunchKernelGGL(brick_points_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ax, ay, az, g, brick_ijk,
                     (long)first, (long)count, pts);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_mc_brick_classify(const float* ub, const int32_t* brick_ijk, int64_t n_bricks, const int32_t* slot, int nx, int ny, int nz,
                                     float threshold, int32_t* vert_count, int32_t* tri_count, int64_t* keys, int32_t* leaks, void* stream) {
  BrickGrid g;
  const int rc = brick_grid(&g, nx, ny, nz, n_bricks, __func__);
  if (rc != VQN_OK) return rc;
  VQN_CHECK_ARG(leaks, "null pointer");
  VQN_HIP(hipMemsetAsync(leaks, 0, sizeof(int32_t), (hipStream_t)stream));
  if (n_bricks == 0) return VQN_OK;
  VQN_CHECK_ARG(ub && brick_ijk && slot && vert_count && tri_count && keys, "null pointer");
  hipLaunchKernelGGL(brick_classify_kernel, dim3((unsigned)n_bricks), dim3(256), 0, (hipStream_t)stream, ub, brick_ijk, (int)n_bricks, slot, g,
                     threshold, vert_count, tri_count, keys, leaks);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}

extern "C" int vqn_mc_brick_emit(const float* ub, const int32_t* brick_ijk, int64_t n_bricks, const int32_t* slot, int nx, int ny, int nz,
                                 float threshold, const int32_t* vert_offset, const int32_t* tri_offset, int64_t n_verts, int64_t n_tris,
                                 const float* origin, const float* step, float* verts, int32_t* tris, void* stream) {
  BrickGrid g;
  const int rc = brick_grid(&g, nx, ny, nz, n_bricks, __func__);
  if (rc != VQN_OK) return rc;
  VQN_CHECK_ARG(n_verts >= 0 && n_tris >= 0 && n_verts < ((int64_t)1 << 31) && 3 * n_tris < ((int64_t)1 << 31), "0 <= n_verts, 3 n_tris < 2^31");
  VQN_CHECK_ARG((origin == nullptr) == (step == nullptr), "origin and step come together");
  if (n_bricks == 0 || (n_verts == 0 && n_tris == 0)) return VQN_OK;
  VQN_CHECK_ARG(ub && brick_ijk && slot && vert_offset && tri_offset && (verts || n_verts == 0) && (tris || n_tris == 0), "null pointer");
  BrickOut o;
  o.voff = vert_offset; o.toff = tri_offset; o.n_verts = (int)n_verts; o.n_tris = (int)n_tris;
  o.ox = origin ? origin[0] : 0.f; o.oy = origin ? origin[1] : 0.f; o.oz = origin ? origin[2] : 0.f;
  o.stx = step ? step[0] : 1.f; o.sty = step ? step[1] : 1.f; o.stz = step ? step[2] : 1.f;
  o.verts = verts; o.tris = tris;
  hipLaunchKernelGGL(brick_emit_kernel, dim3((unsigned)n_bricks), dim3(256), 0, (hipStream_t)stream, ub, brick_ijk, (int)n_bricks, slot, g,
                     threshold, o);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}
