// Per-point statements of the brick marching cubes (marching_cubes_bricks.hip): which points a brick stores and owns, what one owned
// point counts and what it writes.  Kept apart from the kernels so that the same text also compiles as plain C++ (no __HIPCC__): the
// kernels only stage a brick's 9^3 values in LDS and loop these functions over its points.  Conventions: mc_table.h, which the
// includer brings in first (with VQN_MC_TABLE_QUAL set for its side); layout and ownership: include/vqn_mesh.h.  Not public.
#pragma once
#include <stdint.h>

#include "../../include/vqn_mesh.h"  // (by path: the stand-alone build of this header names no include directory)

#ifdef __HIPCC__
#define VQN_BRK_FN __device__ __forceinline__
#else
#include <math.h>
#define VQN_BRK_FN static inline
static inline float __fsub_rn(float a, float b) { return a - b; }
static inline float __fadd_rn(float a, float b) { return a + b; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
static inline float __fmaf_rn(float a, float b, float c) { return fmaf(a, b, c); }
#endif

#define VQN_BRK VQN_MC_BRICK_CELLS             // cells per brick and axis
#define VQN_BRK_N VQN_MC_BRICK_POINTS          // stored points per brick: 9^3, local index l = (li * 9 + lj) * 9 + lk
#define VQN_BRK_NOKEY INT64_MAX                // sort key of a slot that is not an owned point

struct BrickGrid {
  int nx, ny, nz;                              // grid points per axis (>= 2)
  int nbx, nby, nbz;                           // bricks per axis: ceil((n - 1) / 8)
};

struct BrickBox {                              // one brick along one axis
  int b;                                       // brick coordinate
  int lo;                                      // its first grid point, 8 b
  int ns;                                      // stored points 2..9: lo .. min(lo + 8, n - 1)
  int no;                                      // owned points: 8, on the last brick of the axis all ns (the grid's last point too)
};

struct Brick {
  BrickBox x, y, z;
};

VQN_BRK_FN bool brk_axis(const int b, const int n, const int nb, BrickBox* o) {
  if (b < 0 || b >= nb) return false;
  o->b = b;
  o->lo = VQN_BRK * b;
  const int hi = o->lo + VQN_BRK < n - 1 ? o->lo + VQN_BRK : n - 1;
  o->ns = hi - o->lo + 1;
  o->no = b == nb - 1 ? o->ns : VQN_BRK;
  return true;
}

// false for coordinates outside the brick grid (a caller error: such a brick is skipped, nothing of it is read or written)
VQN_BRK_FN bool brk_brick(const BrickGrid g, const int32_t* __restrict__ ijk, Brick* o) {
  const bool a = brk_axis(ijk[0], g.nx, g.nbx, &o->x), b = brk_axis(ijk[1], g.ny, g.nby, &o->y), c = brk_axis(ijk[2], g.nz, g.nbz, &o->z);
  return a && b && c;
}

VQN_BRK_FN bool brk_inside(const float v, const float thr) { return v > thr; }                       // strict; NaN is outside

// crossing of the grid edge leaving local point l = (li, lj, lk) along axis a; owned only if its far end is inside the grid, which for
// an owned point is the same as stored in this brick
VQN_BRK_FN bool brk_owned_crossing(const float* u, const Brick& k, const int l, const int li, const int lj, const int lk, const int a,
                                   const bool in0, const float thr) {
  if (a == 0) return li + 1 < k.x.ns && brk_inside(u[l + 81], thr) != in0;
  if (a == 1) return lj + 1 < k.y.ns && brk_inside(u[l + 9], thr) != in0;
  return lk + 1 < k.z.ns && brk_inside(u[l + 1], thr) != in0;
}

// case of the cell with minimum corner l (which must have one: li + 1 < ns along every axis)
VQN_BRK_FN int brk_case(const float* u, const int l, const float thr) {
  int c = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) c |= (int)brk_inside(u[l + (q & 1) * 81 + ((q >> 1) & 1) * 9 + ((q >> 2) & 1)], thr) << q;
  return c;
}

VQN_BRK_FN bool brk_owned(const Brick& k, const int li, const int lj, const int lk) { return li < k.x.no && lj < k.y.no && lk < k.z.no; }

// classify: local point l of brick k, whose 729 values are u -> owned crossing edges, triangles of its cell, the dense linear index
VQN_BRK_FN void brk_classify_point(const float* u, const BrickGrid g, const Brick& k, const int l, const float thr, int* nv, int* nt,
                                   int64_t* key) {
  const int lk = l % 9, lj = (l / 9) % 9, li = l / 81;
  *nv = 0; *nt = 0; *key = VQN_BRK_NOKEY;
  if (!brk_owned(k, li, lj, lk)) return;
  const bool in0 = brk_inside(u[l], thr);
  int n = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) n += (int)brk_owned_crossing(u, k, l, li, lj, lk, a, in0, thr);
  *nv = n;
  if (li + 1 < k.x.ns && lj + 1 < k.y.ns && lk + 1 < k.z.ns) *nt = vqn_mc_tri_count[brk_case(u, l, thr)];
  *key = ((int64_t)(k.x.lo + li) * g.ny + (k.y.lo + lj)) * g.nz + (k.z.lo + lk);
}

struct BrickOut {
  const int32_t* voff;                         // [n_bricks][729] exclusive prefix sums in the dense order
  const int32_t* toff;
  int n_verts, n_tris;
  float ox, oy, oz, stx, sty, stz;
  float* verts;
  int32_t* tris;
};

// emit: the vertices of the edges local point l of brick k (position s in the list) owns and the triangles of its cell.  u: this
// brick's values; ub: all bricks' values, slot: brick linear index -> position in the list or < 0, for edges a neighbour owns.
VQN_BRK_FN void brk_emit_point(const float* u, const float* __restrict__ ub, const int32_t* __restrict__ slot, const int n_bricks,
                               const BrickGrid g, const Brick& k, const int s, const int l, const float thr, const BrickOut o) {
  const int lk = l % 9, lj = (l / 9) % 9, li = l / 81;
  if (!brk_owned(k, li, lj, lk)) return;
  const long base = (long)s * VQN_BRK_N;
  const float u0 = u[l];
  const bool in0 = brk_inside(u0, thr);
  const int i = k.x.lo + li, j = k.y.lo + lj, kk = k.z.lo + lk;

  int rank = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const bool have = a == 0 ? li + 1 < k.x.ns : (a == 1 ? lj + 1 < k.y.ns : lk + 1 < k.z.ns);
    if (!have) continue;
    const float u1 = u[l + (a == 0 ? 81 : (a == 1 ? 9 : 1))];
    if (brk_inside(u1, thr) == in0) continue;
    const float t = __fdiv_rn(__fsub_rn(thr, u0), __fsub_rn(u1, u0));     // u1 != u0 on a crossing edge
    const int v = o.voff[base + l] + rank;
    ++rank;
    if (v < 0 || v >= o.n_verts) continue;                                  // (offsets that do not belong to this field: write nothing)
    const float px = a == 0 ? __fadd_rn((float)i, t) : (float)i;
    const float py = a == 1 ? __fadd_rn((float)j, t) : (float)j;
    const float pz = a == 2 ? __fadd_rn((float)kk, t) : (float)kk;
    o.verts[3 * (long)v + 0] = __fmaf_rn(px, o.stx, o.ox);
    o.verts[3 * (long)v + 1] = __fmaf_rn(py, o.sty, o.oy);
    o.verts[3 * (long)v + 2] = __fmaf_rn(pz, o.stz, o.oz);
  }

  if (!(li + 1 < k.x.ns && lj + 1 < k.y.ns && lk + 1 < k.z.ns)) return;
  const int c = brk_case(u, l, thr);
  const int nt = vqn_mc_tri_count[c];
  if (nt == 0) return;
  const int t0 = o.toff[base + l];
  for (int e3 = 0; e3 < 3 * nt; ++e3) {
    const int e = vqn_mc_tri_edges[c][e3];
    const int a = e >> 2, lo = e & 1, hi = (e >> 1) & 1;
    // the edge's owning point q, in this brick's local coordinates 0..8 ...
    int qi = li + (a == 0 ? 0 : lo), qj = lj + (a == 0 ? lo : (a == 1 ? 0 : hi)), qk = lk + (a == 2 ? 0 : hi);
    // ... and in its owner's: local 8 on a face that is not the grid boundary is local 0 of the next brick
    const bool nx_ = qi >= k.x.no, ny_ = qj >= k.y.no, nz_ = qk >= k.z.no;
    int id = 0;                                                             // (owner inactive: any index; the call reports the leak)
    if (!(nx_ || ny_ || nz_)) {
      const int q = (qi * 9 + qj) * 9 + qk;
      const bool inq = brk_inside(u[q], thr);
      int r = 0;
      if (a > 0) r += (int)brk_owned_crossing(u, k, q, qi, qj, qk, 0, inq, thr);
      if (a > 1) r += (int)brk_owned_crossing(u, k, q, qi, qj, qk, 1, inq, thr);
      id = o.voff[base + q] + r;
    } else {
      const int32_t nb[3] = {k.x.b + (int)nx_, k.y.b + (int)ny_, k.z.b + (int)nz_};     // inside the brick grid: no < ns only off the last brick
      Brick m;
      brk_brick(g, nb, &m);
      const int sm = slot[((long)nb[0] * g.nby + nb[1]) * g.nbz + nb[2]];
      if (sm >= 0 && sm < n_bricks) {
        if (nx_) qi = 0;
        if (ny_) qj = 0;
        if (nz_) qk = 0;
        const int q = (qi * 9 + qj) * 9 + qk;
        const float* um = ub + (long)sm * VQN_BRK_N;
        const bool inq = brk_inside(um[q], thr);
        int r = 0;
        if (a > 0) r += (int)brk_owned_crossing(um, m, q, qi, qj, qk, 0, inq, thr);
        if (a > 1) r += (int)brk_owned_crossing(um, m, q, qi, qj, qk, 1, inq, thr);
        id = o.voff[(long)sm * VQN_BRK_N + q] + r;
      }
    }
    const long w = 3 * (long)t0 + e3;
    if (t0 >= 0 && w < 3 * (long)o.n_tris) o.tris[w] = id;
  }
}
