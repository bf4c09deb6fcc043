// Material selection and editing on the device: the selection rule of the reference's decomp/nerfvq_nfr3/ui4_offline.py (map_f: box
// conditions on per-pixel properties folded left to right, the VQ code membership ANDed last), the material replacement of its
// vq_nfr.py:325-330 and the opt_scale scaling, in one pass over n rows (decomp/nerfactor/util/material_edit.py; the numpy statement is
// tests/material_edit_model.py).
//
// One kernel, matedit_kernel.  A workgroup of 256 threads takes passes of kPass = 1024 rows, kRows = 4 CONSECUTIVE rows per lane, so
// that a lane's share of a plane of ch channels is ch whole 16-byte pieces (16-byte loads and stores when every pointer is 16-byte
// aligned; the ragged last lane and unaligned tensors go row by row), passes blockIdx.x, blockIdx.x + gridDim.x, ...; the grid is
// min(kGridCap, passes), kGridCap = 1024 = 4 workgroups per CU of the 256-CU chip.  Per pass:
//   1. selection.  The program (include/vqn_material_edit.h; packed by csrc/material_edit_plan.h, its terms sorted by plane) arrives in the
//      kernel arguments and is copied into LDS once per workgroup: its terms are read at a runtime index, which LDS takes and
//      registers do not.  The planes are walked one by one (spelled out, so that the plane is a constant); a plane with terms is
//      loaded once into registers and its terms (a wave-uniform loop, each LDS word moved to a scalar register) set, per row, the bit
//      of their condition in `fail` when lo < v < hi does not hold (a NaN fails).  The channel of a term is picked with compares,
//      never by indexing: no per-thread array has a runtime index.  The conditions are then folded left to right, the membership
//      test of the code and mask_in are ANDed last.
//   2. counts.  `selected` and `invalid` are wave popcounts; the per-code counts merge equal codes across the wave before they touch
//      LDS (code images are flat: a wave usually holds one code), one LDS add per distinct code and wave.  At its end a workgroup
//      issues one 64-bit integer atomic per non-zero word to the output row, which the entry zeroes on the stream ahead of the launch.
//      Integer adds commute: equal inputs give equal counts.
//   3. edit.  albedo / spec / rough: a selected row takes the constant unless the material's first component is negative, any other row
//      keeps its value; with opt_scale the products albedo' * opt_scale and spec' * opt_scale (one rounded multiply) are written too.
//      The selection read the planes before this point, and outputs never alias inputs: it is the pre-edit selection.
#include "common.h"
#include "wave.h"
#include "material_edit_plan.h"
#include "vqn_material_edit.h"

// The only arithmetic is v / (d + eps) and x * scale.  __fadd_rn, __fdiv_rn and __fmul_rn are the plain IEEE operators here, which
// hipcc rounds correctly by default (f32 denormals on, -fhip-fp32-correctly-rounded-divide-sqrt); the Makefile passes no flag that
// relaxes them, contraction is switched off below, and a fast-math build is refused outright.
#pragma clang fp contract(off)
#if defined(__FAST_MATH__) || defined(__FINITE_MATH_ONLY__) && __FINITE_MATH_ONLY__
#error "material_edit.hip: the selection compares NaNs and needs correctly rounded IEEE arithmetic; do not build it with fast-math flags"
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kPass = VQN_MATEDIT_ROWS_PER_PASS;   // 1024 rows per workgroup pass
constexpr int kRows = kPass / kThreads;      // consecutive rows per lane and pass: 4
constexpr int kGridCap = VQN_MATEDIT_GRID_CAP;     // workgroups at most: 4 per CU of a 256-CU MI355X
static_assert(kRows * kThreads == kPass, "a pass is whole lanes");
constexpr int kHead = VQN_MATEDIT_HEAD_WORDS;      // words of the output row ahead of the per-code counts: selected, rows, invalid
constexpr int kWords = kHead + kMatCodes;
constexpr int kMinMerge = 8;                 // keep merging across the wave while a round absorbed this many lanes

// what a workgroup copies into LDS once: the program, whose terms are read at a runtime index, and the constants and the 20 tensor
// pointers of the call, which as kernel arguments overflow the scalar register file (the compiler then spills scalars into vector
// lanes); read back from LDS they live in vector registers, of which there are plenty
struct MatEditConst {
  MatEditProgram prog;
  float dst[7], scale[3];
  int apply[3];                              // the material's first component is not negative
  int pad_;
  const float* plane[kMatPlanes];
  const void* embed;                         // int32 [n] or float32 [n]
  const uint8_t* mask_in;
  const float* src[3];                       // albedo [n][3], spec [n][3], rough [n][1]
  float* out[3];
  float* scaled[2];                          // albedo' * scale, spec' * scale
  uint8_t* mask_out;
};

struct MatEditArgs {
  MatEditConst k;
  unsigned long long* counts;
  int64_t n;
  int embed_float, has_program;
};

// channel c (wave-uniform) of a row's values x0, x1, x2.  The row is passed BY VALUE: a select between two loads from an array is
// folded into one load at a selected address, which would put the array into scratch.
__device__ __forceinline__ float pick(const float x0, const float x1, const float x2, const int c) {
  return c == 2 ? x2 : c == 1 ? x1 : x0;
}
#define VQN_ROW(v, r, CH) v[(r) * CH], v[(r) * CH + (CH > 1 ? 1 : 0)], v[(r) * CH + (CH > 2 ? 2 : 0)]

template <int CH, bool VEC>
__device__ __forceinline__ void load_rows(const float* __restrict__ p, const int64_t i0, const int64_t n, const bool full, float (&v)[kRows * CH]) {
  if (VEC && full) {
    const f32x4* q = (const f32x4*)(p + i0 * CH);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const f32x4 w = q[j];
      v[4 * j] = w[0], v[4 * j + 1] = w[1], v[4 * j + 2] = w[2], v[4 * j + 3] = w[3];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kRows * CH; ++j) v[j] = i0 + j / CH < n ? p[i0 * CH + j] : 0.f;
  }
}

template <int CH, bool VEC>
__device__ __forceinline__ void store_rows(float* __restrict__ p, const int64_t i0, const int64_t n, const bool full, const float (&v)[kRows * CH]) {
  if (VEC && full) {
    f32x4* q = (f32x4*)(p + i0 * CH);
#pragma unroll
    for (int j = 0; j < CH; ++j) q[j] = f32x4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
  } else {
#pragma unroll
    for (int j = 0; j < kRows * CH; ++j)
      if (i0 + j / CH < n) p[i0 * CH + j] = v[j];
  }
}

// a value every lane reads from the same LDS word, moved to a scalar register: loops and compares on it stay wave-uniform
__device__ __forceinline__ int uni(const int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float unif(const float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// the terms t0 .. t1 - 1 of plane p: fail[r] gets the bit of a term's condition when the term does not hold on row r
template <int CH, bool VEC>
__device__ __forceinline__ void eval_plane(const MatEditArgs& a, const MatEditConst& k, const int p, const int t0, const int t1, const int64_t i0,
                                           const bool full, unsigned (&fail)[kRows]) {
  float v[kRows * CH];
  load_rows<CH, VEC>(k.plane[p], i0, a.n, full, v);
  const float eps = unif(k.prog.eps);
  for (int t = t0; t < t1; ++t) {                                            // wave-uniform
    const float lo = unif(k.prog.lo[t]), hi = unif(k.prog.hi[t]);
    const int c = uni(k.prog.ch[t]), d = uni(k.prog.den[t]);
    const unsigned bit = 1u << uni(k.prog.cond[t]);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      float x = pick(VQN_ROW(v, r, CH), c);
      if (d != kMatNoDen) x = __fdiv_rn(x, __fadd_rn(pick(VQN_ROW(v, r, CH), d), eps));
      if (!(x > lo && x < hi)) fail[r] |= bit;                               // strict on both sides; a NaN fails
    }
  }
}

template <int P, bool VEC>
__device__ __forceinline__ void plane_terms(const MatEditArgs& a, const MatEditConst& k, const int64_t i0, const bool full, unsigned (&fail)[kRows]) {
  const int word = uni((int)k.prog.plane_word[P]);                             // one scalar register per plane across the pass loop
  const int t0 = word & 255, t1 = (word >> 8) & 255, ch = word >> 16;
  if (t0 == t1) return;                                                      // no term reads this plane (a null plane never has one)
  if (ch == 3)
    eval_plane<3, VEC>(a, k, P, t0, t1, i0, full, fail);
  else if (ch == 2)
    eval_plane<2, VEC>(a, k, P, t0, t1, i0, full, fail);
  else
    eval_plane<1, VEC>(a, k, P, t0, t1, i0, full, fail);
}

template <int CH, bool VEC>
__device__ __forceinline__ void edit_rows(const MatEditArgs& a, const MatEditConst& k, const int which, const int dst0, const int64_t i0, const bool full,
                                          const bool (&sel)[kRows]) {
  if (!k.out[which]) return;
  float v[kRows * CH];
  load_rows<CH, VEC>(k.src[which], i0, a.n, full, v);
  const bool apply = k.apply[which] != 0;
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int c = 0; c < CH; ++c) v[r * CH + c] = sel[r] && apply ? k.dst[dst0 + c] : v[r * CH + c];
  store_rows<CH, VEC>(k.out[which], i0, a.n, full, v);
  if (CH == 3 && k.scaled[which < 2 ? which : 0]) {
#pragma unroll
    for (int r = 0; r < kRows; ++r)
#pragma unroll
      for (int c = 0; c < CH; ++c) v[r * CH + c] = __fmul_rn(v[r * CH + c], k.scale[c < 3 ? c : 0]);
    store_rows<CH, VEC>(k.scaled[which < 2 ? which : 0], i0, a.n, full, v);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void matedit_kernel(const MatEditArgs a) {
  __shared__ unsigned table[kWords];         // 0 selected, 1 unused, 2 invalid, 3 + c: selected rows of code c
  __shared__ MatEditConst k;
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < kWords) table[tid] = 0u;
  static_assert(sizeof(MatEditConst) % 4 == 0 && sizeof(MatEditConst) / 4 <= kThreads, "one word per thread");
  if (tid < (int)(sizeof(MatEditConst) / 4)) ((uint32_t*)&k)[tid] = ((const uint32_t*)&a.k)[tid];
  __syncthreads();
  const MatEditProgram& prog = k.prog;
  const int n_conds = uni(prog.n_conds), has_codes = uni(prog.has_codes);
  const unsigned or_bits = (unsigned)uni((int)prog.or_bits), code64 = prog.code64;
  const unsigned long long codes_lo = prog.codes_lo;         // (the code set stays in vector registers: the scalar file is full)

  const int64_t passes = (a.n + kPass - 1) / kPass;
  for (int64_t pass = blockIdx.x; pass < passes; pass += gridDim.x) {       // the same trip count for every lane of the workgroup
    const int64_t i0 = pass * kPass + (int64_t)tid * kRows;
    const bool full = i0 + kRows <= a.n;

    // ---- 1. selection ----
    unsigned fail[kRows] = {0u, 0u, 0u, 0u};
    plane_terms<0, VEC>(a, k, i0, full, fail);                             // (spelled out: the plane index must be a constant)
    plane_terms<1, VEC>(a, k, i0, full, fail);
    plane_terms<2, VEC>(a, k, i0, full, fail);
    plane_terms<3, VEC>(a, k, i0, full, fail);
    plane_terms<4, VEC>(a, k, i0, full, fail);
    plane_terms<5, VEC>(a, k, i0, full, fail);
    plane_terms<6, VEC>(a, k, i0, full, fail);
    plane_terms<7, VEC>(a, k, i0, full, fail);
    static_assert(kMatPlanes == 8, "one plane_terms per plane");
    int code[kRows] = {-1, -1, -1, -1};
    if (k.embed) {
      uint32_t w[kRows];
      if (VEC && full) {
        const uint4 x = *(const uint4*)((const uint32_t*)k.embed + i0);
        w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
      } else {
#pragma unroll
        for (int r = 0; r < kRows; ++r) w[r] = i0 + r < a.n ? ((const uint32_t*)k.embed)[i0 + r] : 0u;
      }
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (a.embed_float) {
          const float f = __builtin_rintf(__uint_as_float(w[r]));            // to nearest, ties to even, as np.rint
          code[r] = f >= 0.f && f <= 64.f ? (int)f : -1;                     // (a NaN is out of range)
        } else {
          code[r] = w[r] <= 64u ? (int)w[r] : -1;                            // negative labels wrap to large values
        }
      }
    }
    uint32_t min_bytes = 0x01010101u;
    if (k.mask_in) {
      if (VEC && full) {
        min_bytes = *(const uint32_t*)(k.mask_in + i0);
      } else {
        min_bytes = 0u;
#pragma unroll
        for (int r = 0; r < kRows; ++r)
          if (i0 + r < a.n) min_bytes |= (uint32_t)k.mask_in[i0 + r] << (8 * r);
      }
    }
    bool sel[kRows], bad[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const bool in_rows = i0 + r < a.n;
      bool m = true;
      if (n_conds > 0) {
        m = (fail[r] & 1u) == 0u;
        for (int i = 1; i < n_conds; ++i) {                           // left to right, no precedence
          const bool ci = ((fail[r] >> i) & 1u) == 0u;
          m = ((or_bits >> (i - 1)) & 1u) ? (m || ci) : (m && ci);
        }
      }
      if (has_codes) {
        const unsigned member = code[r] < 64 ? (unsigned)((codes_lo >> (code[r] & 63)) & 1ull) : code64;
        m = m && code[r] >= 0 && member != 0u;
      }
      m = m && ((min_bytes >> (8 * r)) & 255u) != 0u;                        // (all ones without mask_in)
      sel[r] = m && in_rows;
      bad[r] = k.embed != nullptr && code[r] < 0 && in_rows;
    }
    if (k.mask_out) {
      if (VEC && full) {
        *(uint32_t*)(k.mask_out + i0) = (uint32_t)sel[0] | (uint32_t)sel[1] << 8 | (uint32_t)sel[2] << 16 | (uint32_t)sel[3] << 24;
      } else {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
          if (i0 + r < a.n) k.mask_out[i0 + r] = (uint8_t)sel[r];
      }
    }

    // ---- 2. counts ----
    unsigned n_sel = 0u, n_bad = 0u;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      n_sel += (unsigned)__popcll(__ballot(sel[r]));
      n_bad += (unsigned)__popcll(__ballot(bad[r]));
    }
    if (lane == 0) {
      if (n_sel) atomicAdd(&table[0], n_sel);
      if (n_bad) atomicAdd(&table[2], n_bad);
    }
    if (k.embed) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) wave_add<kMinMerge>(table + kHead, sel[r] && code[r] >= 0, code[r], 1u, lane);
    }

    // ---- 3. edit ----
    edit_rows<3, VEC>(a, k, 0, 0, i0, full, sel);
    edit_rows<3, VEC>(a, k, 1, 3, i0, full, sel);
    edit_rows<1, VEC>(a, k, 2, 6, i0, full, sel);
  }
  __syncthreads();
  if (tid < kWords && table[tid]) atomicAdd(&a.counts[tid], (unsigned long long)table[tid]);
  if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.counts[1], (unsigned long long)a.n);
}

}  // namespace

extern "C" int vqn_material_select_edit(const void* const* planes, const int32_t* plane_ch, const void* embed, int embed_is_float,
                                        const uint8_t* mask_in, int64_t n, const int32_t* terms_i, const float* terms_f, int n_terms,
                                        const int32_t* ops, int n_conds, const uint8_t* codes, float eps, const float* albedo,
                                        const float* spec, const float* rough, const float* dst, const float* opt_scale, float* albedo_out,
                                        float* spec_out, float* rough_out, float* albedo_scaled, float* spec_scaled, uint8_t* mask_out,
                                        int64_t* counts, void* stream) {
  MatEditArgs a;
  memset(&a, 0, sizeof(a));
  VQN_CHECK_SHAPE(n >= 0 && n < ((int64_t)1 << 31), "0 <= n < 2^31 rows");
  VQN_CHECK_ARG(counts, "null counts");
  uint8_t present[kMatPlanes] = {0};
  for (int p = 0; p < kMatPlanes; ++p) {
    a.k.plane[p] = planes ? (const float*)planes[p] : nullptr;
    present[p] = a.k.plane[p] != nullptr;
  }
  char why[256];
  const int rc = matedit_pack(plane_ch, present, terms_i, terms_f, n_terms, ops, n_conds, codes, eps, &a.k.prog, why, sizeof(why));
  if (rc != 0) {
    vqn_set_error("%s: %s", __func__, why);
    return rc == -2 ? VQN_ESHAPE : VQN_EARG;
  }
  a.has_program = n_conds > 0 || codes != nullptr;
  VQN_CHECK_ARG(a.has_program || mask_in, "neither a program (conditions or codes) nor mask_in: nothing selects");
  VQN_CHECK_ARG(!codes || embed, "a code set needs embed");
  const bool edit = albedo_out || spec_out || rough_out || albedo_scaled || spec_scaled;
  if (edit) {
    VQN_CHECK_ARG(albedo && spec && rough && dst && albedo_out && spec_out && rough_out, "an edit needs albedo, spec, rough, dst and the three outputs");
    VQN_CHECK_ARG((albedo_scaled != nullptr) == (opt_scale != nullptr) && (spec_scaled != nullptr) == (opt_scale != nullptr),
                  "opt_scale and the two scaled outputs are given together or not at all");
    a.k.src[0] = albedo, a.k.src[1] = spec, a.k.src[2] = rough;
    a.k.out[0] = albedo_out, a.k.out[1] = spec_out, a.k.out[2] = rough_out;
    a.k.scaled[0] = albedo_scaled, a.k.scaled[1] = spec_scaled;
    for (int i = 0; i < 7; ++i) a.k.dst[i] = dst[i];
    a.k.apply[0] = !(dst[0] < 0.f), a.k.apply[1] = !(dst[3] < 0.f), a.k.apply[2] = !(dst[6] < 0.f);
    for (int i = 0; i < 3; ++i) a.k.scale[i] = opt_scale ? opt_scale[i] : 1.f;
  }
  a.k.embed = embed, a.embed_float = embed_is_float, a.k.mask_in = mask_in, a.k.mask_out = mask_out, a.n = n;
  a.counts = (unsigned long long*)counts;
  VQN_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * kWords, (hipStream_t)stream));
  if (n == 0) return VQN_OK;
  uintptr_t bits = (uintptr_t)embed | (uintptr_t)mask_in | (uintptr_t)mask_out;
  for (int p = 0; p < kMatPlanes; ++p)
    if (a.k.prog.begin[p] != a.k.prog.begin[p + 1]) bits |= (uintptr_t)a.k.plane[p];
  for (int i = 0; i < 3; ++i) bits |= (uintptr_t)a.k.src[i] | (uintptr_t)a.k.out[i] | (uintptr_t)a.k.scaled[i < 2 ? i : 0];
  const int64_t passes = (n + kPass - 1) / kPass;
  const unsigned blocks = (unsigned)(passes < kGridCap ? passes : kGridCap);
  if ((bits & 15u) == 0u)
    hipLaunchKernelGGL((matedit_kernel<true>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((matedit_kernel<false>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
  VQN_LAUNCH_CHECK();
  return VQN_OK;
}
