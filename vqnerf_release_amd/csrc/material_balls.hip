// Material balls for gfx950: M materials x P light probes as lit spheres, finished images out (include/vqn_material_balls.h; the host
// side is csrc/material_balls_plan.h, the float64 statement tests/material_balls_model.py).  Replaces the reference's
// decomp/nerfvq_nfr3/brdf/renderer.py SphereRenderer (numpy, one BRDF at a time) with the shading of csrc/brdf_shade.hip.
//
// The sum a pixel needs is, per sample, over (material m, light l, probe p, channel c).  What depends on (sample, light) only -- light
// direction, half vector, cos_l, the Schlick term, the front-lit test -- is shared by all materials; what depends on the material is
// D G1(l) per (m, l) and seven constants.  The per-point kernel (one wave per point and material, lights across the lanes) cannot
// share the first and pays a 64-lane reduction per output value.  Here:
//   * one 64-lane wave (a workgroup of its own) renders one pixel: its spp samples in turn, all materials, all probes;
//   * phase 1, lanes = lights: every lane takes L / 64 lights and computes the shared per-light values.  Lights that are not front-lit
//     contribute an exact 0 to every sum, so only the front-lit ones are kept: a ballot and a prefix count compact them, in ascending
//     light index, into a list in LDS (four floats and the light's index each).  About half of the lights of a probe drop out here;
//   * phase 2, lanes = MATERIALS: lane m holds material m's constants.  The wave walks the list; an entry is one LDS broadcast read,
//     the light's row of the probe table (3 P radiances, the table transposed to [L][3 P] by a first small launch so that a row is
//     contiguous) is read at a wave-uniform address, i.e. by scalar loads into scalar registers.  Per light a lane does the ~25
//     instructions of D G1 F (one sqrt, two reciprocals) once and then 3 P fused multiply-adds, as ceil(3 P / 2) packed ones, into
//     accumulators of its own: no value of the sum ever crosses lanes, there is no reduction;
//   * sums run over 32 lights into a block sum and the block sums into the total (two-level: the rounding error of a 500-term f32
//     running sum would otherwise be the largest error of the kernel), then gamma, clip, and the average over the pixel's samples;
//   * lane m writes its 3 P values of the pixel to the float image, the 8-bit image and its cell of the sheet.  M = 65 takes a second
//     pass for the one material beyond the wave; more than 17 probes take two launches (material_balls_plan.h: three accumulator
//     sets of 36 pairs would spill).
// Nothing of size [samples][materials] exists in memory.  VALU only: see DESIGN.md section 15 for why the matrix engine is not used.
#include "common.h"
#include "launch.h"
#include "srgb.h"
#include "material_balls_plan.h"
#include "vqn_material_balls.h"

namespace {

constexpr float PI_F = 3.14159265358979323846f;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float div_no_nan(float a, float b) { return b == 0.f ? 0.f : a / b; }
__device__ __forceinline__ float inv_norm(float x, float y, float z) { return __builtin_amdgcn_rsqf(fmaxf(x * x + y * y + z * z, 1e-6f)); }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }

struct BallsArgs {
  const float *materials, *lxyz, *areas;
  int M, P, L, ims, sps;
  int p0, n_p, stride;                           // this launch: probes p0 .. p0 + n_p - 1, floats of a row of its table
  float a, step, radius, r2, inv_spp;
  float rot[9], cam[3];
  float gamma_b, gamma_i;
  int has_gamma, white_bg;
  int rows, cols;
  uint32_t cell_words[(kBallsMaxM + 3) / 4];     // BallsPlan::cell_of, four materials to a word
};

// lights [P][L][3] -> table [L][stride]: row l = the 3 P radiances of light l, zero padded
__global__ __launch_bounds__(256) void balls_table_kernel(const float* __restrict__ lights, const int P, const int L, const int stride,
                                                          float* __restrict__ table) {     // (lights: at the launch's first probe)
  const int n = L * stride;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int l = i / stride, k = i - l * stride;
    table[i] = k < 3 * P ? lights[((size_t)(k / 3) * L + l) * 3 + k % 3] : 0.f;
  }
}

// coordinate i of the sample grid: one rounded operation each, as the header states them
__device__ __forceinline__ float grid_coord(const BallsArgs& g, const int i) {
  return __fdiv_rn(__fadd_rn(g.a, __fmul_rn((float)i, g.step)), (float)g.ims);
}

template <int NP>
__global__ __launch_bounds__(64) void balls_kernel(const BallsArgs g, const float* __restrict__ table, float* __restrict__ out_f32,
                                                   uint8_t* __restrict__ out_u8, uint8_t* __restrict__ sheet) {
  extern __shared__ __attribute__((aligned(16))) f32x4 lit[];            // [L] {cos_l * area, (1 - h.v)^5, (h.n)^2, clip(l.n)}
  int* const lit_idx = reinterpret_cast<int*>(lit + g.L);                // [L] the light's index
  const int lane = threadIdx.x;
  const int y = blockIdx.x / g.ims, x = blockIdx.x - y * g.ims;
  const float bg = g.white_bg ? 1.f : 0.f;
  const int n_val = 3 * g.n_p;

  for (int m0 = 0; m0 < g.M; m0 += 64) {
    const int mi = m0 + lane;
    const bool has_m = mi < g.M;
    const float* mat = g.materials + (size_t)(has_m ? mi : 0) * VQN_MATBALLS_MATERIAL_FLOATS;
    float ma[3], f0[3], omf0[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ma[c] = mat[c] * (1.f / PI_F);
      f0[c] = mat[3 + c];
      omf0[c] = 1.f - f0[c];
    }
    const float rough = mat[6];
    const float alpha = rough * rough;
    const float a2 = alpha * alpha, a2_pi = a2 * (1.f / PI_F), oma2 = 1.f - a2;

    f32x2 pix[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) pix[k] = (f32x2){0.f, 0.f};

    for (int sj = 0; sj < g.sps; ++sj)
      for (int si = 0; si < g.sps; ++si) {
        const float dx = __fsub_rn(grid_coord(g, x * g.sps + si), 0.5f), dy = __fsub_rn(grid_coord(g, y * g.sps + sj), 0.5f);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
        if (!(__fsqrt_rn(d2) <= g.radius)) {                             // background sample (wave-uniform)
#pragma unroll
          for (int k = 0; k < NP; ++k) pix[k] += (f32x2){bg, bg};
          continue;
        }
        // ---- the sample's point, normal and view direction: the per-point part of brdf_shade_kernel on xyz = p, rayo = camera ----
        const float hz = sqrtf(fmaxf(g.r2 - d2, 0.f)), cy = -dy;
        const float px = fmaf(g.rot[2], hz, fmaf(g.rot[1], cy, g.rot[0] * dx));
        const float py = fmaf(g.rot[5], hz, fmaf(g.rot[4], cy, g.rot[3] * dx));
        const float pz = fmaf(g.rot[8], hz, fmaf(g.rot[7], cy, g.rot[6] * dx));
        const float ip = inv_norm(px, py, pz);
        float nx = px * ip, ny = py * ip, nz = pz * ip;
        float vx = g.cam[0] - px, vy = g.cam[1] - py, vz = g.cam[2] - pz;
        float iv = inv_norm(vx, vy, vz);
        vx *= iv; vy *= iv; vz *= iv;
        if (nx * vx + ny * vy + nz * vz < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
        iv = inv_norm(vx, vy, vz);
        const float ux = vx * iv, uy = vy * iv, uz = vz * iv;
        const float in_ = inv_norm(nx, ny, nz);
        const float mx = nx * in_, my = ny * in_, mz = nz * in_;
        const float v_dot_n = ux * mx + uy * my + uz * mz;
        const float cv = clip01(v_dot_n);
        const float g1v = div_no_nan(2.f * cv, cv + sqrtf(fabsf(a2 + oma2 * cv * cv)));
        const float kv = div_no_nan(g1v, 2.f * fabsf(v_dot_n));

        // ---- phase 1: lanes = lights.  The shared per-light values of the front-lit lights, compacted in ascending index ----
        __syncthreads();                                                 // (the list of the previous sample has been read)
        int n_lit = 0;
        for (int l0 = 0; l0 < g.L; l0 += 64) {
          const int l = l0 + lane;
          float ex = g.lxyz[l * 3] - px, ey = g.lxyz[l * 3 + 1] - py, ez = g.lxyz[l * 3 + 2] - pz;
          const float il = inv_norm(ex, ey, ez);
          ex *= il; ey *= il; ez *= il;
          const float cosl = dot3(ex, ey, ez, nx, ny, nz);
          const float l_dot_n = dot3(ex, ey, ez, mx, my, mz);
          const bool front = cosl > 0.f && l_dot_n > 0.f;
          float hx = ex + ux, hy = ey + uy, hh = ez + uz;
          const float ih = inv_norm(hx, hy, hh);
          hx *= ih; hy *= ih; hh *= ih;
          const float om = 1.f - clip01(dot3(hx, hy, hh, ux, uy, uz)), om2 = om * om;
          const float cos_m = clip01(dot3(hx, hy, hh, mx, my, mz));
          const unsigned long long ball = __ballot(front);
          const int at = n_lit + __builtin_amdgcn_mbcnt_hi((unsigned)(ball >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ball, 0u));
          if (front) {                                                   // at < L: at most one entry per light
            lit[at] = (f32x4){cosl * g.areas[l], om2 * om2 * om, cos_m * cos_m, clip01(l_dot_n)};
            lit_idx[at] = l;
          }
          n_lit += __popcll(ball);
        }
        __syncthreads();

        // ---- phase 2: lanes = materials ----
        f32x2 tot[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) tot[k] = (f32x2){0.f, 0.f};
        for (int j0 = 0; j0 < n_lit; j0 += kBallsSumBlock) {
          f32x2 acc[NP];
#pragma unroll
          for (int k = 0; k < NP; ++k) acc[k] = (f32x2){0.f, 0.f};
          const int j1 = min(j0 + kBallsSumBlock, n_lit);
          for (int j = j0; j < j1; ++j) {
            const f32x4 q = lit[j];                                      // one address for the wave: a broadcast read
            const int l = __builtin_amdgcn_readfirstlane(lit_idx[j]);
            const f32x2* __restrict__ row = reinterpret_cast<const f32x2*>(table + (size_t)l * g.stride);   // wave-uniform: scalar loads
            const float gw = q[0], om5 = q[1], cm2 = q[2], cl = q[3];
            const float t = fmaf(cm2, -oma2, 1.f);                       // cos_m^2 (a2 - 1) + 1
            const float D = a2_pi * __builtin_amdgcn_rcpf(fmaxf(t * t, 1e-30f));
            const float sl = __builtin_amdgcn_sqrtf(fabsf(fmaf(oma2, cl * cl, a2)));
            const float gdi = D * kv * __builtin_amdgcn_rcpf(fmaxf(cl + sl, 1e-30f));
            const float p0 = (fmaf(omf0[0], om5, f0[0]) * gdi + ma[0]) * gw, p1 = (fmaf(omf0[1], om5, f0[1]) * gdi + ma[1]) * gw,
                        p2 = (fmaf(omf0[2], om5, f0[2]) * gdi + ma[2]) * gw;
            const f32x2 pp[3] = {{p0, p1}, {p2, p0}, {p1, p2}};          // values 2 k, 2 k + 1 are channels (2 k) % 3, (2 k + 1) % 3
#pragma unroll
            for (int k = 0; k < NP; ++k) acc[k] = __builtin_elementwise_fma(pp[k % 3], row[k], acc[k]);
          }
#pragma unroll
          for (int k = 0; k < NP; ++k) tot[k] += acc[k];
        }
#pragma unroll
        for (int k = 0; k < NP; ++k)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            float t = tot[k][e];
            if (g.has_gamma) t = powf(t * g.gamma_b, g.gamma_i);
            pix[k][e] += clip01(t);
          }
      }

    // ---- the pixel of material `mi` under every probe ----
    if (has_m) {
      const uint32_t word = [&] {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < (kBallsMaxM + 3) / 4; ++i) w = (mi >> 2) == i ? g.cell_words[i] : w;
        return w;
      }();
      const int cell = (int)((word >> (8 * (mi & 3))) & 255u);
      const size_t sheet_w = (size_t)g.cols * g.ims;
      const size_t sheet_at = cell == kBallsNoCell ? 0 : ((size_t)(cell / g.cols) * g.ims + y) * sheet_w + (size_t)(cell % g.cols) * g.ims + x;
#pragma unroll
      for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int v = 2 * k + e;
          if (v < n_val) {
            const int p = v / 3, c = v - 3 * p;
            const float val = pix[k][e] * g.inv_spp;
            const size_t at = ((((size_t)mi * g.P + g.p0 + p) * g.ims + y) * g.ims + x) * 3 + c;
            if (out_f32) out_f32[at] = val;
            const uint8_t byte = (uint8_t)(fminf(fmaxf(vqn_srgb_curve(val), 0.f), 1.f) * 255.0f);
            if (out_u8) out_u8[at] = byte;
            if (sheet && cell != kBallsNoCell) sheet[((size_t)(g.p0 + p) * g.rows * g.ims * sheet_w + sheet_at) * 3 + c] = byte;
          }
        }
    }
  }
}

}  // namespace

extern "C" int vqn_material_balls(const float* materials, int n_materials, const float* lights, int n_probes, const float* lxyz,
                                  const float* areas, int n_lights, int ims, int spp, float sphere_radius, const float* cam_rot, int white_bg,
                                  const float* gamma, float* out_f32, uint8_t* out_u8, uint8_t* sheet, const int32_t* order, int n_order,
                                  int sheet_rows, int sheet_cols, void* scratch, int64_t scratch_bytes, void* stream) {
  BallsPlan plan;
  char why[256];
  const int rc = balls_plan(n_materials, n_probes, n_lights, ims, spp, sphere_radius, cam_rot, white_bg, gamma,
                            materials && lights && lxyz && areas, out_f32 != nullptr, out_u8 != nullptr, sheet != nullptr, order, n_order,
                            sheet_rows, sheet_cols, scratch != nullptr, ((uintptr_t)scratch & 15) == 0, scratch_bytes, &plan, why, sizeof(why));
  if (rc != 0) {
    vqn_set_error("%s: %s", __func__, why);
    return rc;
  }
  BallsArgs a;
  memset(&a, 0, sizeof(a));
  a.materials = materials; a.lxyz = lxyz; a.areas = areas;
  a.M = plan.M; a.P = plan.P; a.L = plan.L; a.ims = plan.ims; a.sps = plan.sps;
  a.a = plan.a; a.step = plan.step; a.radius = plan.radius; a.r2 = plan.r2; a.inv_spp = plan.inv_spp;
  memcpy(a.rot, plan.rot, sizeof(a.rot));
  memcpy(a.cam, plan.cam, sizeof(a.cam));
  a.gamma_b = plan.gamma[0]; a.gamma_i = plan.gamma[1]; a.has_gamma = plan.has_gamma; a.white_bg = plan.white_bg;
  a.rows = plan.rows; a.cols = plan.cols;
  for (int m = 0; m < kBallsMaxM; ++m) a.cell_words[m >> 2] |= (uint32_t)(sheet ? plan.cell_of[m] : kBallsNoCell) << (8 * (m & 3));
  const char* fn = __func__;
  // cells that show no ball keep the background: 255 is the byte of 1.0, 0 of 0.0
  if (sheet) VQN_HIP(hipMemsetAsync(sheet, plan.white_bg ? 255 : 0, (size_t)plan.sheet_bytes, (hipStream_t)stream));
  for (int i = 0; i < plan.n_chunks; ++i) {                          // more than 17 probes: the first 12, then the rest
    const BallsChunk& ch = plan.chunk[i];
    float* const table = static_cast<float*>(scratch) + ch.table_at;
    a.p0 = ch.p0; a.n_p = ch.n_p; a.stride = 2 * ch.pairs;
    int rc_l = vqn_launch(fn, balls_table_kernel, dim3((unsigned)((plan.L * a.stride + 255) / 256)), 256, 0, stream,
                          lights + (size_t)ch.p0 * plan.L * 3, ch.n_p, plan.L, a.stride, table);
    if (rc_l != VQN_OK) return rc_l;
    rc_l = vqn_pick<kBallsPairs[0], kBallsPairs[1], kBallsPairs[2], kBallsPairs[3], kBallsPairs[4]>(fn, ch.pairs, [&](auto np) {
      return vqn_launch(fn, balls_kernel<decltype(np)::value>, dim3((unsigned)plan.grid), 64, (size_t)plan.lds_bytes, stream, a,
                        static_cast<const float*>(table), out_f32, out_u8, sheet);
    });
    if (rc_l != VQN_OK) return rc_l;
  }
  return VQN_OK;
}
