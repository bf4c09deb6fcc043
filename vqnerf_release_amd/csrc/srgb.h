// The display transfer of a linear value (nerfactor/util/img.py:142-186: clip to [0, 1], then the piecewise sRGB curve), stated once for
// the kernels that apply it (vqn_linear2srgb in brdf_shade.hip, the 8-bit outputs of material_balls.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float vqn_srgb_curve(const float v) {
  const float t = fminf(fmaxf(v, 0.0f), 1.0f);         // fminf / fmaxf drop a NaN: put it back, as the clip of the statement does
  const float r = t <= 0.0031308f ? t * 12.92f : 1.055f * powf(t, 1.0f / 2.4f) - (1.055f - 1.0f);
  return (v != v) ? v : r;
}
