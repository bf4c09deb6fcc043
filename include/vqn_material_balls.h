/* vqn_material_balls.h -- every material of a list as a lit sphere under every light probe of a list, from libvqnerf_hip.so
 * (csrc/material_balls.hip; sizes, sheet geometry and refusals by csrc/material_balls_plan.h).  Same conventions as vqnerf_hip.h (device
 * pointers owned by the caller, host descriptors, `stream` a hipStream_t, negative return = error with vqn_last_error(), a refused call
 * launches nothing).  The limits and layout sizes stated in the comment below, as values: */
#ifndef VQN_MATERIAL_BALLS_H_
#define VQN_MATERIAL_BALLS_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_MATBALLS_MAX_MATERIALS 65     /* materials at most: 64 codes and one row of the caller's */
#define VQN_MATBALLS_MAX_PROBES 24        /* light probes at most (the shading kernel's limit) */
#define VQN_MATBALLS_LIGHT_STEP 64        /* L is a multiple of this ... */
#define VQN_MATBALLS_MAX_LIGHTS 1024      /* ... and at most this */
#define VQN_MATBALLS_MAX_IMS 1024         /* side of a ball image at most */
#define VQN_MATBALLS_MAX_SPS 4            /* samples per side of a pixel at most: spp = 1, 4, 9, 16 */
#define VQN_MATBALLS_MATERIAL_FLOATS 7    /* floats of a material row: albedo[3], f0[3], rough[1] */
#define VQN_MATBALLS_SCRATCH_PER_LIGHT 288 /* bytes of scratch per light that always suffice (72 floats: 24 probes) */
#define VQN_MATBALLS_SUM_BLOCK 32         /* lights whose terms are summed before they join a pixel's running total */
#define VQN_MATBALLS_MAX_OUT_BYTES 0x7fffffff  /* bytes of each output buffer at most: element offsets are 32-bit */

/* ---- material balls: M materials x P probes as lit spheres, the reference's brdf/renderer.py SphereRenderer on the device -----------
 * materials float32 [M][7] = albedo[3], f0[3], rough[1] (the three arguments of get_brdf); lights float32 [P][L][3]; lxyz [L][3] and
 * areas [L] as gen_light_xyz gives them (all device).  M in 1 .. 65, P in 1 .. 24, L a multiple of 64 up to 1024, ims in 1 .. 1024,
 * spp in {1, 4, 9, 16}.
 * Sample grid (the reference's _gen_scene): sps = sqrt(spp), n = ims * sps samples per axis, a = 1 / (sps + 1),
 * step = (ims - 2 a) / (n - 1) (0 when n = 1), coordinate i is u_i = (a + i * step) / ims; every operation one correctly rounded f32
 * operation, in this order.  Sample (row j, column i) lies at (u_i, u_j); with dx = u_i - 0.5, dy = u_j - 0.5 and
 * d2 = dx * dx + dy * dy (f32, no fused multiply-add) it is foreground iff sqrt(d2) <= sphere_radius (f32 square root).
 * Surface point: the sphere point above the sample, an orthographic lift: p_cam = (dx, -dy, sqrt(max(radius^2 - d2, 0))) in the camera
 * frame (+x right, +y up, +z from the ball toward the camera; image row 0 is the top; radius^2 and the subtraction are f32
 * operations on the d2 above, so the root's argument is the same number for every implementation).  The reference back-projects through a
 * perspective camera instead and gets points close to, not on, the sphere; that is not copied.  cam_rot (HOST [9], row major; NULL =
 * the default) takes the camera frame to the frame of the lights: p = cam_rot p_cam, the camera stands at cam_rot (0, 0, 10).  The
 * default is rows (1, 0, 0), (0, 0, -1), (0, 1, 0): the camera stands on -Y and looks along +Y with +Z up and +X to the right, so the
 * top of the ball is lit by the top rows of the probe.  Normal: p normalised; view direction: normalize(camera - p); both by
 * x * rsqrt(max(|x|^2, 1e-6)) as everywhere in the shading code; the normal is turned toward the camera where normal . view < 0, as
 * the shading kernel turns it (at distance 10 that is the rim ring with sqrt(radius^2 - d2) < radius^2 / 10).  Light directions:
 * normalize(lxyz - p).
 * Shading: the op sequence of vqn_brdf_shade_fwd without a visibility row (front-lit lights only; divide_no_nan; the sum over L), then
 * (rgb * gamma[0]) ^ gamma[1] when gamma (HOST [2]) is given (NULL: none), then the clip to [0, 1].  A background sample is 1
 * (white_bg != 0) or 0.  The spp samples of a pixel are averaged after the clip: summed row by row, column by column within the pixel,
 * then multiplied by the f32 1 / spp.
 * Outputs (device, any may be NULL, not all): out_f32 float32 [M][P][ims][ims][3] linear; out_u8 uint8 [M][P][ims][ims][3]: the
 * piecewise sRGB curve of vqn_linear2srgb on out_f32's value, times 255, truncated; sheet uint8 [P][rows * ims][cols * ims][3]: the
 * same bytes tiled, cell (i / cols, i % cols) shows material order[i] (order: HOST int32 [n_order], NULL = 0 .. M - 1 with n_order = M;
 * distinct entries in 0 .. M - 1; n_order <= rows * cols; rows, cols <= 65), cells past n_order take the background.  Each output
 * holds at most 2^31 - 1 bytes.
 * Sum over L: the front-lit lights in ascending index, 32 at a time into a block sum, the block sums into the total in order.
 * scratch: device, 16-byte aligned, at least 4 * L * s(P) bytes, s(P) the smallest of 4, 12, 24, 36, 52 that is >= 3 P up to 17
 * probes and 36 + s(P - 12) beyond (288 L always suffices): the probe table as the kernel reads it, [L][s], written by a small launch
 * on the stream ahead of the kernel.  More than 17 probes are rendered in two launches, the first 12 and the rest.
 * Returns -2 for M, P, L, ims, spp or an output size outside the limits; -1 for a null input, no output at all, a sheet with too few
 * cells or an order entry out of range, a radius outside (0, 0.5], or a scratch that is NULL, misaligned or too small. */
int vqn_material_balls(const float* materials, int n_materials, const float* lights, int n_probes, const float* lxyz,
                       const float* areas, int n_lights, int ims, int spp, float sphere_radius, const float* cam_rot, int white_bg,
                       const float* gamma, float* out_f32, uint8_t* out_u8, uint8_t* sheet, const int32_t* order, int n_order,
                       int sheet_rows, int sheet_cols, void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_MATERIAL_BALLS_H_ */
