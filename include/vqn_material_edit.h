/* vqn_material_edit.h -- material selection and editing of rows that are on the device, from libvqnerf_hip.so
 * (csrc/material_edit.hip; the program is checked and packed by csrc/material_edit_plan.h).  Same conventions as vqnerf_hip.h (device
 * pointers owned by the caller, host descriptors, `stream` a hipStream_t, negative return = error with vqn_last_error()).  The limits
 * and layout sizes stated in the comment below, as values: */
#ifndef VQN_MATERIAL_EDIT_H_
#define VQN_MATERIAL_EDIT_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_MATEDIT_MAX_PLANES 8        /* property planes at most */
#define VQN_MATEDIT_MAX_CHANNELS 3      /* channels of a plane at most */
#define VQN_MATEDIT_MAX_TERMS 32        /* terms of a program at most */
#define VQN_MATEDIT_MAX_CONDS 8         /* conditions of a program at most */
#define VQN_MATEDIT_CODES 65            /* code labels 0 .. 64 */
#define VQN_MATEDIT_HEAD_WORDS 3        /* words of `counts` ahead of the per-label counts: selected, rows, invalid */
#define VQN_MATEDIT_ROWS_PER_PASS 1024  /* rows a workgroup takes per pass */
#define VQN_MATEDIT_GRID_CAP 1024       /* workgroups at most */

/* ---- material selection and editing: pick rows by VQ code and property bounds, replace their material (csrc/material_edit.hip) ------
 * Replaces the selection rule of the reference's decomp/nerfvq_nfr3/ui4_offline.py (map_f) and the six blend statements of its
 * vq_nfr.py:325-330 for rows that are on the device: selection, edit, opt_scale scaling and counts in ONE launch over n rows.
 * planes: HOST array of 8 device pointers, float32 [n][plane_ch[p]] contiguous, plane_ch [8] HOST ints in 1 .. 3 (read for non-null
 * planes), any plane may be NULL.  embed (may be NULL): the code label of a row, int32 [n], or float32 [n] (embed_is_float != 0) rounded
 * to nearest-even as np.rint; labels 0 .. 64 are valid.  mask_in (may be NULL) uint8 [n].
 * Program (all HOST): terms_i [n_terms][4] = plane, channel, denominator channel or -1, condition id; terms_f [n_terms][2] = lo, hi;
 * n_terms <= 32; ops [n_conds - 1], 0 = 'and', 1 = 'or'; n_conds <= 8; codes: 65 bytes, non-zero = the label is in the set, or NULL
 * (no membership test).  A term holds when lo < v < hi, both strict (a NaN fails), v = plane[channel], or with a denominator
 * v = plane[channel] / (plane[denominator] + eps): one correctly rounded f32 add and one correctly rounded f32 divide.  A condition
 * holds when all of its terms hold (each condition has at least one).  m = cond_0, then m = m | cond_i or m & cond_i for i = 1 ..,
 * strictly left to right; then m &= (the row's label is valid and in the set) when codes is given (needs embed); then m &= mask_in != 0
 * when mask_in is given.  Without conditions and codes, m = mask_in != 0; without all three the call is refused.
 * mask_out (may be NULL) uint8 [n]: 0 / 1.
 * Edit (albedo_out NULL: none): albedo, spec [n][3], rough [n][1]; dst HOST [7] = diff[3], spec[3], rough[1]; a material whose FIRST
 * component is negative is left alone; otherwise a selected row takes the constant, any other row keeps its value; written to
 * albedo_out, spec_out, rough_out.  opt_scale (HOST [3], may be NULL; given together with both scaled outputs): albedo_scaled =
 * albedo_out * opt_scale and spec_scaled = spec_out * opt_scale, one rounded f32 multiply.  The selection reads its planes before the
 * edit; outputs must not overlap inputs.
 * counts: int64 [3 + 65]: selected rows, n, invalid (rows whose label is outside 0 .. 64, whenever embed is given; such rows fail the
 * membership test), then the selected rows of each label 0 .. 64 (zero when embed is NULL; an invalid row enters none).  The entry
 * zeroes the row on the stream ahead of the launch; each workgroup (1024 rows per pass, at most 1024 workgroups) reduces in LDS and
 * issues one 64-bit integer atomic per non-zero word.  No scratch, no host read.  n = 0: the row is zeroed, nothing is launched.
 * 16-byte loads and stores when every pointer is 16-byte aligned, row by row otherwise.
 * Returns -2 for n outside [0, 2^31), more than 8 conditions, more than 32 terms or a plane of more than 3 channels; -1 for a term that
 * names a null plane or a channel out of range, a condition without a term, a code set without embed, nothing that selects, or an
 * incomplete edit. */
int vqn_material_select_edit(const void* const* planes, const int32_t* plane_ch, const void* embed, int embed_is_float,
                             const uint8_t* mask_in, int64_t n, const int32_t* terms_i, const float* terms_f, int n_terms,
                             const int32_t* ops, int n_conds, const uint8_t* codes, float eps, const float* albedo, const float* spec,
                             const float* rough, const float* dst, const float* opt_scale, float* albedo_out, float* spec_out,
                             float* rough_out, float* albedo_scaled, float* spec_scaled, uint8_t* mask_out, int64_t* counts,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_MATERIAL_EDIT_H_ */
