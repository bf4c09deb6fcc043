/* vqn_neus_fold.h -- the folded colour pack of the f32 NeuS inference path (csrc/neus_fold.hip), one entry point of libvqnerf_hip.so.
 * include/vqnerf_hip.h declares the library's first 91 functions and that list is held fixed; everything added since has a header
 * per area beside it: this one, vqn_mesh.h, vqn_eval.h, vqn_material_edit.h, vqn_image_codec.h.  Same conventions as vqnerf_hip.h
 * (device pointers owned by the caller, host descriptors, `stream` a hipStream_t, negative return = error with vqn_last_error()). */
#ifndef VQN_NEUS_FOLD_H_
#define VQN_NEUS_FOLD_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Folded colour pack of the f32 inference path.  The last SDF layer's feature rows carry no activation (fields.py:84-91) and the
 * first colour layer is linear in them (fields.py:147-166), so  Wc0[:, feat] . (W8f . h + b8f) + bc0 = Wfold . h + bfold  with
 * Wfold = Wc0[:, feat] . W8f and bfold = bc0 + Wc0[:, feat] . b8f: vqn_neus_fine_points then runs one K = hidden GEMM where it ran the
 * feature layer and a K = extras GEMM where it ran colour layer 0 over K = features + extras.  This call builds, in one launch,
 * wbuf_out = [the colour pack wbuf_col (col_floats floats), verbatim | Wfold as a forward pack | bfold as a bias pack |
 * Wc0[:, extras] as a forward pack] (float64 accumulation, one rounding to f32) and col_desc_out = col_desc with the float4
 * offsets of the three blocks in ColDesc::reserved1..3 (include/vqn_neus_desc.h; 0 = not folded).  Pass both to
 * vqn_neus_fine_points in place of (col_desc, wbuf_col): out_sdf and out_grad are bit-identical, out_rgb moves by re-association
 * only.  The training forward and the *_f16s / *_x3 entry points take the unfolded pair.  Inputs are the EFFECTIVE weights the packs
 * were gathered from (device, row-major): sdf_w_last [1 + d_feature, sdf_hidden] and sdf_b_last [1 + d_feature] (row 0 = the sdf
 * output), col_w0 [col_hidden, extras + d_feature] and col_b0 [col_hidden] (input order [pts, view, normal, features]).
 * Returns the float count of wbuf_out (nothing is launched when wbuf_out is NULL or out_floats is smaller: a size query;
 * col_desc_out, if given, is written either way) or a negative error code.  Rebuild whenever the packs are rebuilt. */
int64_t vqn_neus_fold_pack(const int32_t* sdf_desc, const int32_t* col_desc, const float* wbuf_col, int64_t col_floats,
                           const float* sdf_w_last, const float* sdf_b_last, int sdf_hidden, int d_feature, const float* col_w0,
                           const float* col_b0, int col_hidden, float* wbuf_out, int64_t out_floats, int32_t* col_desc_out,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_NEUS_FOLD_H_ */
