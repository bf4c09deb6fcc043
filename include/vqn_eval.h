/* vqn_eval.h -- evaluation of results that are on the device, from libvqnerf_hip.so: image metrics (csrc/image_metrics.hip),
 * segmentation scores (csrc/segmentation_metrics.hip) and the mean-shift baseline of the segmentation table (csrc/meanshift.hip).
 * Same conventions as vqnerf_hip.h (device pointers owned by the caller, host descriptors, `stream` a hipStream_t, negative return =
 * error with vqn_last_error()).  The limits and layout sizes stated in the comments below, as values: */
#ifndef VQN_EVAL_H_
#define VQN_EVAL_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_IMAGE_METRICS_WINDOW 11        /* weights of the SSIM window */
#define VQN_IMAGE_METRICS_OUT_WORDS 16     /* 8-byte words of `out` per image pair */

#define VQN_SEG_MAX_SIDE 65                /* table sides R = n_gt + 1, C = n_pd + 1 at most */
#define VQN_SEG_HEAD_WORDS 42              /* 8-byte words of `out` ahead of the table */
#define VQN_SEG_PIXELS_PER_PASS 4096       /* pixels a workgroup takes per pass */
#define VQN_SEG_GRID_CAP 512               /* workgroups at most */

#define VQN_MEANSHIFT_MAX_DIM 8            /* features per point at most */
#define VQN_MEANSHIFT_POINTS_PER_TILE 256  /* points of a seek pass: the period of the neighbour sum's order */
#define VQN_MEANSHIFT_SEEDS_PER_GROUP 64   /* seeds a seek workgroup owns */
#define VQN_MEANSHIFT_ASSIGN_SPAN 256      /* points an assign workgroup labels per pass */
#define VQN_MEANSHIFT_ASSIGN_CENTRES 512   /* centres the assign kernel holds at a time */

/* ---- image metrics: PSNR, MSE, SSIM and their luma forms of B image pairs (csrc/image_metrics.hip) ---------------------------------
 * Replaces xiuminglib/metric.py (PSNR, PSNR_luma, SSIM, SSIM_luma, MSE; third party of the reference, its SSIM is tf.image.ssim) for
 * images that are already on the device.  a, b [B][H][W][C], C in {1, 3}: uint8 (_u8), or float32 rows in [0, 1] (_f32) that the
 * kernel quantises as the writer does, (uint8)(clip(x, 0, 1) * 255) in f32.  alpha (may be NULL): f32 plane(s) [H][W], pair i reads
 * alpha + i * alpha_stride (alpha_stride 0: one plane for all pairs, else H * W); every pixel that is NOT alpha > alpha_thres
 * (strict) becomes white in both images before scoring, the evaluator's standard background (metric_eval.py:735-744).
 * SSIM as tf.image.ssim with its defaults: window [11] = the normalised 1-D Gaussian (sigma 1.5) as HOST doubles, applied as its
 * outer product over the (H - 10)(W - 10) 'VALID' positions; c1 = (0.01 * 255)^2, c2 = (0.03 * 255)^2;
 *   luminance = (2 mx my + c1) / (mx^2 + my^2 + c1),  cs = (2 conv(xy) - 2 mx my + c2) / (conv(x^2 + y^2) - mx^2 - my^2 + c2),
 * a channel's score = mean of luminance * cs, the image's = mean over channels.  Luma = 0.2126 R + 0.7152 G + 0.0722 B
 * (xiuminglib/img.py:597-611) of the bytes, unrounded; for C = 1 it is the channel.  All sums and moments are float64.
 * out [B][16] 8-byte words per pair: 0..4 float64 psnr = 10 log10(255^2 / mse) (inf for mse = 0), mse (mean squared 8-bit
 * difference over pixels and channels, from the exact integer sum), psnr_luma, ssim, ssim_luma; 5..9 float64 the SSIM sums of R, G,
 * B and luma and the luma squared error; 10..14 int64 the squared-difference sums of R, G, B, H * W and (H - 10)(W - 10); 15 zero.
 * scratch: vqn_image_metrics_scratch_bytes(B, H, W) bytes (64 per 32 x 32 tile of positions; 0 for a shape the calls refuse); the
 * per-tile sums are added in a fixed order, without atomics: equal inputs give equal bits.  Two launches.  Returns -2 for
 * H < 11 or W < 11 (nothing is launched), C not in {1, 3}, B > 65535; -1 for null pointers or a scratch that is too small; B = 0 is
 * a no-op. */
int64_t vqn_image_metrics_scratch_bytes(int64_t B, int H, int W);
int vqn_image_metrics_u8(const uint8_t* a, const uint8_t* b, const float* alpha, int64_t alpha_stride, float alpha_thres, int64_t B,
                         int H, int W, int C, const double* window, void* scratch, int64_t scratch_bytes, void* out, void* stream);
int vqn_image_metrics_f32(const float* a, const float* b, const float* alpha, int64_t alpha_stride, float alpha_thres, int64_t B,
                          int H, int W, int C, const double* window, void* scratch, int64_t scratch_bytes, void* out, void* stream);

/* ---- segmentation scores: contingency table of two label images and the clustering scores (csrc/segmentation_metrics.hip) ---------
 * Replaces the reference's decomp/nerfvq_nfr3/cluster_eval.py (img_embed, correspond, purity and sklearn's f1_score /
 * precision_score / recall_score) for pixels that are on the device.  n pixels, the views of a scene flattened and concatenated;
 * coo[g][p] = counted pixels with ground-truth label g and predicted label p, R = n_gt + 1 rows, C = n_pd + 1 columns, R, C <= 65.
 * _rgb: gt_rgb, pd_rgb uint8 [n][3]; gt_palette [n_gt][3], pd_palette [n_pd][3] HOST bytes; a pixel's label is 1 + the index of the
 * first palette row it equals exactly, 0 when it equals none (class 0 takes part); alpha (may be NULL) f32 [n]: a pixel is counted
 * when alpha > alpha_thres (strict).  _labels: gt, pd int32 [n] with labels in [0, n_gt] and [0, n_pd]; mask (may be NULL) uint8
 * [n]: a pixel is counted when its byte is not 0; a counted pixel with a label outside its range is left out of the table and
 * added to `invalid`.
 * out: (42 + R * C) 8-byte words: 0..4 float64 purity, f1_micro, f1_macro, p_macro, r_macro; 5..8 int64 total (the table's sum),
 * invalid, the number of present rows, the number of present columns (present = non-zero sum); 9..41 int32 label_map[65] plus one
 * zero word of padding: label_map[p] = the row with the largest count in column p, ties to the lowest row, -1 for an absent column
 * and for p >= C; 42.. int64 coo[R][C].
 * Scores (float64, fixed order): purity = sum_p max_g coo[g][p] / total; with M[g][g'] = the sum of coo[g][p] over p with
 * label_map[p] = g', per present row g: tp = M[g][g], pred = sum_r M[r][g], true = sum_c M[g][c], precision = tp / pred (0 when
 * pred = 0), recall = tp / true, f1 = 2 tp / (2 tp + (pred - tp) + (true - tp)); the macro scores are the sums over present rows in
 * ascending order divided by their number; f1_micro = sum tp / total.  total = 0: the five scores are NaN.
 * scratch: vqn_seg_scratch_bytes(n, R, C) bytes (one table of R * C + 1 32-bit words per workgroup, at most 512 workgroups of 4096
 * pixels per pass; 0 for a shape the calls refuse).  No atomics across workgroups; the slots are summed in order: equal inputs give
 * equal bits.  Two launches.  Returns -2 for R or C outside 1 .. 65 or n outside [0, 2^31) (nothing is launched), -1 for null
 * pointers or a scratch that is too small. */
int64_t vqn_seg_scratch_bytes(int64_t n, int R, int C);
int vqn_seg_contingency_rgb(const uint8_t* gt_rgb, const uint8_t* pd_rgb, const float* alpha, float alpha_thres, int64_t n,
                            const uint8_t* gt_palette, int n_gt, const uint8_t* pd_palette, int n_pd, void* scratch,
                            int64_t scratch_bytes, void* out, void* stream);
int vqn_seg_contingency_labels(const int32_t* gt, const int32_t* pd, const uint8_t* mask, int64_t n, int n_gt, int n_pd,
                               void* scratch, int64_t scratch_bytes, void* out, void* stream);

/* ---- mean-shift clustering: the baseline of the segmentation table (csrc/meanshift.hip) ---------------------------------------------
 * Replaces sklearn.cluster.MeanShift as the reference's decomp/nerfvq_nfr3/meanshift.py calls it (flat kernel, every sample a seed
 * unless seeds are given, cluster_all) for features that are on the device.  All features are float64, row-major [rows][D],
 * 1 <= D <= 8, rows >= 1, rows * D < 2^31.  The arithmetic is fixed: d2(x, m) = the sum over d = 0 .. D-1, in that order, of
 * (x_d - m_d) * (x_d - m_d), product and sum rounded separately (no FMA).
 * _seek: every seed to convergence in ONE launch.  Per seed, from m = the seed: neighbours = the points with d2(x, m) <= b * b; none:
 * the seed is dropped (count 0, its mean stays); else m' = sum(neighbours) / their number (a division); it stops when
 * sqrt(d2(m', m)) <= 1e-3 * b or when max_iter iterations are complete, else m = m' and one more iteration is complete.
 * means [n_seeds][D] = the last m', counts = the size of the last neighbour set, iters = the completed iterations.  A seed's
 * neighbour sum is added in an order that depends on the point indices alone (points i with (i mod 256) / 32 = w in ascending i for
 * w = 0 .. 7, then the eight partial sums in that order; no atomics): seeds with equal last neighbour sets get bit-identical means.
 * _merge: candidates [n_candidates][D] with their counts, SORTED by the caller descending by (count, coordinates) (count 0 = dropped,
 * last; exact duplicates may stay).  Walks them in order: a candidate with count > 0 that is not suppressed is kept and suppresses
 * every later one with d2 <= b * b.  kept [n_candidates] bytes 0 / 1, *n_kept their number K (one workgroup, K rounds).
 * scratch: vqn_meanshift_merge_scratch_bytes(n_candidates, D) bytes (a state byte per candidate; 0 for a shape the call refuses).
 * _assign: labels [n] = the index of the centre [K][D] with the least d2, ties to the lowest index; dist (may be NULL) [n] =
 * sqrt of that d2; bandwidth > 0: label -1 where that distance is > bandwidth (cluster_all=False); <= 0: every point is labelled.
 * Return -2 for a shape outside the above (nothing is launched), -1 for null pointers, bandwidth <= 0 (seek, merge), max_iter < 0 or
 * a scratch that is too small. */
int vqn_meanshift_seek(const double* points, int64_t n, const double* seeds, int64_t n_seeds, int D, double bandwidth, int max_iter,
                       double* means, int32_t* counts, int32_t* iters, void* stream);
int64_t vqn_meanshift_merge_scratch_bytes(int64_t n_candidates, int D);
int vqn_meanshift_merge(const double* candidates, const int32_t* cand_counts, int64_t n_candidates, int D, double bandwidth,
                        void* scratch, int64_t scratch_bytes, uint8_t* kept, int32_t* n_kept, void* stream);
int vqn_meanshift_assign(const double* points, int64_t n, const double* centres, int K, int D, double bandwidth, int32_t* labels,
                         double* dist, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_EVAL_H_ */
