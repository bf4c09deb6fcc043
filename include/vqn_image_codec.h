/* vqn_image_codec.h -- image files of 8-bit frames that are on the device, from libvqnerf_hip.so: baseline JPEG
 * (csrc/jpeg_encode.hip) and PNG (csrc/png_encode.hip).  Same conventions as vqnerf_hip.h (device pointers owned by the caller, host
 * descriptors, `stream` a hipStream_t, negative return = error with vqn_last_error()).  The planners (host only) describe a batch
 * in a struct of int64 words, which the caller may also read as a flat int64 array in the order of the fields. */
#ifndef VQN_IMAGE_CODEC_H_
#define VQN_IMAGE_CODEC_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_JPEG_HEADER_CAP 1024     /* bytes a JPEG header never reaches (it has 629) */
#define VQN_PNG_HEAD_BYTES 33        /* bytes of a PNG file in front of IDAT: signature + IHDR chunk */
#define VQN_PNG_FILTER_ADAPTIVE 5    /* filter modes 0 .. 4 force that type for every row */
#define VQN_PNG_SEGMENT_TARGET 8192  /* bytes a default segment holds at most, in whole rows (at least one) */

/* The geometry of a JPEG batch: what vqn_jpeg_plan writes to `geom`, 24 words. */
struct VqnJpegGeom {
  int64_t n, h, w, quality, sub, ri;                    /* the arguments; sub = 420 or 444, ri = the restart interval in MCUs */
  int64_t mcu, mcus_x, mcus_y, blocks_per_mcu;          /* MCU side in pixels; MCUs per row and column; blocks of an MCU (6 or 3) */
  int64_t intervals;                                    /* restart intervals of a frame */
  int64_t slot_bytes;                                   /* bytes of an interval's slot (a multiple of 16) */
  int64_t by_y, bx_y, by_c, bx_c;                       /* blocks of the Y plane and of a chroma plane */
  int64_t off_cb, off_cr, off_slots, off_lens, off_dst; /* byte offsets into the scratch: Y coefficients are at 0 */
  int64_t scratch_bytes, out_bytes, header_bytes;
};

/* The geometry of a PNG batch: what vqn_png_plan writes to `geom`, 17 words. */
struct VqnPngGeom {
  int64_t n, h, w, c, filter_mode, rows_per_segment;         /* the arguments; rows_per_segment clipped to h */
  int64_t stride;                                            /* bytes of a filtered row: 1 + w c */
  int64_t segments;                                          /* of an image */
  int64_t segment_bytes;                                     /* of every segment but, perhaps, the last of an image */
  int64_t slot_bytes;                                        /* a segment's slot: segment_bytes + 5 (the stored form), up to a multiple of 16 */
  int64_t off_slots, off_lens, off_adler, off_dst, off_sums; /* byte offsets into the scratch: the filtered stream [n][h][stride] is at 0 */
  int64_t scratch_bytes, out_bytes;
};

/* ---- baseline JPEG of 8-bit frames that are on the device (csrc/jpeg_encode.hip; host side csrc/jpeg_plan.h) -------------------------
 * Replaces the per-frame image files and cv2.VideoWriter('MJPG') of the reference's cv2_render.py for frames that the render left on
 * the device (decomp/nerfactor/util/mjpeg.py, decomp/video.py).  SOF0, 8 bit, Y Cb Cr, JFIF; subsampling 420 (MCU 16 x 16: Y00 Y01 Y10
 * Y11 Cb Cr) or 444 (MCU 8 x 8); frames padded to whole MCUs by repeating their last row and column; JFIF full-range BT.601 in f32, planes
 * not rounded, 420 chroma the mean of each 2 x 2 square; level shift, orthonormal 8 x 8 DCT-II in f32; the Annex K tables scaled by
 * `quality` with the IJG rule, rounding half away from zero; the Annex K Huffman tables; a restart interval of `restart_interval` MCUs,
 * every interval coded on its own (predictors 0, padded with 1-bits, byte-stuffed), RSTm between the intervals of a frame.
 * vqn_jpeg_plan (host only, no device): geom (may be NULL) receives the 24 int64 words of struct VqnJpegGeom (above: among them the
 * block counts of the planes, the restart intervals of a frame, the slot size, the byte offsets of the scratch regions, scratch_bytes,
 * out_bytes, header_bytes); header (may be NULL) the bytes of a file from SOI through SOS, header_cap >= 1024 always suffices.
 * vqn_jpeg_encode: rgb uint8 [n][h][w][3]; scratch: 16-byte aligned, scratch_bytes of the plan (with coefficients_only != 0 the bytes
 * in front of off_slots suffice, only the first kernel runs, and out / meta may be NULL).  It then holds the quantised coefficients,
 * int16 in zigzag order: Y [n][by_y][bx_y][64] at 0, Cb and Cr [n][by_c][bx_c][64] at off_cb and off_cr.  out: out_bytes of the plan
 * (the worst case: no content needs more); meta int64 [n][2] = offset and length of each frame's bytes in `out`, the bytes between
 * the SOS segment and EOI, RST markers included.  Five launches, no host read; equal frames give equal bytes.
 * Refused with the reason in vqn_last_error and nothing launched: -1 for n < 1, a zero side, quality outside 1 .. 100, a
 * restart interval outside 1 .. 65535, an unknown subsampling, buffers smaller than the plan's; -2 for a side over 65535 (and, by
 * vqn_jpeg_encode, for more than 65535 frames in one batch: the grid's second dimension). */
int vqn_jpeg_plan(int64_t n, int64_t h, int64_t w, int quality, int subsampling, int64_t restart_interval, int64_t* geom, uint8_t* header,
                  int header_cap);
int vqn_jpeg_encode(const uint8_t* rgb, int64_t n, int64_t h, int64_t w, int quality, int subsampling, int64_t restart_interval,
                    void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_bytes, int64_t* meta, int coefficients_only,
                    void* stream);

/* ---- PNG files of 8-bit images that are on the device (csrc/png_encode.hip; host side csrc/png_plan.h) -------------------------------
 * Replaces the host PNG writer (PIL) on the output path for images the render left on the device (decomp/nerfactor/util/png.py,
 * vis.vis_batch(png='device')).  8 bit, c = 1 / 2 / 3 / 4 channels (colour type 0 / 4 / 2 / 6), no interlace.  filter_mode 0 .. 4
 * forces none / sub / up / average / paeth for every row, 5 picks per row the type with the smallest sum of |residual as int8| (the
 * lower type on a tie).  The filtered stream of an image (row y: the type, then w c bytes) is cut into segments of rows_per_segment
 * whole rows (more rows than the image has: the image); a segment is one deflate block, coded alone: greedy tokens from the
 * distances 1, 2, 3, 4, 6, 8, stride - c, stride, stride + c (the longest match, the earlier candidate on a tie, at least 3 bytes),
 * under the cheapest of the 14 prefabricated dynamic tables of csrc/png_plan.h, fixed Huffman or stored (the earlier on a tie); a
 * Huffman block is followed by an empty stored block, so every segment ends on a byte boundary; BFINAL on the last block of the image.
 * vqn_png_plan (host only, no device): geom (may be NULL) receives the 17 int64 words of struct VqnPngGeom (above: the row stride, the
 * segments of an image, the slot size, the byte offsets of the scratch regions, scratch_bytes, out_bytes); head (may be NULL) the 33
 * bytes of a file in front of its IDAT chunk (signature, IHDR with its CRC), head_cap >= 33.
 * vqn_png_encode: pix uint8 [n][h][w][c]; scratch: 16-byte aligned, scratch_bytes of the plan (with filtered_only != 0 the n h stride
 * bytes of the filtered stream suffice, only the first kernel runs, and out / meta may be NULL).  It then holds the filtered stream
 * [n][h][stride] at 0.  out: out_bytes of the plan (every segment stored: no content needs more); meta int64 [n][2] = offset and
 * length of each image's zlib stream in `out` (78 01, the blocks, the Adler-32): the data of its IDAT chunk, whose CRC the caller
 * takes.  Four launches, no host read; equal images give equal bytes.
 * Refused with the reason in vqn_last_error and nothing launched: -1 for n < 1, a zero side, c outside 1 .. 4, an unknown filter mode,
 * rows_per_segment < 1, buffers smaller than the plan's; -2 for a segment (so also a row) over 65535 bytes, more than 65535 images in
 * a batch (the grids' second dimension), more than 2^24 rows. */
int vqn_png_plan(int64_t n, int64_t h, int64_t w, int64_t c, int filter_mode, int64_t rows_per_segment, int64_t* geom, uint8_t* head,
                 int head_cap);
int vqn_png_encode(const uint8_t* pix, int64_t n, int64_t h, int64_t w, int64_t c, int filter_mode, int64_t rows_per_segment,
                   void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_bytes, int64_t* meta, int filtered_only,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_IMAGE_CODEC_H_ */
