// Tile-program descriptor of csrc/tile_vm.hip: a list of ops over LDS "activation image" regions of one
// 32-point tile.  Every field is 4 bytes (host side: flat int32 array built by vqnerf_release_amd/geo/train_programs.py).
// Weight offsets are in float4 units into the pack buffer; tensor operands are indices into the pointer table
// handed to the launch.  Public (the C ABI takes it as `const int32_t*`).
//
// Global tensor formats
//   VEC  : [N, ld] row-major floats (points x few components)
//   TFMT : [n_tiles][F/32][32 features][32 points] floats -- feature-major inside a 32-point tile, so that
//          (a) an accumulator register (fixed feature, 32 lanes = 32 points) is one 128-byte store, and
//          (b) the weight-gradient kernel (csrc/wgrad.hip) reads MFMA operands with lanes = features directly.
#pragma once
#include <stdint.h>

#define VQN_VM_MAX_OPS 96
#define VQN_VM_MAX_TENSORS 96

//
// LDS rows.  A region is a run of consecutive rows; a row holds 8 features of the 32 points (a 32-feature tile is 4 rows).  An op that
// loads `feats` features writes the (feats + 7) / 8 rows that hold them, the features past `feats` of the last row as zero.
//
// What an op writes to global memory (its "written set"; nothing else is touched):
//   * a TFMT store of a non-GEMM op receives exactly the rows the op writes to LDS -- features [0, 8 * rows) of every point tile,
//     all 32 points (VM_LD_POSENC with 39 features: 40 features of the image; VM_LD_VEC with c = 3, f0 = 0: 8) -- and must have
//     at least (rows + 3) / 4 feature tiles; the rest of the image is not written;
//   * a TFMT store of VM_GEMM receives all 32 * n_out_tiles features (padded outputs hold the epilogue of a zero accumulator);
//   * in both, the points past N of the last tile are written as zero;
//   * a VEC destination receives components [0, c) (VM_POSENC_VJP: [0, 3)) of the points below N.
// VEC inputs of the posenc ops and of VM_LD_EXTRAS (x, v, dirs, normals) are read three components wide: ld >= 3.
// vqn_tile_program checks all of this (and what the comments below state) before anything is launched: VQN_ESHAPE.
enum VmKind : int {
  VM_LD_POSENC = 1,       // p0 x(VEC,3)  p1 dst_row0  p2 n_freqs (>= 0)  p3 feats (= 3 + 6 n_freqs)  p4 store TFMT idx|-1  p5 scale(float)
                          // features [s, sin(2^k s), cos(2^k s)]_k of s = x * scale
  VM_LD_POSENC_JVP = 2,   // p0 x  p1 v(VEC,3)  p2 dst_row0  p3 n_freqs  p4 feats  p5 store TFMT|-1  p6 scale(float)
                          // J(s) v, J the Jacobian of the features with respect to s = x * scale (the scale itself is not applied to v)
  VM_LD_T = 3,            // p0 TFMT idx  p1 dst_row0  p2 rows (the first `rows` rows of the image; nothing is stored)
  VM_LD_VEC = 4,          // p0 VEC idx  p1 dst_row0  p2 c (1..8)  p3 scale(float)  p4 store TFMT|-1  p5 feature offset f0 (>= 0)
                          // features [f0, f0 + c) <- scale * the c components; features [0, f0) of the (f0 + c + 7) / 8 rows the op
                          // writes are ZERO-FILLED (in LDS and in the store), like the padding behind f0 + c
  VM_LD_EXTRAS = 5,       // p0 x  p1 dirs  p2 normals|-1  p3 dst_row0  p4 n_view_freqs (0 = none, >= 0)  p5 store TFMT|-1  p6 feats
                          // [x(3), posenc(dirs) (3 + 6 n_view_freqs, none at 0), normals(3) if given]: feats must be exactly their number
  VM_GEMM = 6,            // p0 n_out_tiles p1 kA_row0 p2 kA_rows p3 kB_row0 p4 kB_rows p5 w_off p6 b_off|-1 p7 dst_row0|-1
                          // p8 epilogue  p9 act  p10 aux1 TFMT|-1  p11 aux2 TFMT|-1  p12 store TFMT|-1  p13 store2 TFMT|-1
                          // p14 accumulate-into-dst flag (the accumulator starts from the 4 * n_out_tiles rows of dst; no bias then)
                          // dst (4 * n_out_tiles rows) must NOT share a row with either K segment when n_out_tiles > 1: a wave writes
                          // its first tile while the other waves still read K.  (One output tile may be computed in place.)
                          // store2 is written by VM_EPI_TANGENT only.
  VM_ST_VEC = 7,          // p0 src_row0  p1 f0 (>= 0)  p2 c (1..4)  p3 VEC idx  p4 act  p5 scale(float)
                          // component k of the points below N <- act(feature f0 + k) * scale; f0 .. f0 + c may cross a 32-feature tile
  VM_POSENC_VJP = 8,      // p0 src_row0 (adjoint of the embedding)  p1 x  p2 out VEC(3)  p3 n_freqs  p4 scale(float)
                          // J(s)^T adjoint, s = x * scale (the adjoint with respect to s, as VM_LD_POSENC_JVP)
};

enum VmEpi : int {
  VM_EPI_ACT = 0,         // y = act(acc)
  VM_EPI_MUL_DACT = 1,    // y = acc * act'(.)              act' from the activation OUTPUT stored in aux1
  VM_EPI_TANGENT = 2,     // y = act'(.) * acc ; store2 <- aux2 * acc * (act''/act')(.)
  VM_EPI_BWD2 = 3,        // y = acc * act'(.) + aux2
};

struct VmOp {
  int kind;
  int p[15];
};

struct VmDesc {            // 16 + 96*16 ints
  int n_ops;
  int total_rows;
  int n_waves;             // 4 or 8
  int n_tensors;
  int reserved[12];
  VmOp ops[VQN_VM_MAX_OPS];
};

struct VmTensor {
  float* ptr;
  int ld;                  // VEC: row stride in floats;  TFMT: number of 32-feature tiles
  int pad;
};
