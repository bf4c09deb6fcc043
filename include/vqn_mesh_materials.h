/* vqn_mesh_materials.h -- per-vertex material codes on an indexed triangle mesh, from libvqnerf_hip.so (csrc/mesh_materials.hip; limits,
 * scratch sizes and bitmap geometry by csrc/mesh_materials_plan.h): a label clean-up by majority vote over the mesh, one code per
 * face, and the stable split of the mesh into one sub-mesh per code with a compact vertex list each.  Same conventions as vqn_mesh.h
 * (device pointers owned by the caller, `stream` a hipStream_t, negative return = error with vqn_last_error(), a refused call launches
 * nothing, no memory outside the stated extents is touched).  Every kernel is integer-only; sums are integer sums and every write
 * position follows from a prefix sum, so the outputs are the same from run to run and equal any other correct implementation's.
 *
 * Inputs throughout: tris [n_tris][3] int32 vertex indices; codes [n_verts] int32 in [0, n_codes), the 0-based encoding_indices;
 * 1 <= n_codes <= VQN_MESHMAT_MAX_CODES.  With W = ceil(n_verts / 32) words per code row and B = max(1, ceil(n_tris /
 * VQN_MESHMAT_FACES_PER_BLOCK)) face blocks, every call returns
 *   -1 for a negative size or self_weight / iters, a null pointer (where the array it names is not empty), a scratch that is too
 *      small or not 16-byte aligned, totals that contradict the sizes;
 *   -2 for n_verts >= 2^31, 3 n_tris >= 2^31, n_codes outside 1 .. 128, or n_codes * W >= 2^31.
 * A triangle with a vertex index outside [0, n_verts) is a caller error: it votes for nothing, gets face code -1 and is left out of
 * the split.  A code outside [0, n_codes) is a caller error: it casts no vote, and a triangle that uses such a vertex gets face
 * code -1 as well. */
#ifndef VQN_MESH_MATERIALS_H_
#define VQN_MESH_MATERIALS_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VQN_MESHMAT_MAX_CODES 128        /* codes at most */
#define VQN_MESHMAT_FACES_PER_BLOCK 512  /* consecutive faces that share one row entry of block_count */
#define VQN_MESHMAT_WORD_BITS 32         /* vertices per word of the usage bitmap */

/* ---- label clean-up: `iters` rounds of majority vote over the mesh ---------------------------------------------------------------
 * One round: for every triangle t (all three indices in range) and corner i with v = t[i], vertex v receives one vote for
 * code[t[(i + 1) % 3]] and one for code[t[(i + 2) % 3]] (which also defines the degenerate (a, a, b)), and self_weight >= 0 votes for
 * its own code.  new[v] = code[v] if that code's votes equal the maximum, otherwise the smallest code that holds the maximum; a
 * vertex that received no vote at all (no triangle uses it and self_weight = 0, or every vote came from a code out of range) keeps
 * its code.  Every round reads only the codes of the round before (codes_in for the first) and adds the number of vertices it
 * changed to changed[round] (int32 [iters], device, zeroed by the call).  codes_out [n_verts] receives the last round's codes and
 * must not overlap codes_in; iters = 0 copies codes_in.  n_verts = 0 is a no-op.
 * The votes are gathered through a vertex -> incident-corner list built once per call by count, prefix sum and fill (the fill order
 * does not matter: votes are sums) and counted by one thread per vertex in a table of n_codes counters of its own in LDS, whatever
 * the valence.  scratch: device, 16-byte aligned, at least vqn_mesh_label_scratch_bytes(n_tris, n_verts) bytes (the offsets, the
 * list of 3 n_tris corners, one more code array; < 0: sizes the call refuses). */
int64_t vqn_mesh_label_scratch_bytes(int64_t n_tris, int64_t n_verts);
int vqn_mesh_label_mode(const int32_t* tris, int64_t n_tris, const int32_t* codes_in, int64_t n_verts, int n_codes, int self_weight,
                        int iters, int32_t* codes_out, int32_t* changed, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- face codes and the split by code; the caller does the prefix sums between the two calls, as with vqn_mc_classify / _emit ------
 * Face code: with a, b, c the codes of the three vertices: a if a == b or a == c, else b if b == c, else min(a, b, c).
 *
 * vqn_mesh_split_count fills face_code [n_tris] (-1: dropped); block_count [n_codes][B]: the faces of block j (faces 512 j ..
 * 512 j + 511) that carry each code; bitmap uint32 [n_codes][W]: bit v % 32 of word [k][v / 32] is set iff a face of code k uses
 * vertex v; word_count [n_codes][W]: the set bits of each word.  The EXCLUSIVE prefix sum of block_count, flat in this layout, is
 * block_offset: its entry [k][0] is face_offset[k], the first output row of code k, and its total n_faces = F the number of faces
 * kept.  The flat exclusive prefix sum of word_count is word_offset: entry [k][0] is vert_offset[k] and its total n_slots = S.
 *
 * vqn_mesh_split_emit writes
 *   face_src [F]: the original indices of the kept faces, ordered by (code, original index): a stable counting sort on one digit;
 *   vert_src [S]: for each code in turn the original ids of the vertices its faces use, ascending (a vertex on a border appears once
 *     in every group that uses it);
 *   tris_local [F][3]: row j is face face_src[j] with every vertex id replaced by its rank inside its group's slice of vert_src:
 *     word_offset[k][v / 32] - word_offset[k][0] + the number of set bits below bit v % 32.
 * Rows outside [0, F) / [0, S) are not written (offsets that do not belong to these counts: nothing is written for them).
 * n_tris = 0: nothing is kept, tris is not read. */
int vqn_mesh_split_count(const int32_t* tris, int64_t n_tris, const int32_t* codes, int64_t n_verts, int n_codes, int32_t* face_code,
                         int32_t* block_count, uint32_t* bitmap, int32_t* word_count, void* stream);
int vqn_mesh_split_emit(const int32_t* tris, int64_t n_tris, int64_t n_verts, int n_codes, const int32_t* face_code,
                        const int32_t* block_offset, const uint32_t* bitmap, const int32_t* word_offset, int64_t n_faces,
                        int64_t n_slots, int32_t* face_src, int32_t* tris_local, int32_t* vert_src, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQN_MESH_MATERIALS_H_ */
