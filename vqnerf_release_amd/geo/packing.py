"""Host-side weight packing for the fused NeuS kernels, and THE statement of each matrix engine's pack layout on the Python side
(csrc/neus_pack_plan.h and csrc/chain_pack_plan.h are the deliberately independent C statement the tests compare against).

A pack is a pure gather of the effective weight matrix (index tensors are built once per network shape with numpy; applying them
is one `torch.take` per matrix on the device), so it is cheap to redo after every optimiser step.  `LAYOUTS` holds one
`EngineLayout` per engine; everything that depends on the engine is a field or a method of it:

              kernels                 K unit ("step")                 LDS rows per step   steps per A block   weights stored as
    F32       csrc/mlp_prims.h        one LDS row = 8 features        1                   1                   f32
    F16S      csrc/mlp_prims_f16s.h   16 features                     2 (hi, lo)          4                   f16 hi / lo pair
    X3        csrc/mlp_prims_x3.h     16 features                     3 (p0, p1, p2)      2                   exact bf16 x 3 split

    k_features   the local feature held by (step s, lane, slot j), with h = lane >> 5:
                     F32          32 (s >> 2) + 2 (4 (s & 3) + j) + h          j < 4
                     F16S, X3     16 s + 8 (j >> 2) + 4 h + (j & 3)            j < 8
    gemm_index   the A fragments  pack[out tile t][step][lane][j] = M[32 t + row(lane & 31)][col(step, lane, j)]  with row = phi for
                 F32, phi(i) = 2 (i & 3) + 8 (i >> 3) + ((i >> 2) & 1), and the identity otherwise; the steps of all K segments
                 follow each other and are padded with zero columns to whole A blocks
    bias_index   [tile][h][reg]: the output row accumulator register reg of lane half h holds,  F32: 2 reg + h,
                 F16S and X3: (reg & 3) + 8 (reg >> 2) + 4 h
    rowdot_index the rows of a thin matrix as f32 images in activation order: [row][step][h][j] = M[row][col(step, h, j)]

A K segment is `(rows, n_valid, base)` -- `rows` LDS rows whose local features f < n_valid are columns base + f of the matrix, all
others zero -- as `Seg` in the C planner; `(rows, col_fn)` is the escape for a column map that is not of that form.  Without
segments K is the whole tiles of all the matrix's columns (the output image of the GEMM before).
"""
import math

import numpy as np
import torch

MAX_SDF_LAYERS = 12
MAX_COL_LAYERS = 8
SDF_DESC_INTS = 12 + MAX_SDF_LAYERS * 8
COL_DESC_INTS = 16 + MAX_COL_LAYERS * 8


def _phi():
    i = np.arange(32)
    return 2 * (i & 3) + 8 * (i >> 3) + ((i >> 2) & 1)


PHI = _phi()


def split_pack(g):
    """g [T, S, 64, 8] f32 (F16S.gemm_index order) -> flat float32 view of [T, S, 2, 64, 8] f16: hi = f16(w), lo = f16((w - hi) 2^11)."""
    if float(g.abs().max()) > 6.0e4:
        raise ValueError('split-precision packs hold weights as f16 hi/lo: |w| must stay below 6e4')
    hi = g.to(torch.float16)
    lo = ((g - hi.float()) * 2048.0).to(torch.float16)
    return torch.stack([hi, lo], 2).contiguous().view(torch.float32).reshape(-1)


def split3_exact(g):
    """f32 tensor -> (p0, p1, p2) f32 tensors, each with at most 8 significant bits (a bf16 value), p0 + p1 + p2 == g EXACTLY:
    truncation of the low 16 bits of the word, twice on the exact remainders."""
    def trunc(t):
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    p0 = trunc(g)
    r1 = g - p0
    p1 = trunc(r1)
    p2 = trunc(r1 - p1)
    return p0, p1, p2


def split_pack_x3(g):
    """g [T, S, 64, 8] f32 (X3.gemm_index order) -> flat float32 view of [T, S, 3, 64, 8] bf16 pieces (no range limit, no scaling)."""
    if not bool(torch.isfinite(g).all()):
        raise ValueError('x3 packs: non-finite weight')
    pieces = [(p.contiguous().view(torch.int32) >> 16).to(torch.int16) for p in split3_exact(g.float())]
    return torch.stack(pieces, 2).contiguous().view(torch.float32).reshape(-1)


class EngineLayout:
    """The pack layout of one matrix engine: the table of the module docstring, one row per instance."""

    def __init__(self, name, step_feats, rows_per_step, block_steps, split):
        self.name, self.step_feats, self.rows_per_step, self.block_steps, self.split = name, step_feats, rows_per_step, block_steps, split
        self.rows_per_tile = rows_per_step * (32 // step_feats)             # LDS rows per 32-feature tile
        reg, h = np.arange(16)[None, :], np.arange(2)[:, None]
        self.row_map = PHI if step_feats == 8 else np.arange(32)            # output row of a tile that lane & 31 holds in the A fragment
        self.acc_rows = 2 * reg + h if step_feats == 8 else (reg & 3) + 8 * (reg >> 2) + 4 * h     # ... that (lane half, register) accumulates

    def rows_for(self, n_feats):
        """LDS rows of an image of n_feats features"""
        return self.rows_per_step * ((n_feats + self.step_feats - 1) // self.step_feats)

    def tile_seg(self, n_feats, base=0):
        """the K segment of an image that occupies whole 32-feature tiles (a GEMM output), n_feats of them valid"""
        return (self.rows_per_tile * ((n_feats + 31) // 32), n_feats, base)

    def pack_words(self, n):
        """f32 words that n gathered weights occupy once split"""
        return n if self.step_feats == 8 else n * self.rows_per_step // 2    # (f32 as it is; otherwise one 16-bit piece per row of a step)

    def k_features(self, n_rows):
        """[steps, 64, slots] -> local feature held by (step, lane, slot) of an n_rows-row K segment"""
        assert n_rows % self.rows_per_step == 0
        s = np.arange(n_rows // self.rows_per_step)[:, None, None]
        h = (np.arange(64) >> 5)[None, :, None]
        if self.step_feats == 8:
            j = np.arange(4)[None, None, :]
            return 32 * (s >> 2) + 2 * (4 * (s & 3) + j) + h
        j = np.arange(8)[None, None, :]
        return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)

    def _cols(self, segs, n_cols):
        """[steps of all segments, 64, slots] -> column of the matrix (negative = padding); segs None: the whole tiles of all columns"""
        cols = []
        for rows, *m in segs or [self.tile_seg(n_cols)]:
            f = self.k_features(rows)
            cols.append(m[0](f) if len(m) == 1 else np.where(f < m[0], f + m[1], -1))
        return np.concatenate(cols, 0)

    def gemm_index(self, n_out, n_cols, segs=None):
        """Gather index [out tiles, steps (whole A blocks), 64, slots] into M[n_out, n_cols].flatten() ++ [0]."""
        col = self._cols(segs, n_cols)
        pad = (-col.shape[0]) % self.block_steps
        if pad:
            col = np.concatenate([col, np.full((pad,) + col.shape[1:], -1, col.dtype)], 0)
        n_tiles = (n_out + 31) // 32
        row = 32 * np.arange(n_tiles)[:, None, None, None] + self.row_map[np.arange(64) & 31][None, None, :, None]
        row = np.broadcast_to(row, (n_tiles,) + col.shape)
        return np.where((row < n_out) & (col[None] >= 0), row * n_cols + col[None], n_out * n_cols).astype(np.int64)

    def bias_index(self, n_out):
        """[out tiles, 2, 16] gather index into bias[n_out] ++ [0], in accumulator order."""
        f = 32 * np.arange((n_out + 31) // 32)[:, None, None] + self.acc_rows[None]
        return np.where(f < n_out, f, n_out).astype(np.int64)

    def rowdot_index(self, n_out, n_cols, segs=None):
        """[n_out, steps, 2, slots] gather index into M[n_out, n_cols].flatten() ++ [0]: M's rows as f32 images in activation order."""
        col = self._cols(segs, n_cols)[:, ::32, :]                                  # lanes 0 and 32 -> h = 0, 1
        o = np.arange(n_out)[:, None, None, None]
        return np.where((col[None] >= 0) & (col[None] < n_cols), o * n_cols + col[None], n_out * n_cols).astype(np.int64)


F32 = EngineLayout('f32', step_feats=8, rows_per_step=1, block_steps=1, split=lambda g: g.reshape(-1))
F16S = EngineLayout('f16s', step_feats=16, rows_per_step=2, block_steps=4, split=split_pack)
X3 = EngineLayout('x3', step_feats=16, rows_per_step=3, block_steps=2, split=split_pack_x3)
LAYOUTS = {'f32': F32, 'f16s': F16S, 'x3': X3}


def _take(mat, idx_dev):
    flat = torch.cat([mat.reshape(-1), mat.new_zeros(1)])
    return torch.take(flat, idx_dev).reshape(-1)


class FlatLayout:
    """Positions of named source tensors inside one flat vector (the last slot is a constant zero): any transpose / slice
    of a source is then just an integer index array, so a whole weight pack is ONE gather from the flat vector."""

    def __init__(self, shapes):
        self.names = [n for n, _ in shapes]
        self.views, off = {}, 0
        for n, shp in shapes:
            k = int(np.prod(shp))
            self.views[n] = np.arange(off, off + k, dtype=np.int64).reshape(shp)
            off += k
        self.zero = off
        self.size = off + 1
        self._offsets, self._zero = None, {}

    def __getitem__(self, name):
        return self.views[name]

    def flatten(self, tensors):
        """tensors: dict name -> tensor (same shapes as declared) -> flat vector on their device.  One launch (torch.cat of many
        contiguous pieces issues a device-to-device copy per piece on this build: 60 of a captured reflectance step's launches)."""
        first = tensors[self.names[0]]
        if not first.is_cuda:
            return torch.cat([tensors[n].reshape(-1).float() for n in self.names] + [first.new_zeros(1, dtype=torch.float32)])
        from vqnerf_release_amd import parallel
        if self._offsets is None:
            self._offsets = np.cumsum([0] + [int(self.views[n].size) for n in self.names])
        zero = self._zero.get(str(first.device))
        if zero is None:
            zero = self._zero[str(first.device)] = torch.zeros(1, dtype=torch.float32, device=first.device)
        flat = torch.empty(self.size, dtype=torch.float32, device=first.device)
        srcs = [tensors[n].reshape(-1).float() for n in self.names] + [zero]
        o = self._offsets
        parallel.multi_copy([flat[o[i]:o[i + 1]] for i in range(len(self.names))] + [flat[self.zero:]], srcs)
        return flat


class GatherPack:
    """A weight pack as ONE integer gather from a FlatLayout's flat vector, built chunk by chunk.  `pieces`: the chunks are A
    fragments that vqn_pack_x3_gather splits as it gathers, so offsets count the split result: a K step of one tile is
    512 gathered words -> 3 pieces x 64 lanes x 16 B = 192 float4."""

    def __init__(self, layout, pieces=False):
        self.zero, self.pieces, self.chunks, self.off4 = layout.zero, pieces, [], 0

    def add(self, view, idx):
        """view: flat-vector positions shaped like the source matrix; idx: gather index into view.flatten() ++ [zero].
        -> float4 offset of the chunk inside the pack"""
        c = np.append(np.ascontiguousarray(view).reshape(-1), self.zero)[idx.reshape(-1)]
        per4 = 512 if self.pieces else 4
        assert c.size % per4 == 0
        o4, self.off4 = self.off4, self.off4 + (c.size // 512 * 192 if self.pieces else c.size // 4)
        self.chunks.append(c)
        return o4

    def index(self):
        return np.concatenate(self.chunks)


class _PackPlan:
    """What SdfPackPlan and ColPackPlan share: `plan` = [(kind, layer, gather index)] in pack order, then one float4 holding the
    first `n_tail` biases of the last layer (they ride in the pack: no device -> host copy per re-pack)."""
    GEMM_KINDS = ('w', 'wfeat', 'wT', 'wTE')                               # the chunks the engine stores split

    def _finish(self, plan):
        """chunk sizes -> float4 offsets (they depend on the shape alone)"""
        self.plan, self._dev_idx, self.offsets, off = plan, {}, {}, 0
        for kind, l, ix in plan:
            n = self.layout.pack_words(ix.size) if kind in self.GEMM_KINDS else ix.size
            assert n % 4 == 0
            self.offsets[kind, l] = off // 4
            off += n
        self.tail_off = off // 4

    def _layer_rows(self, desc, base):
        for l in range(self.n_lin):
            o = lambda *kinds: next((self.offsets[k, l] for k in kinds if (k, l) in self.offsets), -1)
            desc[base + 8 * l: base + 8 * l + 8] = [self.tiles[l], 0, 0, o('w', 'wfeat'), o('b', 'bfeat'), o('wT'), o('wTE'), 0]

    def _indices(self, device):
        key = str(device)
        if key not in self._dev_idx:
            self._dev_idx[key] = [torch.from_numpy(ix).to(device) for _, _, ix in self.plan]
        return self._dev_idx[key]

    def _tail_index(self, n_bias):
        return np.where(np.arange(4) < self.n_tail, np.arange(4), n_bias)

    def pack(self, weights, biases):
        """weights[l]: effective [out_l, in_l] (weight-norm already applied), biases[l]: [out_l].
        Returns (wbuf float32 [n], desc int32 numpy)."""
        weights = self._scaled(weights)
        chunks = []
        for (kind, l, _), ix in zip(self.plan, self._indices(weights[0].device)):
            c = _take(self._source(kind, l, weights, biases).contiguous(), ix)
            chunks.append(self.layout.split(c.reshape(ix.shape)) if kind in self.GEMM_KINDS else c)
        last = biases[self.n_lin - 1]
        chunks.append(torch.cat([last[:self.n_tail].reshape(-1).float(), weights[0].new_zeros(4 - self.n_tail, dtype=torch.float32)]))
        return torch.cat(chunks).contiguous(), self.desc.copy()

    def gather_index(self, layout, weights, biases):
        """The whole pack as ONE int64 gather index into the flat vector of `layout` (a FlatLayout), given its views of the
        weights and biases.  No scaling: a flat vector that is to reproduce pack() holds what pack() gathers from."""
        assert self.layout is F32, 'a split pack is not a gather of f32 words'
        g = GatherPack(layout)
        for kind, l, ix in self.plan:
            g.add(self._source(kind, l, weights, biases), ix)
        last = biases[self.n_lin - 1]
        g.add(last, self._tail_index(last.size))
        return g.index()


class SdfPackPlan(_PackPlan):
    """Index tensors + descriptor for an SDFNetwork-shaped MLP (fields.py:9-107)."""
    n_tail = 1

    def __init__(self, dims, skip_in, multires, scale, max_tiles=None, with_reverse=True, mode='f32'):
        # dims: [d0, hidden..., d_out] as in fields.py:24 (d0 = embedded input width)
        self.mode = mode                    # 'f16s': packs for csrc/neus_mlp_f16s.hip (f16 pair engine); 'x3': csrc/neus_mlp_x3.hip (exact bf16x3 split)
        self.layout = LAYOUTS[mode]
        self.dims = list(dims)
        self.n_lin = len(dims) - 1
        assert 2 <= self.n_lin <= MAX_SDF_LAYERS
        skips = [l for l in skip_in if 0 < l < self.n_lin]
        assert len(skips) <= 1, 'one skip connection supported'
        self.skip = skips[0] if skips else -1
        assert self.skip != self.n_lin - 1, 'skip into the last layer is not supported'
        self.multires = multires
        self.emb = dims[0]
        assert self.emb == 3 + 6 * multires and self.emb <= 64
        self.emb_rows = self.layout.rows_for(self.emb)
        self.scale = float(scale)
        # true output width of every linear layer (fields.py:38-41)
        self.out_dims = []
        for l in range(self.n_lin):
            o = dims[l + 1] - dims[0] if (l + 1) == self.skip else dims[l + 1]
            self.out_dims.append(o)
        self.in_dims = [dims[l] for l in range(self.n_lin)]
        self.tiles = [(o + 31) // 32 for o in self.out_dims]
        self.feat_out = self.out_dims[-1] - 1
        self.tiles[-1] = (self.feat_out + 31) // 32 if self.feat_out > 0 else 0
        self.max_tiles = max(max(self.tiles), max_tiles or 1)
        self.with_reverse = with_reverse
        self._build()

    def _build(self):
        E, er, lay = self.emb, self.emb_rows, self.layout
        plan = []          # (kind, layer, index array)
        for l in range(self.n_lin):
            if l == 0:
                segs = [(er, E, 0)]
            elif l == self.skip:
                prev = self.out_dims[l - 1]
                segs = [lay.tile_seg(prev), (er, E, prev)]
            else:
                segs = None
            if l < self.n_lin - 1:
                plan.append(('w', l, lay.gemm_index(self.out_dims[l], self.in_dims[l], segs)))
                plan.append(('b', l, lay.bias_index(self.out_dims[l])))
            else:
                if self.feat_out > 0:   # feature rows = rows 1.. of the last layer
                    plan.append(('wfeat', l, lay.gemm_index(self.feat_out, self.in_dims[l], segs)))
                    plan.append(('bfeat', l, lay.bias_index(self.feat_out)))
                plan.append(('wrow', l, lay.rowdot_index(1, self.in_dims[l])))
            if self.with_reverse and l < self.n_lin - 1:
                if l >= 1:
                    prev = self.out_dims[l - 1]
                    plan.append(('wT', l, lay.gemm_index(prev, self.out_dims[l])))
                if l == 0 or l == self.skip:
                    plan.append(('wTE', l, lay.gemm_index(E, self.out_dims[l])))
        self._finish(plan)
        desc = np.zeros(SDF_DESC_INTS, np.int32)
        desc[0:6] = [self.n_lin, self.skip, self.multires, self.emb, self.emb_rows, self.max_tiles]
        desc[6] = np.float32(self.scale).view(np.int32)
        desc[7] = self.offsets['wrow', self.n_lin - 1]
        desc[9] = self.tail_off
        self._layer_rows(desc, 12)
        self.desc = desc

    def _scaled(self, weights):
        """the skip layer's input is [u ; e] / sqrt2 (fields.py:82): folded into its weights"""
        return [W / math.sqrt(2.0) if l == self.skip else W for l, W in enumerate(weights)]

    def _source(self, kind, l, weights, biases):
        W = weights[l]
        if kind in ('b', 'bfeat'):
            return biases[l] if kind == 'b' else biases[l][1:]
        if kind == 'wT':
            return W[:, :self.out_dims[l - 1]].T
        if kind == 'wTE':
            return W[:, self.out_dims[l - 1]:].T if l == self.skip else W.T
        return {'w': W, 'wfeat': W[1:], 'wrow': W[:1]}[kind]


class ColPackPlan(_PackPlan):
    """RenderingNetwork-shaped MLP (fields.py:111-172); input order [pts, view_embed, normals, feat]."""
    n_tail = 3

    def __init__(self, d_feature, mode, d_hidden, n_layers, d_out, multires_view, squeeze_out, feat_tiles, matrix_mode='f32'):
        self.matrix_mode = matrix_mode
        self.layout = lay = LAYOUTS[matrix_mode]
        self.mode = mode
        self.n_view = (3 + 6 * multires_view) if mode in ('idr', 'no_normal') else 0
        self.has_normal = 1 if mode in ('idr', 'no_view_dir') else 0
        self.extra = 3 + self.n_view + 3 * self.has_normal
        self.extra_rows = lay.rows_for(self.extra)
        self.d_feature = d_feature
        self.dims = [self.extra + d_feature] + [d_hidden] * n_layers + [d_out]
        self.n_lin = len(self.dims) - 1
        assert 2 <= self.n_lin <= MAX_COL_LAYERS and d_out == 3
        self.tiles = [(self.dims[l + 1] + 31) // 32 for l in range(self.n_lin)]
        self.squeeze_out = 1 if squeeze_out else 0
        self.feat_tiles = feat_tiles
        plan = []
        for l in range(self.n_lin - 1):
            if l == 0:
                segs = [(lay.rows_per_tile * feat_tiles, d_feature, self.extra), (self.extra_rows, self.extra, 0)]
            else:
                segs = None
            plan.append(('w', l, lay.gemm_index(self.dims[l + 1], self.dims[l], segs)))
            plan.append(('b', l, lay.bias_index(self.dims[l + 1])))
        L = self.n_lin - 1
        plan.append(('wrow', L, lay.rowdot_index(d_out, self.dims[L])))
        self._finish(plan)
        desc = np.zeros(COL_DESC_INTS, np.int32)
        desc[0:8] = [self.n_lin, self.n_view, self.has_normal, self.extra, self.extra_rows, 3, self.squeeze_out, self.offsets['wrow', L]]
        desc[12] = self.tail_off
        self._layer_rows(desc, 16)
        self.desc = desc

    def _scaled(self, weights):
        return weights

    def _source(self, kind, l, weights, biases):
        return weights[l] if kind in ('w', 'wrow') else biases[l]
