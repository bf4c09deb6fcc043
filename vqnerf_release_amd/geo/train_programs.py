"""Training passes of the fused NeuS networks as tile programs for csrc/tile_vm.hip (+ csrc/wgrad.hip).

The reference gets these from autograd: `loss.backward()` through SDFNetwork / RenderingNetwork
(geo/NeuS-ours2/models/fields.py:72-107,147-172), with `create_graph=True` in SDFNetwork.gradient (fields.py:100-106)
so that the eikonal term and the normal-dependent colour differentiate through d sdf / dx.  Here, per 32-point tile:

  forward   e = posenc(x);  u_{l+1} = softplus(W_l in_l + b_l)   (in_l = u_l, or [u_l ; e]/sqrt2 at the skip layer)
            out = W_L u_L + b_L = [sdf ; feat]
            reverse sweep  g^_l = (W_{l+1}^T g^_{l+1}) * softplus'(a_l)  ->  n = J_posenc^T e_bar          (= d sdf / dx)
            colour net on [x, posenc(view), n, feat]
  backward  colour reverse sweep -> d/d feat, d/d n;   v = d loss / d n (compositing + eikonal + colour)
            tangent pass along v:  u'_{l+1} = softplus'(a_l) * (W_l in'_l),  source S_l = g^_l * (W_l in'_l) * softplus''/softplus'
            reverse sweep          a_bar_l = (W_{l+1}^T a_bar_{l+1}) * softplus'(a_l) + S_l
  weights   dW_l = a_bar_l (x) in_l + g^_l (x) in'_l   (contractions over points: csrc/wgrad.hip),  db_l = sum a_bar_l
(the adjoint of the tangent stream IS the forward's reverse sweep, which is why g^_l is saved rather than recomputed).
"""
import os
import math

import numpy as np
import torch

from vqnerf_release_amd import _C

# Weight-gradient contraction: 'f32' = the f32-input MFMA (bit-for-bit a k-ordered fmaf chain); 'bf16x3' = every operand split
# exactly into three bf16 pieces, six MFMAs per product down to 2^-24 (csrc/wgrad_x3.hip): f32-level results, 2.7x less matrix time.
# Round 3: 'bf16x3' is the DEFAULT -- it holds the same 5e-3 bound against the REAL reference's parameter gradients as the f32
# contraction (tests/test_gpu_neus_hits.py, tests/test_gpu_neus_render.py run both), is as deterministic (fixed order, no
# atomics) and 2e-6 of max|g| from it.  VQN_WGRAD=f32 / wgrad_mode('f32') selects the f32-input MFMA contraction.
WGRAD_ENTRY = {'f32': 'vqn_wgrad_partials', 'bf16x3': 'vqn_wgrad_partials_x3'}
_wgrad_mode = [os.environ.get('VQN_WGRAD', 'bf16x3')]


def wgrad_mode(new=None):
    """Get (or set) the contraction used by every training engine of the process."""
    if new is not None:
        assert new in WGRAD_ENTRY, new
        _wgrad_mode[0] = new
    return _wgrad_mode[0]

from vqnerf_release_amd.geo import packing
from vqnerf_release_amd.geo.packing import F32, FlatLayout, GatherPack

# forward of the full-size training engine: 'x3' = the exact-split render kernel (bf16 piece triples, products to 2^-24: f32-level
# saved tensors, 6.4 ms per 2560-ray step), 'fused' = the f32-input MFMA one (8.1 ms), 'prog' = the interpreted program (9.3 ms);
# VQN_TRAIN_FWD overrides.  x3 is the default since every training test -- the reference's gradient goldens at the unchanged 5e-3 bound,
# the torch-autograd comparisons, the graph replays -- passes under it (the gate VERDICT r02 set for the bf16x3 contraction).
TRAIN_FWD_DEFAULT = 'x3'
TRAIN_COARSE_DEFAULT = 'x3'       # the no-grad up-sampling SDF passes of a training render: 'x3' (the step's x3 packs) | 'f32'; VQN_TRAIN_COARSE
TRAIN_BWD_DEFAULT = 'x3'          # the backward likewise: 'x3' 6.8 ms, 'fused' (f32-input MFMA) 8.6 ms, 'prog' 9.8 ms; same gate, same result

# one finalize launch per backward pass (WgradBatch) instead of a reduce / transpose / cat / scale sequence per weight; VQN_WGRAD_BATCH=0
# keeps the per-weight sequence (same sums, bit for bit)
BATCHED_WGRAD = [os.environ.get('VQN_WGRAD_BATCH', '1') != '0']


class WgradBatch:
    """Deferred weight-gradient contractions of one backward pass.  contract() queues a contraction; flush() launches the
    split-over-points partial-block kernels of all of them (one launch per kernel variant, vqn_wgrad_partials_batched, each problem
    into its own slice of ONE workspace), then sums every contraction's blocks in the fixed order of vqn_reduce_partials and writes
    each result where it belongs -- a slice of a concatenated matrix, transposed, scaled, two contractions added -- in ONE launch
    (vqn_wgrad_finalize) instead of a reduce + transpose + cat + scale kernel sequence per weight."""

    def __init__(self, n_split, thin=False, tiles_per_block=1):
        self.n_split = n_split
        # small batches: at least `tiles_per_block` point tiles per partial block.  The reference batch of the reflectance step is 64 point
        # tiles; one block per tile made every workgroup of the partial kernels write a whole weight-sized block for two K steps of
        # matrix work (200 MB of partials per step, as much again read by the finalize launch)
        self.tiles_per_block = max(1, int(tiles_per_block))
        self.thin = thin          # contractions of at most 8 output rows on the vector-ALU stream kernel (vqn_wgrad_thin_batched)
        self.e, self.keep, self.p, self.nt, self.ws_floats, self.pt = [], [], [], None, 0, []

    def _partials(self, A, B, at, a0, an, bt, b0, bn, nt, want_rs):
        """queue one partial-block problem; -> (workspace offset, row-sum workspace offset | None) in floats"""
        if self.nt is None:
            self.nt = nt
            self.n_split = max(1, min(self.n_split, nt // self.tiles_per_block))
        assert nt == self.nt, 'one WgradBatch = contractions over the same points'
        n_blocks = min(self.n_split, nt)
        ws, self.ws_floats = self.ws_floats, self.ws_floats + n_blocks * an * 32 * bn * 32
        rs = None
        if want_rs:
            rs, self.ws_floats = self.ws_floats, self.ws_floats + n_blocks * an * 32
        self.p.append((A, at, a0, an, B, bt, b0, bn, ws, rs))
        return ws, rs

    def contract(self, A, B, a_rows, b_cols, dst, sr, sc, bias_dst=None, A2=None, B2=None, scale=1.0, col_first=0):
        """sum_p A[o][p] B[i][p] (+ sum_p A2[o][p] B2[i][p]), times scale -> element (o, i) at dst.flatten()[o * sr + i * sc] for
        o < a_rows, col_first <= i < b_cols (dst: a tensor / view whose first element is where (0, 0) goes); bias_dst [a_rows]:
        also sum_p A[o][p].  A, B: TFMT tensors [point tiles, feature tiles, 32, 32]."""
        nt, at, bt = A.shape[0], A.shape[1], B.shape[1]
        a_nt_all, b_nt_all = (a_rows + 31) // 32, (b_cols + 31) // 32
        if self.thin and a_rows <= 8 and A2 is None and col_first == 0 and A.shape[1] == 1:
            self.contract_thin_rows(A, 0, a_rows, B, b_cols, [(0, a_rows, dst, sr, sc, bias_dst)])
            return
        for a0 in range(0, a_nt_all, 8):
            an = min(8, a_nt_all - a0)
            rs_done = False
            for b0 in range(0, b_nt_all, 8):
                bn = min(8, b_nt_all - b0)
                if col_first >= min(bn * 32, b_cols - b0 * 32) + b0 * 32:
                    continue
                want_rs = bias_dst is not None and not rs_done      # with the first block that runs (block 0 unless col_first skips it)
                rs_done = rs_done or want_rs
                ws, rs = self._partials(A, B, at, a0, an, bt, b0, bn, nt, want_rs)
                ws2 = None
                if A2 is not None:
                    ws2, _ = self._partials(A2, B2, A2.shape[1], a0, an, B2.shape[1], b0, bn, nt, False)
                self.e.append(dict(ws=ws, ws2=ws2, src_rows=an * 32, src_cols=bn * 32, rows_valid=min(an * 32, a_rows - a0 * 32),
                                   col_first=max(0, col_first - b0 * 32), cols_valid=min(bn * 32, b_cols - b0 * 32),
                                   dst=dst.data_ptr() + 4 * (a0 * 32 * sr + b0 * 32 * sc), sr=sr, sc=sc, scale=scale))
                if want_rs:
                    self.e.append(dict(ws=rs, ws2=None, src_rows=1, src_cols=an * 32, rows_valid=1, col_first=0,
                                       cols_valid=min(an * 32, a_rows - a0 * 32), dst=bias_dst.data_ptr() + 4 * a0 * 32, sr=0, sc=1, scale=1.0))
        self.keep += [A, B, A2, B2, dst, bias_dst]

    def contract_thin_rows(self, A, a_row0, a_rows, B, b_cols, targets):
        """Thin contraction (vqn_wgrad_thin_batched): rows a_row0 .. a_row0 + a_rows - 1 (a_rows <= 8) of the ONE feature tile of A against
        the b_cols features of B, streamed once; targets = [(row_off, n_rows, dst, sr, sc, bias_dst)]: rows row_off .. row_off + n_rows - 1
        of the result (local numbering) -> element (o, i) at dst.flatten()[o * sr + i * sc], their point sums -> bias_dst."""
        nt, at, bt = A.shape[0], A.shape[1], B.shape[1]
        assert at == 1 and a_rows <= 8
        if self.nt is None:
            self.nt = nt
            self.n_split = max(1, min(self.n_split, nt // self.tiles_per_block))
        assert nt == self.nt, 'one WgradBatch = contractions over the same points'
        n_blocks = min(self.n_split, nt)
        b_nt_all = (b_cols + 31) // 32
        for b0 in range(0, b_nt_all, 8):
            bn = min(8, b_nt_all - b0)
            ws, self.ws_floats = self.ws_floats, self.ws_floats + n_blocks * 8 * bn * 32
            want_rs = b0 == 0 and any(t[5] is not None for t in targets)
            rs = None
            if want_rs:
                rs, self.ws_floats = self.ws_floats, self.ws_floats + n_blocks * 32
            self.pt.append((A, at, 0, a_row0, a_rows, B, bt, b0, bn, ws, rs))
            for row_off, n_rows, dst, sr, sc, bias_dst in targets:
                # transposed partial blocks [features, 8]: finalize's row = the feature i, its column = the result row o
                self.e.append(dict(ws=ws, ws2=None, src_rows=bn * 32, src_cols=8, rows_valid=min(bn * 32, b_cols - b0 * 32), col_first=row_off,
                                   cols_valid=row_off + n_rows, dst=dst.data_ptr() + 4 * (b0 * 32 * sc - row_off * sr), sr=sc, sc=sr, scale=1.0))
                if want_rs and bias_dst is not None:
                    self.e.append(dict(ws=rs, ws2=None, src_rows=1, src_cols=32, rows_valid=1, col_first=row_off, cols_valid=row_off + n_rows,
                                       dst=bias_dst.data_ptr() - 4 * row_off, sr=0, sc=1, scale=1.0))
                self.keep += [dst, bias_dst]
        self.keep += [A, B]

    def flush(self):
        e, k, q, m = self.e, len(self.e), self.p, len(self.p)
        qt, mt = self.pt, len(self.pt)
        if m or mt:
            buf = torch.empty(self.ws_floats, dtype=torch.float32, device=(q or qt)[0][0].device)
            base = buf.data_ptr()
            assert base % 16 == 0
            at = lambda off: 0 if off is None else base + 4 * off
            n = min(self.n_split, self.nt)
        if mt:             # columns of the problem tuples: A, a_tiles, a_t0, a_row0, a_rows, B, b_tiles, b_t0, b_nt, ws, rs
            c = list(zip(*qt))
            nthin = _C.wgrad_thin_batched(*c[:9], self.nt, self.n_split, [at(o) for o in c[9]], [at(o) for o in c[10]])
            assert nthin == n
        if m:              # A, a_tiles, a_t0, a_nt, B, b_tiles, b_t0, b_nt, ws, rs
            c = list(zip(*q))
            n = _C.wgrad_partials_batched(*c[:8], self.nt, self.n_split, [at(o) for o in c[8]], [at(o) for o in c[9]], wgrad_mode() == 'bf16x3')
            assert n == min(self.n_split, self.nt)
        if m or mt:
            col = lambda key: [x[key] for x in e]
            _C.wgrad_finalize([at(o) for o in col('ws')], [n] * k, [at(o) for o in col('ws2')], [n] * k, col('src_rows'), col('src_cols'),
                              col('rows_valid'), col('col_first'), col('cols_valid'), col('dst'), col('sr'), col('sc'), col('scale'))
        self.e, self.keep, self.p, self.nt, self.ws_floats, self.pt = [], [], [], None, 0, []


K_LD_POSENC, K_LD_POSENC_JVP, K_LD_T, K_LD_VEC, K_LD_EXTRAS, K_GEMM, K_ST_VEC, K_POSENC_VJP = 1, 2, 3, 4, 5, 6, 7, 8
EPI_ACT, EPI_MUL_DACT, EPI_TANGENT, EPI_BWD2 = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_SIGMOID = 0, 1, 2, 3
MAX_OPS, MAX_TENSORS = 96, 96
DESC_INTS = 16 + MAX_OPS * 16


def _f2i(x):
    return int(np.float32(x).view(np.int32))


class Region:
    """`feats` features of a 32-point tile in LDS rows [row0, row0 + alloc_rows); row0 is assigned by Program.finalize()."""

    def __init__(self, feats, alloc_rows):
        self.row0, self.feats, self.alloc_rows = None, feats, alloc_rows
        self.rows = F32.rows_for(feats)


class _Row:          # placeholder inside an op: "row0 of this region", resolved when the program is finalized
    def __init__(self, region):
        self.region = region


class Program:
    """Op list + the weight gathers its GEMMs need.  LDS rows are assigned at finalize() by an exact depth-first search over
    the allocation requests (each new region must not overlap the regions live at that point), minimising the row count --
    staying under 80 rows keeps two workgroups resident per CU."""

    def __init__(self, tensor_names):
        self.tn = {n: i for i, n in enumerate(tensor_names)}
        assert len(self.tn) <= MAX_TENSORS
        self.ops, self.gathers, self.total_rows = [], [], 0
        self.requests = []          # (region, live regions) in program order

    def t(self, name):
        return -1 if name is None else self.tn[name]

    def alloc(self, feats, live, tiles=None):
        rows = F32.rows_per_tile * tiles if tiles is not None else F32.rows_for(feats)
        r = Region(feats, rows)
        self.requests.append((r, [x for x in live if x is not None]))
        return r

    def gemm(self, key, M_shape, segs, cols, out_feats, live, epi=EPI_ACT, act=ACT_NONE, bias_key=None, aux1=None, aux2=None,
             store=None, store2=None, dst=None, accumulate=False, want_dst=True):
        """segs: Regions forming K; cols[i] = (n_valid, base): local feature f < n_valid of segs[i] is column base + f of M, the others
        are padding (geo/packing.py's K segments) -- or a function f -> column (or -1) where the map is not of that form."""
        tiles = (out_feats + 31) // 32
        if dst is None and want_dst:
            dst = self.alloc(out_feats, list(segs) + list(live), tiles=tiles)
        seg_desc = [(s.rows, c) if callable(c) else (s.rows,) + tuple(c) for s, c in zip(segs, cols)]
        self.gathers.append((key, (M_shape[0], M_shape[1], seg_desc), bias_key, out_feats if bias_key else None, len(self.ops)))
        kA, kB = segs[0], (segs[1] if len(segs) > 1 else None)
        self.ops.append([K_GEMM, tiles, _Row(kA), kA.rows, _Row(kB) if kB else 0, kB.rows if kB else 0, -1, -1,
                         _Row(dst) if dst is not None else -1, epi, act, self.t(aux1), self.t(aux2), self.t(store), self.t(store2),
                         1 if accumulate else 0])
        return dst

    def op(self, kind, *p):
        self.ops.append([kind] + list(p) + [0] * (15 - len(p)))

    def row(self, region):
        return _Row(region)

    def materialize(self):
        """build the (large) gather index arrays"""
        self.gathers = [(key, F32.gemm_index(*spec), bkey, None if bo is None else F32.bias_index(bo), oi)
                        for key, spec, bkey, bo, oi in self.gathers]
        return self

    def _solve_rows(self, node_limit=400000):
        reqs = self.requests
        n = len(reqs)
        best = {'top': None, 'pos': None}
        nodes = [0]
        placed = []

        def rec(i, top, pos):
            if best['top'] is not None and top >= best['top']:
                return
            if i == n:
                best['top'], best['pos'] = top, list(pos)
                return
            nodes[0] += 1
            if nodes[0] > node_limit and best['pos'] is not None:
                return
            reg, live = reqs[i]
            need = reg.alloc_rows
            cands = sorted({0} | {r.row0 + r.alloc_rows for r in placed})
            for c in cands:
                if any(c < r.row0 + r.alloc_rows and r.row0 < c + need for r in live):
                    continue
                reg.row0 = c
                placed.append(reg)
                rec(i + 1, max(top, c + need), pos + [c])
                placed.pop()
                reg.row0 = None
                if best['top'] is not None and nodes[0] > node_limit:
                    return

        rec(0, 0, [])
        assert best['pos'] is not None
        if best['top'] > 80:
            # a packing over 80 rows costs the second resident workgroup: look once more for one that fits, now with every
            # 4-row-aligned offset as a candidate (placing a region only at the end of an earlier one cannot leave room "in front"
            # of a region that is requested later but lives shorter)
            fit = self._solve_rows_under(80)
            if fit is not None:
                best['top'], best['pos'] = max(c + r.alloc_rows for (r, _), c in zip(reqs, fit)), fit
        for (reg, _), c in zip(reqs, best['pos']):
            reg.row0 = c
        return best['top']

    def _solve_rows_under(self, cap, node_limit=300000):
        reqs = self.requests
        n = len(reqs)
        nodes = [0]
        pos = []

        def rec(i):
            if i == n:
                return True
            nodes[0] += 1
            if nodes[0] > node_limit:
                return False
            reg, live = reqs[i]
            need = reg.alloc_rows
            for c in range(0, cap - need + 1, 4):
                if any(c < r.row0 + r.alloc_rows and r.row0 < c + need for r in live):
                    continue
                reg.row0 = c
                pos.append(c)
                if rec(i + 1):
                    return True
                pos.pop()
                reg.row0 = None
                if nodes[0] > node_limit:
                    return False
            return False

        ok = rec(0)
        out = list(pos) if ok else None
        for reg, _ in reqs:
            reg.row0 = None
        return out

    def finalize(self, n_waves=None):
        self.total_rows = self._solve_rows()
        self.ops = [[(e.region.row0 if isinstance(e, _Row) else e) for e in op] for op in self.ops]
        lds = self.total_rows * 1024
        self.n_waves = n_waves or (4 if 2 * lds <= 160 * 1024 else 8)
        assert len(self.ops) <= MAX_OPS, len(self.ops)
        return self


def _shift(lo, hi, base):
    """local features lo..hi-1 -> columns base.., everything else padding (the one column map that is no (n_valid, base) segment:
    OUTF = [sdf ; feat] read without its first row)"""
    return lambda f: np.where((f >= lo) & (f < hi), f - lo + base, -1)


def build_static_packs(programs, layout, mat_index):
    """programs: {name: Program (materialized)}.  mat_index(key) -> int64 array (positions in the flat vector, layout.zero for
    structural zeros) shaped like the matrix / bias the gather key denotes.
    Returns (global gather index [wbuf_len] int64 numpy, {name: desc int32 numpy}) -- both independent of the weight values."""
    pack, descs = GatherPack(layout), {}
    for name, prog in programs.items():
        ops = [list(o) for o in prog.ops]
        for key, wi, bkey, bi, oi in prog.gathers:
            ops[oi][6] = pack.add(mat_index(key), wi)
            if bkey is not None:
                ops[oi][7] = pack.add(mat_index(bkey), bi)
        d = np.zeros(DESC_INTS, np.int32)
        d[0:4] = [len(ops), prog.total_rows, prog.n_waves, len(prog.tn)]
        for i, o in enumerate(ops):
            d[16 + 16 * i: 32 + 16 * i] = o
        descs[name] = d
    return pack.index(), descs


class NeusTrainEngine:
    """Programs, packs and launches for one (SDFNetwork, RenderingNetwork) pair."""

    def __init__(self, sdf_net, col_net, n_split=256):
        self.sdf_net, self.col_net = sdf_net, col_net
        d = sdf_net.dims
        self.nL = len(d) - 2                                   # hidden layers 0..nL-1, final layer nL
        skips = [l for l in sdf_net.skip_in if 0 < l < self.nL + 1]
        assert len(skips) <= 1 and sdf_net.d_in == 3 and sdf_net.multires > 0
        self.skip = skips[0] if skips else -1
        self.E = d[0]
        self.mr = sdf_net.multires
        self.scale = float(sdf_net.scale)
        self.out = [(d[l + 1] - d[0] if (l + 1) == self.skip else d[l + 1]) for l in range(self.nL + 1)]
        self.inn = [d[l] for l in range(self.nL + 1)]
        assert self.skip != self.nL, 'skip into the last layer is not supported'
        self.F = self.out[self.nL]                             # 257 = sdf + features
        c = col_net
        assert c.mode == 'idr' and c.multires_view > 0 and c.dims[-1] == 3
        self.nC = len(c.dims) - 2                              # colour hidden layers 0..nC-1, final nC
        self.mrv = c.multires_view
        self.X = 3 + (3 + 6 * self.mrv) + 3                    # extras: pts, posenc(view), normals
        assert c.dims[0] == self.X + (self.F - 1)
        self.cout = [c.dims[l + 1] for l in range(self.nC + 1)]
        self.cin = [c.dims[l] for l in range(self.nC + 1)]
        self.squeeze = bool(c.squeeze_out)
        self.n_split = int(os.environ.get('VQN_GEO_WGRAD_SPLIT', n_split))      # partial blocks of the contractions over the point tiles
        self._rs_ws = None             # workspace of the fused bias-gradient partial sums
        self._fused_dev = {}           # per device: gather indices + descriptors of the fused forward's packs
        self._bwd_dev = {}             # per device: gather index + descriptor of the fused backward's pack
        self._x3_pack = None           # library-built packs of the exact-split forward (vqn_neus_pack_create, engine 2)
        self._bwd_x3_dev = {}          # per device: gather indices + descriptor of the exact-split backward's packs
        self._x3_prepared = None       # prepare_step() packed these weights already (their key)
        for name, build in (('prog_fwd', self._build_forward), ('prog_cbwd', self._build_colour_backward),
                            ('prog_sbwd', self._build_sdf_backward)):
            prog = build()
            assert prog.total_rows * 1024 <= 160 * 1024, f'{name}: {prog.total_rows} KB of LDS'
            setattr(self, name, prog.materialize())
        self._dev = {}

    # tensor tables -------------------------------------------------------------------------------
    def _tiles(self, f):
        return (f + 31) // 32

    def _tensor_specs(self):
        """name -> ('vec', width) | ('t', feature tiles)"""
        s = {'X': ('vec', 3), 'DIRS': ('vec', 3), 'ONES': ('vec', 1), 'SDF': ('vec', 1), 'N': ('vec', 3), 'RGB': ('vec', 3),
             'DOUT': ('vec', 3), 'GNCOL': ('vec', 3), 'V': ('vec', 3), 'GS': ('vec', 1),
             'E': ('t', self._tiles(self.E)), 'ED': ('t', self._tiles(self.E)), 'OUTF': ('t', self._tiles(self.F)),
             'GOUTF': ('t', self._tiles(self.F)), 'EXTR': ('t', self._tiles(self.X)), 'DC%d' % self.nC: ('t', 1)}
        for l in range(self.nL):
            for nm in ('U%d' % (l + 1), 'UD%d' % (l + 1), 'GH%d' % l, 'S%d' % l, 'AB%d' % l):
                s[nm] = ('t', self._tiles(self.out[l]))
        for l in range(self.nC):
            s['C%d' % (l + 1)] = ('t', self._tiles(self.cout[l]))
            s['DC%d' % l] = ('t', self._tiles(self.cout[l]))
        return s

    # programs --------------------------------------------------------------------------------------
    def _names(self):
        return list(self._tensor_specs().keys())

    def _sdf_fwd_cols(self, l, prev, emb):
        """column maps of W_l for K = [prev (, emb at the skip layer)]"""
        if l == 0:
            return [emb], [(self.E, 0)]
        if l == self.skip:
            return [prev, emb], [(self.out[l - 1], 0), (self.E, self.out[l - 1])]
        return [prev], [(self.inn[l], 0)]

    def _build_forward(self):
        P = Program(self._names())
        nL, nC = self.nL, self.nC
        rE = P.alloc(self.E, [])
        P.op(K_LD_POSENC, P.t('X'), P.row(rE), self.mr, self.E, P.t('E'), _f2i(self.scale))
        prev = None
        for l in range(nL):
            segs, cols = self._sdf_fwd_cols(l, prev, rE)
            prev = P.gemm(('W', l), (self.out[l], self.inn[l]), segs, cols, self.out[l], live=[rE], act=ACT_SOFTPLUS,
                          bias_key=('b', l), store='U%d' % (l + 1))
        rU = prev
        rOUT = P.gemm(('W', nL), (self.F, self.inn[nL]), [rU], [(self.inn[nL], 0)], self.F, live=[], bias_key=('b', nL), store='OUTF')
        P.op(K_ST_VEC, P.row(rOUT), 0, 1, P.t('SDF'), ACT_NONE, _f2i(1.0 / self.scale))
        # reverse sweep for n = d sdf / dx.  rOUT is NOT kept in LDS meanwhile (it is re-read from OUTF for the colour net):
        # that keeps the program under 80 KB, i.e. two workgroups per CU.
        rONE = P.alloc(1, [])
        P.op(K_LD_VEC, P.t('ONES'), P.row(rONE), 1, _f2i(1.0), -1, 0)
        g = P.gemm(('WT_sdfrow',), (self.out[nL - 1], 1), [rONE], [(1, 0)], self.out[nL - 1], live=[],
                   epi=EPI_MUL_DACT, act=ACT_SOFTPLUS, aux1='U%d' % nL, store='GH%d' % (nL - 1))
        rEB, have_eb = None, False
        for l in range(nL - 1, 0, -1):
            # adjoint of in_l = W_l^T g^_l ; its u-part times softplus'(a_{l-1}) is g^_{l-1}
            if l == self.skip:
                rEB = P.gemm(('WT_e', l), (self.E, self.out[l]), [g], [(self.out[l], 0)], self.E, live=[g])
                have_eb = True
            keep = [g] + ([rEB] if have_eb else [])
            g = P.gemm(('WT_u', l), (self.out[l - 1], self.out[l]), [g], [(self.out[l], 0)], self.out[l - 1], live=keep,
                       epi=EPI_MUL_DACT, act=ACT_SOFTPLUS, aux1='U%d' % l, store='GH%d' % (l - 1))
        if have_eb:
            P.gemm(('WT_e', 0), (self.E, self.out[0]), [g], [(self.out[0], 0)], self.E, live=[], dst=rEB, accumulate=True)
        else:
            rEB = P.gemm(('WT_e', 0), (self.E, self.out[0]), [g], [(self.out[0], 0)], self.E, live=[g])
        P.op(K_POSENC_VJP, P.row(rEB), P.t('X'), P.t('N'), self.mr, _f2i(self.scale))
        # colour network on [pts, posenc(view), normals, feat]
        rOUT = P.alloc(self.F, [], tiles=self._tiles(self.F))
        P.op(K_LD_T, P.t('OUTF'), P.row(rOUT), rOUT.rows)
        rEX = P.alloc(self.X, [rOUT])
        P.op(K_LD_EXTRAS, P.t('X'), P.t('DIRS'), P.t('N'), P.row(rEX), self.mrv, P.t('EXTR'), self.X)
        prev = P.gemm(('Wc', 0), (self.cout[0], self.cin[0]), [rOUT, rEX], [_shift(1, self.F, self.X), (self.X, 0)], self.cout[0],
                      live=[], act=ACT_RELU, bias_key=('bc', 0), store='C1')
        for l in range(1, nC):
            prev = P.gemm(('Wc', l), (self.cout[l], self.cin[l]), [prev], [(self.cin[l], 0)], self.cout[l], live=[], act=ACT_RELU,
                          bias_key=('bc', l), store='C%d' % (l + 1))
        rRGB = P.gemm(('Wc', nC), (3, self.cin[nC]), [prev], [(self.cin[nC], 0)], 3, live=[],
                      act=ACT_SIGMOID if self.squeeze else ACT_NONE, bias_key=('bc', nC))
        P.op(K_ST_VEC, P.row(rRGB), 0, 3, P.t('RGB'), ACT_NONE, _f2i(1.0))
        return P.finalize()

    def _build_colour_backward(self):
        P = Program(self._names())
        nC = self.nC
        rD = P.alloc(3, [], tiles=1)
        P.op(K_LD_VEC, P.t('DOUT'), P.row(rD), 3, _f2i(1.0), P.t('DC%d' % nC), 0)
        for l in range(nC, 0, -1):                            # delta_{l-1} = (Wc_l^T delta_l) * relu'(c_l)
            rD = P.gemm(('WcT', l), (self.cin[l], self.cout[l]), [rD], [(self.cout[l], 0)], self.cin[l], live=[],
                        epi=EPI_MUL_DACT, act=ACT_RELU, aux1='C%d' % l, store='DC%d' % (l - 1))
        # adjoints of the colour-net inputs: [sdf(=0) ; feat] in OUTF feature order, and the extras (normals at X-3..X-1)
        P.gemm(('WcT0_feat',), (self.F, self.cout[0]), [rD], [(self.cout[0], 0)], self.F, live=[rD], store='GOUTF', want_dst=False)
        rGX = P.gemm(('WcT0_extra',), (self.X, self.cout[0]), [rD], [(self.cout[0], 0)], self.X, live=[rD])
        P.op(K_ST_VEC, P.row(rGX), self.X - 3, 3, P.t('GNCOL'), ACT_NONE, _f2i(1.0))
        return P.finalize()

    def _build_sdf_backward(self):
        P = Program(self._names())
        nL = self.nL
        rED = P.alloc(self.E, [])
        P.op(K_LD_POSENC_JVP, P.t('X'), P.t('V'), P.row(rED), self.mr, self.E, P.t('ED'), _f2i(self.scale))
        prev = None
        for l in range(nL):                                   # tangent pass (no bias)
            segs, cols = self._sdf_fwd_cols(l, prev, rED)
            prev = P.gemm(('W', l), (self.out[l], self.inn[l]), segs, cols, self.out[l], live=[rED], epi=EPI_TANGENT, act=ACT_SOFTPLUS,
                          aux1='U%d' % (l + 1), aux2='GH%d' % l, store='UD%d' % (l + 1), store2='S%d' % l)
        # adjoint of u_L from the final layer: W_L[1:]^T g_feat + W_L[0]^T g_sdf / scale
        rGO = P.alloc(self.F, [])
        P.op(K_LD_T, P.t('GOUTF'), P.row(rGO), rGO.rows)
        rGS = P.alloc(1, [rGO])
        P.op(K_LD_VEC, P.t('GS'), P.row(rGS), 1, _f2i(1.0 / self.scale), -1, 0)
        ab = P.gemm(('WT_last',), (self.out[nL - 1], self.F), [rGO, rGS], [_shift(1, self.F, 1), (1, 0)], self.out[nL - 1], live=[],
                    epi=EPI_BWD2, act=ACT_SOFTPLUS, aux1='U%d' % nL, aux2='S%d' % (nL - 1), store='AB%d' % (nL - 1))
        for l in range(nL - 1, 0, -1):
            ab = P.gemm(('WT_u', l), (self.out[l - 1], self.out[l]), [ab], [(self.out[l], 0)], self.out[l - 1], live=[],
                        epi=EPI_BWD2, act=ACT_SOFTPLUS, aux1='U%d' % l, aux2='S%d' % (l - 1), store='AB%d' % (l - 1))
        return P.finalize()

    # packs -----------------------------------------------------------------------------------------
    def _layout(self):
        shapes = [('W%d' % l, (self.out[l], self.inn[l])) for l in range(self.nL + 1)] + \
                 [('b%d' % l, (self.out[l],)) for l in range(self.nL + 1)] + \
                 [('Wc%d' % l, (self.cout[l], self.cin[l])) for l in range(self.nC + 1)] + \
                 [('bc%d' % l, (self.cout[l],)) for l in range(self.nC + 1)]
        return FlatLayout(shapes)

    def _matrix_index(self, key, L):
        """positions (in the flat source vector) of the [rows, cols] matrix a gather key refers to.  The skip layer's 1/sqrt2
        (fields.py:82) is applied to its source W before flattening (see pack)."""
        kind = key[0]
        if kind == 'W':
            return L['W%d' % key[1]]
        if kind == 'b':
            return L['b%d' % key[1]]
        if kind == 'Wc':
            return L['Wc%d' % key[1]]
        if kind == 'bc':
            return L['bc%d' % key[1]]
        if kind == 'WT_sdfrow':
            return L['W%d' % self.nL][:1].T
        if kind == 'WT_u':                                     # rows = features of u_l (the part of in_l that is u_l)
            l = key[1]
            return L['W%d' % l][:, :self.out[l - 1]].T
        if kind == 'WT_e':
            l = key[1]
            return (L['W%d' % l][:, self.out[l - 1]:] if l == self.skip and l > 0 else L['W%d' % l]).T
        if kind == 'WT_last':
            return L['W%d' % self.nL].T
        if kind == 'WcT':
            return L['Wc%d' % key[1]].T
        if kind == 'WcT0_feat':                                 # rows in OUTF order: [0 (sdf) ; feat]
            M = L['Wc0'][:, self.X:].T
            return np.concatenate([np.full((1, M.shape[1]), L.zero, np.int64), M], 0)
        if kind == 'WcT0_extra':
            return L['Wc0'][:, :self.X].T
        raise KeyError(key)

    def _static(self, device):
        """weight-independent part of the packs: one global gather index + the three descriptors (cached per device)."""
        k = str(device)
        if k not in self._dev:
            L = self._layout()
            progs = {n: getattr(self, n) for n in ('prog_fwd', 'prog_cbwd', 'prog_sbwd')}
            gidx, descs = build_static_packs(progs, L, lambda key: self._matrix_index(key, L))
            self._dev[k] = (L, torch.from_numpy(gidx).to(device), {n: (d, torch.from_numpy(d).to(device)) for n, d in descs.items()})
        return self._dev[k]

    def pack(self, W, b, Wc, bc, want_flat=False):
        """effective weights -> one flat buffer (ONE gather) + the cached per-program descriptors (+ the flat source vector)."""
        L, gidx, descs = self._static(W[0].device)
        src = {}
        for l in range(self.nL + 1):
            src['W%d' % l] = W[l] * (1.0 / math.sqrt(2.0)) if l == self.skip else W[l]
            src['b%d' % l] = b[l]
        for l in range(self.nC + 1):
            src['Wc%d' % l], src['bc%d' % l] = Wc[l], bc[l]
        flat = L.flatten(src)
        return (flat[gidx], descs, flat) if want_flat else (flat[gidx], descs)

    # launches --------------------------------------------------------------------------------------
    def _scratch_names(self):
        """Temporaries of ONE program (the tangent pass's second-order sources, consumed by the reverse sweep of the same prog_sbwd
        program for the same tile): per-workgroup images that stay cache-resident (vqn_tile_program_grid, negative ld)."""
        return {'S%d' % l for l in range(self.nL)}

    def alloc_tensors(self, P, device):
        nt = (P + 31) // 32
        scratch, n_wg = self._scratch_names(), nt
        if scratch:
            n_wg = _C.tile_program_grid(self._static(device)[2]['prog_sbwd'][0], P)
        out = {}
        for name, (kind, w) in self._tensor_specs().items():
            out[name] = torch.empty((P, w), dtype=torch.float32, device=device) if kind == 'vec' \
                else torch.empty((n_wg if name in scratch else nt, w, 32, 32), dtype=torch.float32, device=device)
        out['ONES'].fill_(1.0)
        return out

    def run(self, which, descs, wbuf, tensors, P):
        prog = getattr(self, which)
        d_host, d_dev = descs[which]
        names = list(prog.tn.keys())
        specs, scratch = self._tensor_specs(), self._scratch_names()
        _C.tile_program(which, d_dev, d_host, wbuf, [tensors[n] for n in names], [-specs[n][1] if n in scratch else specs[n][1] for n in names], P)

    # the forward on the render kernel ---------------------------------------------------------------
    def fused_forward(self):
        """Run the forward as ONE launch of the two-image render kernel (csrc/neus_mlp.hip, vqn_neus_train_fwd) instead of the
        interpreted prog_fwd: same saved tensors, the render kernel's summation order.  VQN_TRAIN_FWD=prog selects the interpreter."""
        return self.forward_mode() is not None

    def forward_mode(self):
        """'f32' (vqn_neus_train_fwd) | 'x3' (vqn_neus_train_fwd_x3: the exact-split engine) | None (the interpreted prog_fwd).
        VQN_TRAIN_FWD = fused | x3 | prog; networks of fewer than 5 or more than 8 feature tiles always take the interpreter."""
        want = os.environ.get('VQN_TRAIN_FWD', TRAIN_FWD_DEFAULT)
        if want not in ('fused', 'x3') or os.environ.get('VQN_NEUS_TILE32') is not None:
            return None
        mt = max(self.sdf_net.plan(max_tiles=self.col_net.max_tiles()).max_tiles, self.col_net.max_tiles())
        # 5..8 tiles: the kernels' two-image form (two activation images of 9 tiles are 166 KB of LDS: vqn_neus_train_fwd refuses them)
        if not (5 <= mt <= 8 and self.skip != 0 and self.E <= 64 and self.X <= 64):      # (embedding / extras: at most two feature tiles)
            return None
        return 'x3' if want == 'x3' else 'f32'

    def _x3_handle(self):
        if self._x3_pack is None:
            c, sn = self.col_net, self.sdf_net
            self._x3_pack = _C.NeusPackHandle(list(sn.dims), self.skip, self.mr, self.scale, 0, c.dims[1], c.num_layers - 2, self.mrv,
                                              self.squeeze, 2)
        return self._x3_pack

    def prepare_step(self, s_lins, c_lins):
        """Start of a training render whose forward runs on the exact-split engine: the library-built x3 packs from the current
        weights (one weight-norm launch, one gather + split launch per network), made BEFORE the no-grad up-sampling passes so that
        those read them too (the exact-split SDF kernel, 1.5 x the f32-input one) instead of packing the f32 SDF net chunk by chunk;
        the forward of the same step then skips its own update.  Returns the pack handle, or None when this does not apply."""
        if self.forward_mode() != 'x3' or os.environ.get('VQN_TRAIN_COARSE', TRAIN_COARSE_DEFAULT) != 'x3':
            return None
        from vqnerf_release_amd.geo.models.fields import effective_weights
        with torch.no_grad():
            ws = [w.float().contiguous() for w in effective_weights(list(s_lins) + list(c_lins))]
            n = len(s_lins)
            h = self._x3_handle()
            h.update(ws[:n], [m.bias.detach().float().contiguous() for m in s_lins], ws[n:], [m.bias.detach().float().contiguous() for m in c_lins])
        self._x3_prepared = self._weights_key()
        return h

    def _weights_key(self):
        """what the x3 packs were built from: the process-wide weights epoch (optimiser steps, graph replays) + every parameter's version"""
        import vqnerf_release_amd
        return vqnerf_release_amd.WeightsStamp([p for m in (self.sdf_net, self.col_net) for p in m.parameters()],
                                               (vqnerf_release_amd.weights_epoch(),))

    def run_fused_forward_x3(self, W, b, Wc, bc, T, P):
        """the forward on the exact-split engine: packs by the library's own builder (one gather + split launch per network)"""
        if self._x3_prepared is not None and self._x3_prepared == self._weights_key():      # packed at the start of this render: same weights
            self._x3_prepared = None
        else:
            self._x3_prepared = None
            cont = lambda ts: [t if t.is_contiguous() else t.contiguous() for t in ts]
            self._x3_handle().update(cont(W), cont(b), cont(Wc), cont(bc))
        saved = [T['E'], T['OUTF'], T['EXTR']] + [T['U%d' % (l + 1)] for l in range(self.nL)] + [T['GH%d' % l] for l in range(self.nL)] \
            + [T['C%d' % (l + 1)] for l in range(self.nC)]
        _C.neus_train_fwd(None, None, None, None, T['X'], T['DIRS'], saved, self._tiles(self.E), self._tiles(self.F), self._tiles(self.X),
                          T['SDF'], T['N'], T['RGB'], pack=self._x3_pack)

    def _fused_static(self, device):
        """Gather indices of the render kernel's two packs INTO THE FLAT SOURCE VECTOR of pack() (so the forward's packs cost one
        gather each per step) and their descriptors: the plans' own gathers composed with the flat vector's views.  The flat
        vector already holds the skip layer divided by sqrt2, as SdfPackPlan.pack() gathers it."""
        k = str(device)
        if k not in self._fused_dev:
            L = self._layout()
            views = lambda name, n: [L[name + '%d' % l] for l in range(n)]
            plan = self.sdf_net.plan(max_tiles=self.col_net.max_tiles())
            c = self.col_net
            col_plan = packing.ColPackPlan(c.d_feature, c.mode, c.dims[1], c.num_layers - 2, c.dims[-1], c.multires_view, c.squeeze_out,
                                           plan.tiles[-1])
            gi_s = plan.gather_index(L, views('W', self.nL + 1), views('b', self.nL + 1))
            gi_c = col_plan.gather_index(L, views('Wc', self.nC + 1), views('bc', self.nC + 1))
            self._fused_dev[k] = (torch.from_numpy(gi_s).to(device), plan.desc.copy(), torch.from_numpy(gi_c).to(device), col_plan.desc.copy())
        return self._fused_dev[k]

    def run_fused_forward(self, flat, T, P):
        """flat: the flat source vector pack() gathered from (its second result with want_flat=True)."""
        gi_s, d_s, gi_c, d_c = self._fused_static(flat.device)
        saved = [T['E'], T['OUTF'], T['EXTR']] + [T['U%d' % (l + 1)] for l in range(self.nL)] + [T['GH%d' % l] for l in range(self.nL)] \
            + [T['C%d' % (l + 1)] for l in range(self.nC)]
        _C.neus_train_fwd(d_s, flat[gi_s], d_c, flat[gi_c], T['X'], T['DIRS'], saved, self._tiles(self.E), self._tiles(self.F),
                          self._tiles(self.X), T['SDF'], T['N'], T['RGB'])

    # the backward on the two-image engine ---------------------------------------------------------------
    TB_MAX_L = 12

    def backward_mode(self):
        """'x3' (vqn_neus_train_bwd_x3, layers of at most 256 outputs) | 'f32' (vqn_neus_train_bwd) | None (the interpreted programs).
        VQN_TRAIN_BWD = x3 | fused | prog."""
        want = os.environ.get('VQN_TRAIN_BWD', TRAIN_BWD_DEFAULT)
        if want not in ('fused', 'x3') or not self._fused_backward_shape():
            return None
        return 'x3' if want == 'x3' else 'f32'

    def fused_backward(self):
        return self.backward_mode() is not None

    def run_fused_backward_x3(self, flat, T, P, g_rgb, g_n, g_sdf):
        gidx, n_steps, fidx, desc = self._bwd_static(flat.device, 'x3')
        nL, nC = self.nL, self.nC
        saved = [T['U%d' % (l + 1)] for l in range(nL)] + [T['GH%d' % l] for l in range(nL)] + [T['C%d' % (l + 1)] for l in range(nC)]
        outs = [T['DC%d' % l] for l in range(nC + 1)] + [T['GOUTF'], T['ED']] + [T['UD%d' % (l + 1)] for l in range(nL)] + \
            [T['AB%d' % l] for l in range(nL)]
        pieces, wf = _C.pack_x3_gather(flat, gidx, n_steps, fidx)
        _C.neus_train_bwd_x3(desc, pieces, wf, T['X'], g_rgb, T['RGB'] if self.squeeze else None, g_n,
                             g_sdf, saved, outs)

    def _fused_backward_shape(self):
        """Run colour backward + SDF backward as ONE launch of csrc/neus_train_bwd.hip (vqn_neus_train_bwd) instead of the
        interpreted prog_cbwd / prog_sbwd (VQN_TRAIN_BWD=prog selects those).  Same tensors out, the kernel's summation order."""
        if os.environ.get('VQN_NEUS_TILE32') is not None:
            return False
        mt = max(self._tiles(w) for w in self.out[:self.nL] + self.cout[:self.nC] + [self.F - 1])
        return 5 <= mt <= 8 and self.skip != 0 and self.nL >= 2 and self.nC >= 1 and max(self.nL, self.nC) < self.TB_MAX_L and self.E <= 64 and self.X <= 64

    def _bwd_static(self, device, mode='f32'):
        """The backward kernel's weight packs as gathers from the flat source vector of pack(), and its int32 descriptor (TrainBwdDesc),
        in the layout of the engine `mode`.  Matrices in A-fragment order, the thin ones as f32 images.
        'f32' (csrc/neus_train_bwd.hip): ONE buffer -> (int64 gather index, descriptor).
        'x3' (csrc/neus_train_bwd_x3.hip): the matrices form a piece pack (vqn_pack_x3_gather splits what it gathers), the thin
        images an f32 buffer of their own -> (int32 index [steps, 64, 8] of the piece pack, its K steps, int32 index of the images,
        descriptor)."""
        cache, k = (self._bwd_x3_dev if mode == 'x3' else self._bwd_dev), str(device)
        if k in cache:
            return cache[k]
        lay, x3 = packing.LAYOUTS[mode], mode == 'x3'
        L, nL, nC, M = self._layout(), self.nL, self.nC, self.TB_MAX_L
        tl = self._tiles
        emb_rows = lay.rows_for(self.E)
        mats = GatherPack(L, pieces=x3)
        thin = GatherPack(L) if x3 else mats

        def gemm(view, n_out, n_cols, segs=None):
            return mats.add(view, lay.gemm_index(n_out, n_cols, segs))

        offT, offB, offCB = [0] * M, [0] * M, [0] * M
        for l in range(nL):                                   # W_l over K = [u_{l-1} (, e at the skip layer)] (the 1/sqrt2 is in the flat vector)
            if l == 0:
                segs = [(emb_rows, self.E, 0)]
            elif l == self.skip:
                prev = self.out[l - 1]
                segs = [lay.tile_seg(prev), (emb_rows, self.E, prev)]
            else:
                segs = None
            offT[l] = gemm(L['W%d' % l], self.out[l], self.inn[l], segs)
        for l in range(1, nL):                                # W_l[:, :out_{l-1}]^T
            offB[l] = gemm(L['W%d' % l][:, :self.out[l - 1]].T, self.out[l - 1], self.out[l])
        nf, n_last = self.F - 1, self.inn[nL]
        offBtop = gemm(L['W%d' % nL][1:].T, n_last, nf)
        if x3:                                                # the sdf row of W_L: the x3 kernel reads it in accumulator (bias) order,
            offWrow = thin.add(L['W%d' % nL][0], lay.bias_index(n_last))
        else:                                                 # the f32 kernel as a row-dot image
            offWrow = thin.add(L['W%d' % nL][:1], lay.rowdot_index(1, n_last))
        for l in range(1, nC + 1):                            # Wc_l^T; l = nC: its three columns are ONE K step (1 row for f32, 3 for x3)
            segs = [(lay.rows_per_step, self.cout[l], 0)] if l == nC else None
            offCB[l] = gemm(L['Wc%d' % l].T, self.cin[l], self.cout[l], segs)
        offCBfeat = gemm(L['Wc0'][:, self.X:].T, nf, self.cout[0])
        offCBnrm = thin.add(L['Wc0'][:, self.X - 3:self.X].T, lay.rowdot_index(3, self.cout[0]))
        mt = max(tl(w) for w in self.out[:nL] + self.cout[:nC] + [nf])
        desc = np.zeros(16 + 5 * M, np.int32)
        desc[0:14] = [nL, nC, self.skip, emb_rows, self.E, tl(self.E), mt, tl(nf), tl(self.F), int(self.squeeze), offBtop, offWrow, offCBfeat,
                      offCBnrm]
        desc[14] = np.float32(self.scale).view(np.int32)
        desc[15] = np.float32(1.0 / self.scale).view(np.int32)
        for l in range(nL):
            desc[16 + l] = tl(self.out[l])
        for l in range(nC):
            desc[16 + M + l] = tl(self.cout[l])
        desc[16 + 2 * M:16 + 3 * M] = offT
        desc[16 + 3 * M:16 + 4 * M] = offB
        desc[16 + 4 * M:16 + 5 * M] = offCB
        gidx = mats.index()
        if x3:
            assert gidx.size % 512 == 0 and gidx.max() < 2 ** 31
            cache[k] = (torch.from_numpy(gidx.astype(np.int32)).to(device), gidx.size // 512,
                        torch.from_numpy(thin.index().astype(np.int32)).to(device), desc)
        else:
            cache[k] = (torch.from_numpy(gidx).to(device), desc)
        return cache[k]

    def run_fused_backward(self, flat, T, P, g_rgb, g_n, g_sdf):
        """g_rgb [P,3] (adjoint of the colours AFTER the sigmoid when the colour net has one), g_n [P,3] | None, g_sdf [P] | None."""
        gidx, desc = self._bwd_static(flat.device)
        nL, nC = self.nL, self.nC
        saved = [T['U%d' % (l + 1)] for l in range(nL)] + [T['GH%d' % l] for l in range(nL)] + [T['C%d' % (l + 1)] for l in range(nC)]
        outs = [T['DC%d' % l] for l in range(nC + 1)] + [T['GOUTF'], T['ED']] + [T['UD%d' % (l + 1)] for l in range(nL)] + \
            [T['AB%d' % l] for l in range(nL)]
        _C.neus_train_bwd(desc, flat[gidx], T['X'], g_rgb, T['RGB'] if self.squeeze else None, g_n, g_sdf, saved, outs)

    def wgrad(self, A, B, a_rows, b_cols, ws, A2=None, B2=None, rowsum=False):
        """sum_p A[o][p] B[i][p] (+ sum_p A2[o][p] B2[i][p]) -> [a_rows, b_cols] (TFMT tensors [tiles, ft, 32, 32]); the partial
        blocks of the split over points are summed in a fixed order by vqn_reduce_partials (deterministic).
        rowsum=True: also sum_p A[o][p] -> [a_rows] (the bias gradient), accumulated by the same kernel pass."""
        nt, at, bt = A.shape[0], A.shape[1], B.shape[1]
        a_nt_all, b_nt_all = (a_rows + 31) // 32, (b_cols + 31) // 32
        out = torch.empty((a_nt_all * 32, b_nt_all * 32), dtype=torch.float32, device=A.device)
        rs_out = torch.empty((1, a_nt_all * 32), dtype=torch.float32, device=A.device) if rowsum else None
        if rowsum and (self._rs_ws is None or self._rs_ws.device != A.device):
            self._rs_ws = torch.empty(self.n_split * 256, dtype=torch.float32, device=A.device)
        for pi, (A_, B_) in enumerate(((A, B), (A2, B2))):
            if A_ is None:
                continue
            for a0 in range(0, a_nt_all, 8):
                an = min(8, a_nt_all - a0)
                for b0 in range(0, b_nt_all, 8):
                    bn = min(8, b_nt_all - b0)
                    want_rs = rowsum and pi == 0 and b0 == 0
                    n = _C.wgrad_partials(A_, at, a0, an, B_, bt, b0, bn, nt, self.n_split, ws, self._rs_ws if want_rs else None,
                                          x3=wgrad_mode() == 'bf16x3')
                    _C.reduce_partials(ws, n, an * 32, bn * 32, out[a0 * 32:, b0 * 32:], out.stride(0), pi,
                                       rowsum=(self._rs_ws, rs_out[:, a0 * 32:], a_nt_all * 32) if want_rs else None)
        if rowsum:
            return out[:a_rows, :b_cols], rs_out[0, :a_rows]
        return out[:a_rows, :b_cols]

    def weight_grads(self, T, g_sdf, goutf_row0_is_gs=False):
        """dict of gradients w.r.t. the EFFECTIVE weights / biases, from the saved tensors.  goutf_row0_is_gs: the backward kernel left
        d loss / d sdf / scale in row 0 of GOUTF (the fused kernels do, round 4), so the contraction GOUTF x u_L already holds row 0 of
        the last layer's gradient and of its bias -- in torch that row was an elementwise product over u_L (84 M elements at the bench
        batch) and a sum over it: 1 GB of traffic per step."""
        nL, nC, s2 = self.nL, self.nC, 1.0 / math.sqrt(2.0)
        dev = T['X'].device
        tsum = lambda t, n: t.sum((0, 3)).reshape(-1)[:n]        # sum over points of a TFMT tensor -> [features]
        dW, db, dWc, dbc = [None] * (nL + 1), [None] * (nL + 1), [None] * (nC + 1), [None] * (nC + 1)
        uL, udL = T['U%d' % nL], T['UD%d' % nL]
        nt = uL.shape[0]
        if not goutf_row0_is_gs:
            gs = torch.zeros(nt * 32, dtype=torch.float32, device=dev)
            gs[:g_sdf.numel()] = g_sdf.reshape(-1) / self.scale
        if BATCHED_WGRAD[0]:
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            batch = WgradBatch(self.n_split)
            for l in range(nL):
                ab, gh = T['AB%d' % l], T['GH%d' % l]
                dW[l], db[l] = new(self.out[l], self.inn[l]), new(self.out[l])
                ld, sc = self.inn[l], (s2 if l == self.skip else 1.0)
                if l == 0:
                    batch.contract(ab, T['E'], self.out[0], self.E, dW[0], ld, 1, bias_dst=db[0], A2=gh, B2=T['ED'])
                else:
                    pu = self.out[l - 1]
                    batch.contract(ab, T['U%d' % l], self.out[l], pu, dW[l], ld, 1, bias_dst=db[l], A2=gh, B2=T['UD%d' % l], scale=sc)
                    if l == self.skip:
                        batch.contract(ab, T['E'], self.out[l], self.E, dW[l][:, pu:], ld, 1, A2=gh, B2=T['ED'], scale=sc)
            # final layer: rows 1.. from the feature adjoints (row 0 of the contraction is dropped: set below)
            dW[nL], db[nL] = new(self.F, self.inn[nL]), new(self.F)
            batch.contract(T['GOUTF'], uL, self.F, self.out[nL - 1], dW[nL], self.inn[nL], 1, bias_dst=db[nL])
            # colour net: layer 0's input is [extras ; features], the features' columns come from OUTF = [sdf ; features] without its row 0
            dWc[0], dbc[0] = new(self.cout[0], self.cin[0]), new(self.cout[0])
            d0 = T['DC0']
            batch.contract(d0, T['EXTR'], self.cout[0], self.X, dWc[0], self.cin[0], 1)
            batch.contract(d0, T['OUTF'], self.cout[0], self.F, dWc[0][:, self.X - 1:], self.cin[0], 1, bias_dst=dbc[0], col_first=1)
            for l in range(1, nC + 1):
                dWc[l], dbc[l] = new(self.cout[l], self.cin[l]), new(self.cout[l])
                batch.contract(T['DC%d' % l], T['C%d' % l], self.cout[l], self.cin[l], dWc[l], self.cin[l], 1, bias_dst=dbc[l])
            batch.flush()
            # row 0 of the final layer = (g_sdf/scale) (x) u_L + u'_L ; its bias = sum of g_sdf / scale
            if goutf_row0_is_gs:
                dW[nL][0] += tsum(udL, self.out[nL - 1])
            else:
                dW[nL][0] = (uL * gs.view(nt, 1, 1, 32)).sum((0, 3)).reshape(-1)[:self.out[nL - 1]] + tsum(udL, self.out[nL - 1])
                db[nL][0] = gs.sum()
            return dW, db, dWc, dbc
        ws = torch.empty(self.n_split * 256 * 256, dtype=torch.float32, device=dev)
        for l in range(nL):
            ab, gh = T['AB%d' % l], T['GH%d' % l]
            if l == 0:
                g, bsum = self.wgrad(ab, T['E'], self.out[0], self.E, ws, gh, T['ED'], rowsum=True)
            else:
                pu = self.out[l - 1]
                g, bsum = self.wgrad(ab, T['U%d' % l], self.out[l], pu, ws, gh, T['UD%d' % l], rowsum=True)
                if l == self.skip:
                    ge = self.wgrad(ab, T['E'], self.out[l], self.E, ws, gh, T['ED'])
                    g = torch.cat([g, ge], 1) * s2
            dW[l], db[l] = g, bsum
        # final layer: rows 1.. from the feature adjoints, row 0 = (g_sdf/scale) (x) u_L + u'_L
        gl, bl = self.wgrad(T['GOUTF'], T['U%d' % nL], self.F, self.out[nL - 1], ws, rowsum=True)
        if goutf_row0_is_gs:
            gl = gl.clone()
            gl[0] += tsum(udL, self.out[nL - 1])
        else:
            row0 = (uL * gs.view(nt, 1, 1, 32)).sum((0, 3)).reshape(-1)[:self.out[nL - 1]] + tsum(udL, self.out[nL - 1])
            gl = torch.cat([row0[None], gl[1:]], 0)
            bl = bl.clone()
            bl[0] = gs.sum()
        dW[nL], db[nL] = gl, bl
        # colour net
        d0 = T['DC0']
        g_feat, b0 = self.wgrad(d0, T['OUTF'], self.cout[0], self.F, ws, rowsum=True)
        g_ext = self.wgrad(d0, T['EXTR'], self.cout[0], self.X, ws)
        dWc[0], dbc[0] = torch.cat([g_ext, g_feat[:, 1:]], 1), b0
        for l in range(1, nC + 1):
            dl = T['DC%d' % l]
            dWc[l], dbc[l] = self.wgrad(dl, T['C%d' % l], self.cout[l], self.cin[l], ws, rowsum=True)
        return dW, db, dWc, dbc


class NeusCoreFunction(torch.autograd.Function):
    """(x, dirs, W_0.., b_0.., Wc_0.., bc_0..) -> (sdf [P,1], n [P,3], rgb [P,3]); backward = the tile programs."""

    @staticmethod
    def forward(ctx, engine, x, dirs, *params):
        nS, nCc = engine.nL + 1, engine.nC + 1
        W, b = list(params[:nS]), list(params[nS:2 * nS])
        Wc, bc = list(params[2 * nS:2 * nS + nCc]), list(params[2 * nS + nCc:])
        P = x.shape[0]
        # an output the loss does not touch reaches backward() as None (the kernels take a NULL adjoint), not as a tensor of zeros
        ctx.set_materialize_grads(False)
        with torch.no_grad():
            wbuf, descs, flat = engine.pack([w.detach().float() for w in W], [t.detach().float() for t in b],
                                            [w.detach().float() for w in Wc], [t.detach().float() for t in bc], want_flat=True)
            T = engine.alloc_tensors(P, x.device)
            T['X'].copy_(x)
            T['DIRS'].copy_(dirs)
            mode = engine.forward_mode()
            if mode == 'x3':
                engine.run_fused_forward_x3([w.detach().float() for w in W], [t.detach().float() for t in b],
                                            [w.detach().float() for w in Wc], [t.detach().float() for t in bc], T, P)
            elif mode == 'f32':
                engine.run_fused_forward(flat, T, P)
            else:
                engine.run('prog_fwd', descs, wbuf, T, P)
        ctx.engine, ctx.T, ctx.descs, ctx.wbuf, ctx.P, ctx.flat = engine, T, descs, wbuf, P, flat
        return T['SDF'], T['N'], T['RGB']

    @staticmethod
    def backward(ctx, g_sdf, g_n, g_rgb):
        e, T, P = ctx.engine, ctx.T, ctx.P
        with torch.no_grad():
            rgb = T['RGB']
            g_rgb = torch.zeros_like(rgb) if g_rgb is None else g_rgb
            gs = torch.zeros_like(T['SDF']) if g_sdf is None else g_sdf.reshape(-1, 1).contiguous()
            bmode = e.backward_mode()
            if bmode is not None:
                run = e.run_fused_backward_x3 if bmode == 'x3' else e.run_fused_backward
                run(ctx.flat, T, P, g_rgb.contiguous().float(), None if g_n is None else g_n.contiguous().float(),
                    None if g_sdf is None else gs.float())
            else:
                T['DOUT'].copy_(g_rgb * rgb * (1.0 - rgb) if e.squeeze else g_rgb)
                e.run('prog_cbwd', ctx.descs, ctx.wbuf, T, P)
                T['V'].copy_(T['GNCOL'] if g_n is None else g_n + T['GNCOL'])
                T['GS'].copy_(gs)
                e.run('prog_sbwd', ctx.descs, ctx.wbuf, T, P)
            dW, db, dWc, dbc = e.weight_grads(T, gs, goutf_row0_is_gs=bmode is not None)
        ctx.T = ctx.flat = None
        return (None, None, None) + tuple(dW) + tuple(db) + tuple(dWc) + tuple(dbc)
