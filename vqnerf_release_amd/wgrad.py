"""Weight-gradient contractions over points (csrc/wgrad.hip, csrc/wgrad_x3.hip): the process-wide switches and the two executors
every training engine states its contractions against -- WgradBatch (deferred, one finalize launch per backward pass) and
WgradPerWeight (one partials + reduce sequence per window, at once).  Same contract() / flush(), same sums bit for bit."""
import os

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


# one finalize launch per backward pass (WgradBatch) instead of a reduce + strided write per weight window (WgradPerWeight);
# VQN_WGRAD_BATCH=0 keeps the per-weight sequence (same sums, bit for bit)
BATCHED_WGRAD = [os.environ.get('VQN_WGRAD_BATCH', '1') != '0']


def wgrad_executor(n_split, **batch_kw):
    """the executor BATCHED_WGRAD selects for one backward pass (batch_kw: WgradBatch's own options)"""
    return WgradBatch(n_split, **batch_kw) if BATCHED_WGRAD[0] else WgradPerWeight(n_split)


def _windows(a_rows, b_cols, col_first):
    """the 8 x 8-tile windows of an [a_rows, b_cols] result that hold a column >= col_first: (a0, an, b0, bn, first of its row
    window) in tiles -- the cut both executors share"""
    a_nt_all, b_nt_all = (a_rows + 31) // 32, (b_cols + 31) // 32
    for a0 in range(0, a_nt_all, 8):
        an, first = min(8, a_nt_all - a0), True
        for b0 in range(0, b_nt_all, 8):
            bn = min(8, b_nt_all - b0)
            if col_first >= min(bn * 32, b_cols - b0 * 32) + b0 * 32:
                continue
            yield a0, an, b0, bn, first
            first = False


class WgradBatch:
    """Deferred weight-gradient contractions of one backward pass.  contract() queues a contraction; flush() launches the
    split-over-points partial-block kernels of all of them (one launch per kernel variant, vqn_wgrad_partials_batched, each problem
    into its own slice of ONE workspace), then sums every contraction's blocks in the fixed order of vqn_reduce_partials and writes
    each result where it belongs -- a slice of a concatenated matrix, transposed, scaled, two contractions added -- in ONE launch
    (vqn_wgrad_finalize) instead of a reduce + strided write sequence per weight."""

    def __init__(self, n_split, thin=False, tiles_per_block=1):
        self.n_split = n_split
        # small batches: at least `tiles_per_block` point tiles per partial block.  The reference batch of the reflectance step is 64 point
        # tiles; one block per tile made every workgroup of the partial kernels write a whole weight-sized block for two K steps of
        # matrix work (200 MB of partials per step, as much again read by the finalize launch)
        self.tiles_per_block = max(1, int(tiles_per_block))
        self.thin = thin          # contractions of at most 8 output rows on the vector-ALU stream kernel (vqn_wgrad_thin_batched)
        self.e, self.keep, self.p, self.nt, self.ws_floats, self.pt = [], [], [], None, 0, []

    def _blocks(self, nt):
        """partial blocks per problem (the first contraction fixes the points and with them the split)"""
        if self.nt is None:
            self.nt = nt
            self.n_split = max(1, min(self.n_split, nt // self.tiles_per_block))
        assert nt == self.nt, 'one WgradBatch = contractions over the same points'
        return min(self.n_split, nt)

    def _partials(self, A, B, at, a0, an, bt, b0, bn, nt, want_rs):
        """queue one partial-block problem; -> (workspace offset, row-sum workspace offset | None) in floats"""
        n_blocks = self._blocks(nt)
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
        if self.thin and a_rows <= 8 and A2 is None and col_first == 0 and A.shape[1] == 1:
            self.contract_thin_rows(A, 0, a_rows, B, b_cols, [(0, a_rows, dst, sr, sc, bias_dst)])
            return
        for a0, an, b0, bn, first in _windows(a_rows, b_cols, col_first):
            want_rs = bias_dst is not None and first            # with the first block that runs (block 0 unless col_first skips it)
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
        n_blocks, b_nt_all = self._blocks(nt), (b_cols + 31) // 32
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


class WgradPerWeight:
    """The same contractions run at once, window by window: vqn_wgrad_partials[_x3] + vqn_reduce_partials per 8 x 8-tile window (the
    blocks of the split over points summed in a fixed order; the second operand pair accumulated onto the first), then one strided
    write of the scaled result.  It owns the partial-block workspaces of its pass."""

    def __init__(self, n_split):
        self.n_split = n_split
        self.ws = self.rs_ws = None          # partial blocks / partial row sums of ONE window, at most 8 x 8 tiles

    def contract(self, A, B, a_rows, b_cols, dst, sr, sc, bias_dst=None, A2=None, B2=None, scale=1.0, col_first=0):
        """WgradBatch.contract(), done when it returns."""
        nt, dev = A.shape[0], A.device
        if self.ws is None:              # a call writes min(n_split, point tiles) blocks
            self.nt, self.ws = nt, torch.empty(min(self.n_split, nt) * 256 * 256, dtype=torch.float32, device=dev)
        assert nt == self.nt, 'one executor = contractions over the same points'
        if bias_dst is not None and self.rs_ws is None:
            self.rs_ws = torch.empty(min(self.n_split, nt) * 256, dtype=torch.float32, device=dev)
        rows, cols = (a_rows + 31) // 32 * 32, (b_cols + 31) // 32 * 32
        out = torch.empty((rows, cols), dtype=torch.float32, device=dev)
        rs_out = torch.empty((1, rows), dtype=torch.float32, device=dev) if bias_dst is not None else None
        for pi, (A_, B_) in enumerate(((A, B), (A2, B2))):
            if A_ is None:
                continue
            for a0, an, b0, bn, first in _windows(a_rows, b_cols, col_first):
                want_rs = bias_dst is not None and pi == 0 and first
                n = _C.wgrad_partials(A_, A_.shape[1], a0, an, B_, B_.shape[1], b0, bn, nt, self.n_split, self.ws,
                                      self.rs_ws if want_rs else None, x3=wgrad_mode() == 'bf16x3')
                _C.reduce_partials(self.ws, n, an * 32, bn * 32, out[a0 * 32:, b0 * 32:], cols, pi,
                                   rowsum=(self.rs_ws, rs_out[:, a0 * 32:], rows) if want_rs else None)
        block = out[:a_rows, col_first:b_cols]
        dst.as_strided((a_rows, b_cols - col_first), (sr, sc), dst.storage_offset() + col_first * sc).copy_(
            block if scale == 1.0 else block * scale)
        if bias_dst is not None:
            bias_dst[:a_rows].copy_(rs_out[0, :a_rows])

    def flush(self):
        pass
