"""Builder of the tile programs csrc/tile_vm.hip interprets: the op list of one 32-point tile, the LDS rows of its regions, and the
weight gathers of its GEMMs (descriptor layout: include/vqn_vm_desc.h).  The geometry and reflectance training engines
(geo/train_programs.py, decomp/train_programs.py) state their passes with it; tests/tile_vm_model.py translates its cases into it."""
import numpy as np

from vqnerf_release_amd.geo.packing import F32, GatherPack

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
