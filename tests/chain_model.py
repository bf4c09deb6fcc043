"""numpy emulators of the data movement of the two Dense-stack kernels (csrc/mlp_chain.hip, csrc/mlp_chain_f16s.hip): the activation
image, the A-fragment packs, the MFMA operand maps, executed over a descriptor + weight pack of vqnerf_release_amd/decomp/packing.py
in float64.  They pin the host logic (row allocation, gather indices, descriptor fields) without a GPU: tests/test_chain_packing.py
(the reflectance model's programs) and tests/test_chain_cases.py (the case table of tests/chain_cases.py)."""
import numpy as np
import torch

from oracle import decomp as od

PHI = np.array([2 * (i & 3) + 8 * (i >> 3) + ((i >> 2) & 1) for i in range(32)])


def row_feat(r, h, j):
    return 32 * (r >> 2) + 2 * (4 * (r & 3) + j) + h


def act(a, x):
    """activation of a layer record (bit 8, the late epilogue, is no part of it): 1 relu, 2 softplus(beta = 100), 3 sigmoid"""
    a &= 0xff
    if a == 1:
        return np.maximum(x, 0)
    if a == 2:
        return np.logaddexp(0.0, 100.0 * x) / 100.0
    if a == 3:
        return 1.0 / (1.0 + np.exp(-np.maximum(x, -700.0)))
    return x


def _features(d, x):
    in_mode, in_feats, n_freqs = int(d[1]), int(d[2]), int(d[5])
    if in_mode == 1:
        return od.posenc(torch.tensor(x[:, :3], dtype=torch.float64), n_freqs).numpy()
    return x[:, :in_feats].astype(np.float64)


def emulate(desc, wbuf, x, out_widths):
    """x [P<=32, in_stride] -> list of outputs; float64 arithmetic over the packed float32 weights."""
    d = np.asarray(desc)
    w4 = np.asarray(wbuf, np.float64).reshape(-1, 4)
    n_layers, in_mode, in_feats, in_rows, in_row0, n_freqs, total_rows = [int(v) for v in d[:7]]
    P = x.shape[0]
    lds = np.full((total_rows, 64, 4), np.nan)
    feats = _features(d, x)

    def load_input(row0):
        for r in range(in_rows):
            for lane in range(64):
                p, h = lane & 31, lane >> 5
                for j in range(4):
                    f = row_feat(r, h, j)
                    lds[row0 + r, lane, j] = feats[p, f] if (p < P and f < in_feats) else 0.0

    load_input(in_row0)
    outs = [np.zeros((P, w)) for w in out_widths]
    for l in range(n_layers):
        L = d[16 + 16 * l: 32 + 16 * l]
        kind, a, tiles, kA0, kA, kB0, kB, dst0, w_off, b_off, slot, out_feats = [int(v) for v in L[:12]]
        if kind == 2:                                                                                    # the input image again
            load_input(dst0)
            continue
        rows = [kA0 + i for i in range(kA)] + [kB0 + i for i in range(kB)]
        ng = len(rows)
        if kind == 0:
            # (read once, before any tile is written: a late-epilogue layer writes over its own K rows after the K loops)
            B = np.stack([lds[r] for r in rows]).reshape(ng, 2, 32, 4)                                  # [g,h,n,j]
            for ot in range(tiles):
                # D[i][n] = bias + sum_{g,j,h} A[g][lane=(i,h)][j] * B[g][lane=(n,h)][j]
                A = w4[w_off + ot * ng * 64: w_off + (ot + 1) * ng * 64].reshape(ng, 2, 32, 4)      # [g,h,i,j]
                D = np.einsum('ghij,ghnj->in', A, B)
                bias = w4[b_off + ot * 8: b_off + (ot + 1) * 8].reshape(2, 16)                          # [h][reg]
                for lane in range(64):
                    n_, h = lane & 31, lane >> 5
                    for reg in range(16):
                        i = (reg & 3) + 8 * (reg >> 2) + 4 * h
                        lds[dst0 + ot * 4 + (reg >> 2), lane, reg & 3] = act(a, D[i, n_] + bias[h, reg])
            if slot >= 0:
                for f in range(out_feats):
                    r, fi = f >> 3, f & 7
                    h, j = fi & 1, fi >> 1
                    assert row_feat(r, h, j) == f
                    outs[slot][:, f] = lds[dst0 + r, np.arange(P) + 32 * h, j]
        else:
            img = w4[w_off: w_off + tiles * ng * 2].reshape(tiles, ng, 2, 4)
            B = np.stack([lds[r] for r in rows]).reshape(ng, 2, 32, 4)
            bias4 = d[16 + 16 * l + 12: 16 + 16 * l + 16].view(np.float32).astype(np.float64)
            val = np.einsum('oghj,ghnj->no', img, B)
            outs[slot][:, :tiles] = act(a, val[:P] + bias4[None, :tiles])
    return outs


# ------------------------------------------------------------------ split-precision (f16 hi/lo) programs
def step_feat(sl, h, jj):
    return 16 * sl + 8 * (jj >> 2) + 4 * h + (jj & 3)


def _split(x):
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float64)) * 2048.0).astype(np.float16)
    return hi, lo


def emulate_f16s(desc, wbuf, x, out_widths):
    """numpy emulator of csrc/mlp_chain_f16s.hip: split activation image (row pairs hi / lo), f16 hi/lo A-fragment packs,
    v_mfma_f32_32x32x16_f16 operand maps, three products per step; products and sums in float64."""
    d = np.asarray(desc)
    wb = np.ascontiguousarray(np.asarray(wbuf, np.float32))
    w16 = wb.view(np.float16).astype(np.float64).reshape(-1, 8)          # one 16-byte lane fragment per row
    w4 = wb.astype(np.float64).reshape(-1, 4)
    n_layers, in_mode, in_feats, in_rows, in_row0, n_freqs, total_rows = [int(v) for v in d[:7]]
    assert in_rows % 2 == 0
    P = x.shape[0]
    lds = np.full((total_rows, 64, 8), np.nan)                           # halves, as float64
    feats = _features(d, x)

    def store(row, lane, vals):
        hi, lo = _split(np.asarray(vals, np.float64))
        lds[row, lane], lds[row + 1, lane] = hi, lo

    def load_input(row0):
        for sl in range(in_rows // 2):
            for lane in range(64):
                p, h = lane & 31, lane >> 5
                v = [feats[p, step_feat(sl, h, jj)] if (p < P and step_feat(sl, h, jj) < in_feats) else 0.0 for jj in range(8)]
                store(row0 + 2 * sl, lane, v)

    load_input(in_row0)
    outs = [np.zeros((P, w)) for w in out_widths]
    for l in range(n_layers):
        L = d[16 + 16 * l: 32 + 16 * l]
        kind, a, tiles, kA0, kA, kB0, kB, dst0, w_off, b_off, slot, out_feats = [int(v) for v in L[:12]]
        if kind == 2:
            load_input(dst0)
            continue
        assert kA % 2 == 0 and kB % 2 == 0
        rows = [kA0 + i for i in range(kA)] + [kB0 + i for i in range(kB)]
        nr, ns = len(rows), len(rows) // 2
        B = np.stack([lds[r] for r in rows]).reshape(ns, 2, 2, 32, 8)                                 # [step, part, h, n, jj]
        if kind == 0:
            for ot in range(tiles):
                nrp = 8 * ((nr + 7) // 8)                                                               # packs hold whole 4-step blocks
                A = w16[w_off + ot * nrp * 64: w_off + (ot + 1) * nrp * 64].reshape(nrp // 2, 2, 2, 32, 8)
                assert not A[ns:].any()                                                                # zero padding
                A = A[:ns]                                                                              # [step, part, h, i, jj]
                acc1 = np.einsum('shij,shnj->in', A[:, 0], B[:, 0])
                acc2 = np.einsum('shij,shnj->in', A[:, 0], B[:, 1]) + np.einsum('shij,shnj->in', A[:, 1], B[:, 0])
                bias = w4[b_off + ot * 8: b_off + (ot + 1) * 8].reshape(2, 16)
                for lane in range(64):
                    n_, h = lane & 31, lane >> 5
                    for s in range(2):
                        v = []
                        for jj in range(8):
                            reg = 8 * s + jj
                            i = (reg & 3) + 8 * (reg >> 2) + 4 * h
                            assert i == step_feat(s, h, jj)                                           # registers ARE the half-slots
                            v.append(act(a, acc1[i, n_] + bias[h, reg] + acc2[i, n_] / 2048.0))
                        store(dst0 + ot * 4 + 2 * s, lane, v)
                        if slot >= 0 and n_ < P:
                            for jj in range(8):
                                f = 32 * ot + step_feat(s, h, jj)
                                if f < out_feats:
                                    outs[slot][n_, f] = v[jj]
        elif kind == 1:
            img = w4[w_off: w_off + tiles * ns * 2 * 2].reshape(tiles, ns, 2, 8)
            X = B[:, 0] + B[:, 1] / 2048.0                                                             # [step, h, n, jj]
            bias4 = d[16 + 16 * l + 12: 16 + 16 * l + 16].view(np.float32).astype(np.float64)
            val = np.einsum('oshj,shnj->no', img, X)
            outs[slot][:, :tiles] = act(a, val[:P] + bias4[None, :tiles])
    return outs
