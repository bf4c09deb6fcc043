"""The stream format of the device PNG encoder (csrc/png_encode.hip, csrc/png_plan.h), stated in numpy and plain Python: the yardstick
the kernels are held to byte for byte (tests/test_gpu_png.py) and that the CPU checks on its own (tests/test_png_model.py).

File: signature, IHDR, one IDAT, IEND; 8 bits, colour type 0 / 4 / 2 / 6 for C = 1 / 2 / 3 / 4, no interlace.
Filtered stream: row y is 1 + W C bytes, the filter type first.  'adaptive' takes per row the type 0 .. 4 with the smallest sum of
|residual as int8| (ties: the lower type); the other modes force one type.
zlib stream: 78 01, deflate blocks, the big-endian Adler-32 of the filtered stream.  The filtered stream is cut into segments of
rows_per_segment whole rows (default: as many as fit 8 KiB, at least one); every segment is ONE deflate block that ends on a byte
boundary: a Huffman block is followed by an empty stored block (bits 000, zero padding, 00 00 FF FF).  BFINAL is set on the last block
of the last segment only.
Tokens (greedy from the segment start): at p try the distances 1, 2, 3, 4, 6, 8, stride - C, stride, stride + C in that order; a
candidate d is dropped when d > 32768 or p - d lies before the image; the match length counts b[p + l] == b[p + l - d], capped at 258
and at the segment end; the longest wins, ties the earlier; >= 3 is a match, else a literal.
Code: the T prefabricated dynamic tables in order (scripts/make_png_tables.py), then fixed Huffman, then stored; the smallest exact
byte size wins, ties the earlier."""
import importlib.util
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': 5}
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
SEGMENT_TARGET = 8192
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _generator():
    spec = importlib.util.spec_from_file_location('make_png_tables', os.path.join(ROOT, 'scripts', 'make_png_tables.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- bits ------------------------------------------------------------------------------------------------------------------------------
class Bits:
    """an LSB-first bit string: Huffman codes go in from their most significant bit, everything else from the least"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits.extend((value >> i) & 1 for i in range(n))

    def code(self, code, n):
        self.bits.extend((code >> (n - 1 - i)) & 1 for i in range(n))

    def __len__(self):
        return len(self.bits)

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical_codes(lens):
    """RFC 1951 3.2.2: codes of the symbols with lens > 0 (value, msb first)"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = [0] * len(lens)
    for s, n in enumerate(lens):
        if n:
            out[s] = nxt[n]
            nxt[n] += 1
    return out


class Table:
    def __init__(self, lit_lens, dist_lens, header):
        self.lit_lens, self.dist_lens, self.header = list(lit_lens), list(dist_lens), header       # header: Bits, without BFINAL
        self.lit_codes, self.dist_codes = canonical_codes(self.lit_lens), canonical_codes(self.dist_lens)


def dynamic_header(lit_lens, dist_lens, cl_lens, gen):
    """BTYPE 10, HLIT 29, HDIST 29, HCLEN, the code-length code lengths, the run-length-coded 286 + 30 lengths"""
    b = Bits()
    b.put(2, 2)
    b.put(29, 5)
    b.put(29, 5)
    n_cl = max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1
    n_cl = max(n_cl, 4)
    b.put(n_cl - 4, 4)
    for s in CL_ORDER[:n_cl]:
        b.put(cl_lens[s], 3)
    cl_codes = canonical_codes(cl_lens)
    for s, nbits, extra in gen.run_length_code(list(lit_lens[:286]) + list(dist_lens)):
        b.code(cl_codes[s], cl_lens[s])
        b.put(extra, nbits)
    return b


_tables = None


def tables():
    """the candidates of a segment in order: the dynamic tables, then fixed Huffman"""
    global _tables
    if _tables is None:
        gen = _generator()
        _tables = [Table(l, d, dynamic_header(l, d, c, gen)) for l, d, c in gen.tables()]
        fixed = Bits()
        fixed.put(1, 2)
        _tables.append(Table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30, fixed))
    return _tables


# ---- filters -----------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, mode='adaptive'):
    """uint8 [H, W, C] (or [H, W]) -> (uint8 [H, 1 + W C], the type of every row)"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    raw = img.reshape(H, W * C).astype(np.int64)
    out = np.zeros((H, 1 + W * C), np.uint8)
    for y in range(H):
        x = raw[y]
        up = raw[y - 1] if y else np.zeros_like(x)
        left = np.concatenate([np.zeros(C, np.int64), x[:-C]]) if W * C > C else np.zeros_like(x)
        upleft = np.concatenate([np.zeros(C, np.int64), up[:-C]]) if W * C > C else np.zeros_like(x)
        res = [x, x - left, x - up, x - (left + up) // 2, x - _paeth(left, up, upleft)]
        res = [(r & 255).astype(np.uint8) for r in res]
        if mode == 'adaptive':
            sums = [int(np.abs(r.view(np.int8).astype(np.int64)).sum()) for r in res]
            t = sums.index(min(sums))
        else:
            t = FILTERS[mode]
        out[y, 0], out[y, 1:] = t, res[t]
    return out, out[:, 0].copy()


def unfilter_rows(filtered, C):
    """the decoder of the PNG specification, for the tests: uint8 [H, 1 + W C] -> uint8 [H, W C]"""
    H, stride = filtered.shape
    out = np.zeros((H, stride - 1), np.int64)
    for y in range(H):
        t = int(filtered[y, 0])
        for i in range(stride - 1):
            a = out[y, i - C] if i >= C else 0
            b = out[y - 1, i] if y else 0
            c = out[y - 1, i - C] if y and i >= C else 0
            pred = [0, a, b, (a + b) // 2, int(_paeth(np.int64(a), np.int64(b), np.int64(c)))][t]
            out[y, i] = (int(filtered[y, i + 1]) + pred) & 255
    return out.astype(np.uint8)


# ---- tokens ------------------------------------------------------------------------------------------------------------------------------
def default_rows_per_segment(stride):
    return max(SEGMENT_TARGET // stride, 1)


def candidates(stride, C):
    return [1, 2, 3, 4, 6, 8, stride - C, stride, stride + C]


def _runs(b, d):
    """run[p] = how many l >= 0 in a row have b[p + l] == b[p + l - d] (0 where p < d)"""
    n = len(b)
    eq = np.zeros(n + 1, bool)
    if d < n:
        eq[d:n] = b[d:] == b[:-d]
    stop = np.flatnonzero(~eq)
    return stop[np.searchsorted(stop, np.arange(n))] - np.arange(n)


def tokenize(b, start, end, stride, C):
    """tokens of the segment b[start:end] of an image's filtered stream b: [('lit', byte) | ('match', length, distance)]"""
    cands = [d for d in candidates(stride, C)]
    runs = [(_runs(b, d) if 1 <= d <= 32768 else None) for d in cands]
    out, p = [], start
    while p < end:
        best, best_d = 0, 0
        for d, r in zip(cands, runs):
            if r is None or p - d < 0:
                continue
            n = min(int(r[p]), 258, end - p)
            if n > best:
                best, best_d = n, d
        if best >= 3:
            out.append(('match', best, best_d))
            p += best
        else:
            out.append(('lit', int(b[p])))
            p += 1
    return out


def _len_symbol(n):
    k = max(i for i in range(29) if LEN_BASE[i] <= n)
    return k, n - LEN_BASE[k]


def _dist_symbol(d):
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, d - DIST_BASE[k]


def token_bits(tokens, t):
    n = 0
    for tok in tokens:
        if tok[0] == 'lit':
            n += t.lit_lens[tok[1]]
        else:
            k, _ = _len_symbol(tok[1])
            j, _ = _dist_symbol(tok[2])
            n += t.lit_lens[257 + k] + LEN_EXTRA[k] + t.dist_lens[j] + DIST_EXTRA[j]
    return n + t.lit_lens[256]


def huffman_bytes(bits):
    """bytes of a Huffman block of `bits` bits (header, tokens, end of block) with the empty stored block behind it"""
    return (bits + 3 + 7) // 8 + 4


def encode_segment(b, start, end, stride, C, final):
    """-> (the bytes of the segment's block(s), the index of the chosen candidate: len(tables()) = stored)"""
    tokens = tokenize(b, start, end, stride, C)
    tabs = tables()
    sizes = [huffman_bytes(1 + len(t.header) + token_bits(tokens, t)) for t in tabs] + [5 + end - start]
    choice = sizes.index(min(sizes))
    if choice == len(tabs):
        n = end - start
        return bytes([1 if final else 0]) + struct.pack('<HH', n, n ^ 0xffff) + bytes(b[start:end]), choice
    t = tabs[choice]
    out = Bits()
    out.put(0, 1)
    out.bits.extend(t.header.bits)
    for tok in tokens:
        if tok[0] == 'lit':
            out.code(t.lit_codes[tok[1]], t.lit_lens[tok[1]])
        else:
            k, e = _len_symbol(tok[1])
            j, f = _dist_symbol(tok[2])
            out.code(t.lit_codes[257 + k], t.lit_lens[257 + k])
            out.put(e, LEN_EXTRA[k])
            out.code(t.dist_codes[j], t.dist_lens[j])
            out.put(f, DIST_EXTRA[j])
    out.code(t.lit_codes[256], t.lit_lens[256])
    out.put(1 if final else 0, 1)
    out.put(0, 2)
    data = out.tobytes() + b'\x00\x00\xff\xff'
    assert len(data) == sizes[choice]
    return data, choice


def zlib_stream(filtered, C, rows_per_segment=None, want_choices=False):
    """filtered uint8 [H, stride] -> the zlib stream"""
    H, stride = filtered.shape
    rows = default_rows_per_segment(stride) if rows_per_segment is None else rows_per_segment
    if rows < 1 or min(rows, H) * stride > 65535:
        raise ValueError('a segment is 1 .. 65535 bytes')
    b = np.ascontiguousarray(filtered).reshape(-1)
    out, choices = [b'\x78\x01'], []
    for y in range(0, H, rows):
        data, c = encode_segment(b, y * stride, min(y + rows, H) * stride, stride, C, y + rows >= H)
        out.append(data)
        choices.append(c)
    out.append(struct.pack('>I', zlib.adler32(b.tobytes())))
    return (b''.join(out), choices) if want_choices else b''.join(out)


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def head(H, W, C):
    """the 33 bytes in front of IDAT"""
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, COLOUR_TYPE[C], 0, 0, 0))


def png_file(img, filters='adaptive', rows_per_segment=None):
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    filtered, _ = filter_rows(img, filters)
    return head(H, W, C) + chunk(b'IDAT', zlib_stream(filtered, C, rows_per_segment)) + chunk(b'IEND', b'')


def chunks(data):
    """[(kind, data, crc ok)] of a file"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    out, p = [], 8
    while p < len(data):
        n, = struct.unpack('>I', data[p:p + 4])
        kind, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        crc, = struct.unpack('>I', data[p + 8 + n:p + 12 + n])
        out.append((kind, body, crc == zlib.crc32(kind + body)))
        p += 12 + n
    return out
