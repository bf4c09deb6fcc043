"""float64 numpy statement of the device JPEG encoder (csrc/jpeg_encode.hip, csrc/jpeg_plan.h): the yardstick of its tests.

Baseline sequential JPEG (SOF0), 8 bit, Y Cb Cr, JFIF.  A frame uint8 [H, W, 3] is padded to whole MCUs by replicating its last row
and column, converted with the JFIF full-range BT.601 matrix (the planes are NOT rounded), the chroma of '420' is the mean of each
2 x 2 square, every 8 x 8 block is level-shifted by 128, transformed with the orthonormal DCT-II, divided by the IJG-scaled Annex K
table and rounded half away from zero.  The entropy coder uses the Annex K Huffman tables and a restart interval of Ri MCUs: every
interval starts with DC predictors 0, is padded with 1-bits to a byte and byte-stuffed on its own; RSTm (m cycling 0 .. 7) stands
between intervals.  Written from the standard (ITU-T T.81) and the JFIF specification, and independent of csrc/jpeg_plan.h."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                 100, 103, 99])
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                   99] + [99] * 32)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546474849'
    '4a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5'
    'c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'), bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748'
    '494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3'
    'c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'))


def quant_tables(quality):
    """(luma, chroma) int [64], natural order: the IJG rule"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((b * s + 50) // 100, 1, 255) for b in (LUMA, CHROMA))


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a BITS / HUFFVAL pair (Annex C)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = tuple(huff_codes(b, DC_VALS) for b in DC_BITS)
AC_CODES = tuple(huff_codes(b, v) for b, v in zip(AC_BITS, AC_VALS))
_x = np.arange(8)
DCT = np.where(_x[:, None] == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * _x[None, :] + 1) * _x[:, None] * np.pi / 16)     # [u, x], orthonormal


def mcu_side(subsampling):
    return {'420': 16, '444': 8}[subsampling]


def planes(rgb, subsampling='420'):
    """uint8 [H, W, 3] -> (Y, Cb, Cr) float64 planes of the padded frame, chroma subsampled for '420'; none rounded"""
    m = mcu_side(subsampling)
    H, W = rgb.shape[:2]
    x = np.pad(rgb, ((0, -H % m), (0, -W % m), (0, 0)), mode='edge').astype(np.float64)
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    Y = .299 * R + .587 * G + .114 * B
    Cb = -.168735892 * R - .331264108 * G + .5 * B + 128
    Cr = .5 * R - .418687589 * G - .081312411 * B + 128
    if subsampling == '420':
        Cb, Cr = (c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3)) for c in (Cb, Cr))
    return Y, Cb, Cr


def _blocks(p):
    by, bx = p.shape[0] // 8, p.shape[1] // 8
    return p.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)           # [by, bx, y, x]


def coefficients(rgb, quality=75, subsampling='420'):
    """-> ({'y', 'cb', 'cr': int16 [by, bx, 64] in zigzag order}, the same keys: the unrounded coef / q, float64)"""
    ql, qc = quant_tables(quality)
    q, raw = {}, {}
    for name, p, table in zip(('y', 'cb', 'cr'), planes(rgb, subsampling), (ql, qc, qc)):
        b = _blocks(p) - 128.0
        c = np.einsum('uy,abyx,vx->abuv', DCT, b, DCT).reshape(b.shape[0], b.shape[1], 64) / table
        c = c[..., ZIGZAG]
        raw[name] = c
        q[name] = (np.sign(c) * np.floor(np.abs(c) + 0.5)).astype(np.int16)     # half away from zero
    return q, raw


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _magnitude(v):
    a = abs(int(v))
    cat = a.bit_length()
    return cat, (int(v) if v > 0 else int(v) - 1) & ((1 << cat) - 1)


def _block(w, zz, pred, cls):
    zz = [int(v) for v in zz]
    cat, bits = _magnitude(zz[0] - pred)
    w.put(*DC_CODES[cls][cat])
    w.put(bits, cat)
    run = 0
    for v in zz[1:]:
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*AC_CODES[cls][0xf0])
            run -= 16
        cat, bits = _magnitude(v)
        w.put(*AC_CODES[cls][run << 4 | cat])
        w.put(bits, cat)
        run = 0
    if run:
        w.put(*AC_CODES[cls][0x00])
    return zz[0]


def mcu_blocks(subsampling, my, mx):
    """the blocks of MCU (my, mx) in scan order: (plane name, block row, block column, table class)"""
    if subsampling == '420':
        return [('y', 2 * my + i, 2 * mx + j, 0) for i in (0, 1) for j in (0, 1)] + [('cb', my, mx, 1), ('cr', my, mx, 1)]
    return [('y', my, mx, 0), ('cb', my, mx, 1), ('cr', my, mx, 1)]


def entropy_encode(coeffs, Ri, subsampling='420'):
    """coeffs {'y', 'cb', 'cr': int [by, bx, 64]} of ONE frame -> the bytes between SOS and EOI"""
    mcus_y, mcus_x = coeffs['cb'].shape[:2]
    order = [(my, mx) for my in range(mcus_y) for mx in range(mcus_x)]
    out = bytearray()
    for i, start in enumerate(range(0, len(order), Ri)):
        if i:
            out += bytes([0xff, 0xd0 + (i - 1) % 8])
        w, pred = _Bits(), {'y': 0, 'cb': 0, 'cr': 0}
        for my, mx in order[start:start + Ri]:
            for name, r, c, cls in mcu_blocks(subsampling, my, mx):
                pred[name] = _block(w, coeffs[name][r, c], pred[name], cls)
        out += w.finish()
    return bytes(out)


def header(H, W, quality, subsampling, Ri):
    b = bytearray(b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t, q in enumerate(quant_tables(quality)):
        b += b'\xff\xdb\x00\x43' + bytes([t]) + bytes(int(v) for v in q[ZIGZAG])
    b += b'\xff\xc0\x00\x11\x08' + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + b'\x03'
    b += bytes([1, 0x22 if subsampling == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for ident, bits, vals in ((0x00, DC_BITS[0], DC_VALS), (0x10, AC_BITS[0], AC_VALS[0]), (0x01, DC_BITS[1], DC_VALS), (0x11, AC_BITS[1], AC_VALS[1])):
        b += b'\xff\xc4' + (19 + len(vals)).to_bytes(2, 'big') + bytes([ident]) + bytes(bits) + bytes(vals)
    b += b'\xff\xdd\x00\x04' + Ri.to_bytes(2, 'big')
    b += b'\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'
    return bytes(b)


def default_interval(W, subsampling):
    """one MCU row"""
    m = mcu_side(subsampling)
    return (W + m - 1) // m


def encode(rgb, quality=75, subsampling='420', Ri=None):
    """uint8 [H, W, 3] -> a complete file"""
    H, W = rgb.shape[:2]
    Ri = default_interval(W, subsampling) if Ri is None else Ri
    q, _ = coefficients(rgb, quality, subsampling)
    return header(H, W, quality, subsampling, Ri) + entropy_encode(q, Ri, subsampling) + b'\xff\xd9'
