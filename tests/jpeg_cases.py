"""Frames and case lists shared by the JPEG tests (tests/test_jpeg_model.py on the CPU, tests/test_gpu_jpeg.py on the device)."""
import numpy as np

SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (40, 56), (64, 64)]          # (H, W)
SUBSAMPLINGS = ['420', '444']

# an 8 x 8 block of grey levels whose only coefficient that rounds away from zero at quality 100 (all table entries 1) is natural (7, 7)
# = zigzag 63 (294.3; every other one is below 0.36 in magnitude): found by rounding 293 C7 (x) C7 + 128 and nudging single pixels
ZIGZAG63_BLOCK = np.array([[131, 120, 140, 114, 142, 116, 136, 125], [120, 151, 94, 168, 88, 162, 105, 136],
                           [140, 94, 179, 68, 188, 77, 162, 116], [114, 168, 68, 199, 58, 188, 88, 142],
                           [142, 88, 188, 57, 199, 68, 168, 114], [116, 162, 77, 188, 68, 179, 94, 140],
                           [136, 105, 162, 88, 168, 94, 150, 120], [125, 136, 116, 142, 114, 140, 120, 131]], np.uint8)


def frame(content, H, W, seed=0):
    """uint8 [H, W, 3]"""
    rng = np.random.default_rng([seed, H, W])
    yy, xx = np.mgrid[0:H, 0:W]
    if content == 'noise':
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if content == 'white':
        return np.full((H, W, 3), 255, np.uint8)
    if content == 'black':
        return np.zeros((H, W, 3), np.uint8)
    if content == 'gradient':
        r = 255.0 * xx / max(W - 1, 1)
        g = 255.0 * yy / max(H - 1, 1)
        b = 255.0 * (xx + yy) / max(H + W - 2, 1)
        return np.stack([r, g, 255.0 - b], -1).astype(np.uint8)
    if content == 'disc':
        inside = (yy - (H - 1) / 2) ** 2 + (xx - (W - 1) / 2) ** 2 <= (0.35 * min(H, W)) ** 2
        out = np.full((H, W, 3), 255, np.uint8)
        out[inside] = (200 - 3 * seed, 60, 30 + 5 * seed)
        return out
    if content == 'zigzag63':
        tile = np.tile(ZIGZAG63_BLOCK, ((H + 7) // 8, (W + 7) // 8))[:H, :W]
        return np.repeat(tile[:, :, None], 3, axis=2)
    if content == 'checker':                                             # full swing from pixel to pixel: the largest categories
        c = (((yy + xx + seed) & 1) * 255).astype(np.uint8)
        return np.stack([c, c, 255 - c], -1)
    raise KeyError(content)


def batch(content, H, W, N):
    """uint8 [N, H, W, 3], a different frame per index where the content allows it"""
    return np.stack([frame(content, H, W, seed=i) for i in range(N)])


def one_row(W, subsampling):
    m = 16 if subsampling == '420' else 8
    return (W + m - 1) // m


def encoder_cases():
    """(id, content, H, W, N, quality, subsampling, Ri or None).  Every size with every subsampling and every interval on noise, three
    different frames a batch; every quality on the two larger sizes; every content; N = 1; batches of more restart intervals than
    the 256 threads of the one-workgroup scan that places them (csrc/codec_stream.h), so that a thread takes a run of them."""
    out = []
    for H, W in SIZES:
        for sub in SUBSAMPLINGS:
            for ri in (1, 3, None):
                out.append(('noise', H, W, 3, 75, sub, ri))
    for H, W in [(40, 56), (64, 64)]:
        for sub in SUBSAMPLINGS:
            out.append(('noise', H, W, 1, 50, sub, None))
            out.append(('noise', H, W, 3, 100, sub, 3))                  # noise at quality 100: the slot-capacity case
    for sub in SUBSAMPLINGS:
        for content in ('white', 'black'):
            out.append((content, 17, 23, 1, 75, sub, 1))
            out.append((content, 64, 64, 3, 100, sub, None))
        for content in ('gradient', 'disc'):
            out.append((content, 64, 64, 3, 50, sub, None))
            out.append((content, 40, 56, 3, 75, sub, 3))
            out.append((content, 17, 23, 1, 100, sub, 1))
        out.append(('zigzag63', 16, 16, 1, 100, sub, None))
        out.append(('zigzag63', 17, 23, 3, 100, sub, 1))
        out.append(('checker', 64, 64, 3, 100, sub, None))
        out.append(('checker', 17, 23, 3, 75, sub, 1))
        out.append(('checker', 40, 56, 1, 50, sub, 3))
    out.append(('noise', 8, 2056, 1, 75, '444', 1))                      # 257 intervals: runs of 2, one of 1, empty threads behind
    out.append(('noise', 72, 72, 4, 75, '444', 1))                       # 4 x 81: frames begin and end in the middle of a run
    out.append(('noise', 16, 128, 16, 75, '444', 1))                     # 16 x 32 = 512: every thread a full run of 2
    out.append(('noise', 8, 128, 16, 75, '444', 1))                      # 16 x 16 = 256: exactly one interval per thread
    return [('-'.join(str(v) for v in c), ) + c for c in out]
