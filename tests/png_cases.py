"""Images and case lists shared by the PNG tests (tests/test_png_model.py on the CPU, tests/test_gpu_png.py on the device), and the
model's files of a case, computed once per process."""
import functools

import numpy as np

from tests import png_model as model

SHAPES = [(1, 1), (1, 7), (5, 1), (3, 5), (16, 16), (33, 17), (64, 64)]       # (H, W)
FORCED = ['none', 'sub', 'up', 'average', 'paeth']
ZERO_RUNS = [2, 3, 4, 257, 258, 259, 517]


def zero_run_row():
    """one row of bytes: runs of exactly ZERO_RUNS zeros between groups of eight non-zero bytes that repeat nowhere (eight: no short
    candidate distance reaches from a run back into the run before).  Under 'none' a run of r zeros is a literal and matches at
    distance 1 of r - 1 bytes in all: none (2, 3), 3, 256, 257, 258 (the longest), 258 + 258"""
    out = []
    for k, r in enumerate(ZERO_RUNS):
        out += [11 + k, 37 + k, 59 + k, 83 + k, 101 + k, 131 + k, 151 + k, 173 + k] + [0] * r
    return np.array(out + [9, 99, 199], np.uint8)


def image(content, H, W, C, seed=0):
    """uint8 [H, W, C]"""
    rng = np.random.default_rng([seed, H, W, C])
    yy, xx = np.mgrid[0:H, 0:W]
    if content == 'noise':
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if content in ('zeros', 'full'):
        return np.full((H, W, C), 0 if content == 'zeros' else 255, np.uint8)
    if content == 'gradient':
        planes = [255.0 * xx / max(W - 1, 1), 255.0 * yy / max(H - 1, 1), 255.0 - 255.0 * (xx + yy) / max(H + W - 2, 1), 128.0 + 0 * xx]
        return np.stack(planes[:C], -1).astype(np.uint8)
    if content == 'disc':                                                 # shaded, over white; alpha (C = 2, 4) its coverage
        r2 = (yy - (H - 1) / 2) ** 2 + (xx - (W - 1) / 2) ** 2
        inside = r2 <= (0.4 * min(H, W)) ** 2
        shade = np.clip(230.0 - 6.0 * np.sqrt(r2) + 4 * seed, 0, 255)
        planes = [np.where(inside, shade * f, 255.0) for f in (1.0, 0.6, 0.3)]
        planes = planes[:C - 1 if C in (2, 4) else C] + ([np.where(inside, 255.0, 0.0)] if C in (2, 4) else [])
        return np.stack(planes, -1).astype(np.uint8)
    if content == 'checker':
        c = (((yy + xx + seed) & 1) * 255).astype(np.uint8)
        return np.stack([c, 255 - c, c, c][:C], -1)
    if content == 'stripes':
        c = ((xx + seed) % 3 * 100).astype(np.uint8)
        return np.stack([c, c + 1, c + 2, c + 3][:C], -1)
    if content == 'same_rows':
        row = rng.integers(0, 256, (1, W, C), dtype=np.uint8)
        return np.repeat(row, H, axis=0)
    if content == 'zero_runs':
        row = zero_run_row()
        assert (H, W * C) == (H, len(row)), (H, W, C, len(row))
        return np.repeat(row.reshape(1, W, C), H, axis=0)
    raise KeyError(content)


def batch(content, H, W, C, N):
    return np.stack([image(content, H, W, C, seed=i) for i in range(N)])


def encoder_cases():
    """(id, content, H, W, C, N, filters, rows_per_segment: an int, 'all' or None).  Every shape with every channel count under the
    adaptive filter and the default segments; every forced filter and every segment length on the shapes of more than one row; every
    content; the row of the largest stride; the runs at the length-code boundaries; runs and match sources across segment ends;
    batches of at least as many images as the 256 threads of the one-workgroup scan that places them (csrc/codec_stream.h)."""
    out = []
    for H, W in SHAPES:
        for C in (1, 2, 3, 4):
            out.append(('noise' if (H + W + C) % 2 else 'gradient', H, W, C, 3 if C == 3 else 1, 'adaptive', None))
    for H, W in [(3, 5), (33, 17), (64, 64)]:
        for i, f in enumerate(FORCED):
            out.append(('disc', H, W, 1 + i % 4, 1, f, [1, 2, 'all', None][i % 4]))
            out.append(('gradient', H, W, 4 - i % 4, 3, f, [2, 'all', None, 1][i % 4]))
        for rows in (1, 2, 'all'):
            out.append(('disc', H, W, 3, 1, 'adaptive', rows))
    for content in ('zeros', 'full', 'noise', 'gradient', 'disc', 'checker', 'stripes', 'same_rows'):
        out.append((content, 64, 64, 3, 3, 'adaptive', None))
        out.append((content, 33, 17, 1, 1, 'adaptive', 2))
        out.append((content, 16, 16, 4, 1, 'none', 1))
    out.append(('noise', 2, 65534, 1, 1, 'adaptive', 1))                  # stride 65535: the limit
    out.append(('disc', 2, 65534, 1, 1, 'sub', None))
    W = len(zero_run_row())
    out.append(('zero_runs', 1, W, 1, 1, 'none', None))
    out.append(('zero_runs', 3, W, 1, 1, 'none', 1))                      # ... and every row after the first a copy of the segment before
    out.append(('zeros', 4, 40, 1, 1, 'none', 1))                         # a run cut by every segment end
    out.append(('zeros', 7, 300, 1, 1, 'none', 2))                        # ... by matches of 258 and by the end
    out.append(('same_rows', 6, 23, 3, 1, 'none', 1))                     # match sources in the previous segment only
    out.append(('same_rows', 6, 23, 3, 3, 'none', 2))
    out.append(('noise', 1, 1, 1, 257, 'none', None))                     # a scan thread takes two images, the last threads none
    out.append(('noise', 2, 3, 1, 256, 'none', 1))                        # one image per thread, two segments each
    out = list(dict.fromkeys(out))                                        # (a case two of the rules name is one case)
    return [('-'.join(str(v) for v in c), ) + c for c in out]


def rows_of(rows, H):
    return H if rows == 'all' else rows


@functools.lru_cache(maxsize=None)
def expected(content, H, W, C, N, filters, rows):
    """-> (the batch uint8 [N, H, W, C], the model's filtered streams [N, H, stride], its files): computed once, shared, read only"""
    frames = batch(content, H, W, C, N)
    filtered = np.stack([model.filter_rows(f, filters)[0] for f in frames])
    files = tuple(model.png_file(f, filters, rows_of(rows, H)) for f in frames)
    frames.setflags(write=False), filtered.setflags(write=False)
    return frames, filtered, files
