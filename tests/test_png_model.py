"""CPU: the stream format of the device PNG encoder as tests/png_model.py states it, checked on its own: the files against PIL and
zlib, the filters against a separate decoder, the prefabricated tables (scripts/make_png_tables.py, csrc/png_plan.h), and the sizes.
Sizes against zlib and PIL at level 3 are written to profiles/observed_png_sizes.json by `python -m tests.test_png_model`; they are
recorded, not asserted."""
import io
import json
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_cases as cases
from tests import png_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {1: 'L', 2: 'LA', 3: 'RGB', 4: 'RGBA'}
CASES = [c for c in cases.encoder_cases() if c[2] * c[3] <= 4096]              # (the two rows of 65534 pixels: the GPU test's)


@pytest.mark.parametrize('name,content,H,W,C,N,filters,rows', CASES, ids=[c[0] for c in CASES])
def test_files_open_and_inflate_to_the_filtered_stream(name, content, H, W, C, N, filters, rows):
    frames, filtered, files = cases.expected(content, H, W, C, N, filters, rows)
    for i in range(N):
        img = Image.open(io.BytesIO(files[i]))
        assert img.mode == MODES[C] and img.size == (W, H)
        assert np.array_equal(np.asarray(img).reshape(H, W, C), frames[i])
        chunks = model.chunks(files[i])
        assert [k for k, _, _ in chunks] == [b'IHDR', b'IDAT', b'IEND'] and all(ok for _, _, ok in chunks)
        assert chunks[0][1] == struct.pack('>IIBBBBB', W, H, 8, model.COLOUR_TYPE[C], 0, 0, 0)
        assert files[i][:33] == model.head(H, W, C)
        idat = chunks[1][1]
        assert idat[:2] == b'\x78\x01'
        assert zlib.decompress(idat) == filtered[i].tobytes()
        assert np.array_equal(model.unfilter_rows(filtered[i], C), frames[i].reshape(H, W * C))
        if filters != 'adaptive':
            assert (filtered[i][:, 0] == model.FILTERS[filters]).all()


def test_segment_sizes_are_bounded_and_noise_falls_back():
    for name, content, H, W, C, N, filters, rows in CASES:
        frames, filtered, _ = cases.expected(content, H, W, C, N, filters, rows)
        r = cases.rows_of(rows, H) or model.default_rows_per_segment(1 + W * C)
        stride = 1 + W * C
        b = filtered[0].reshape(-1)
        choices = []
        for y in range(0, H, r):
            end = min(y + r, H)
            data, choice = model.encode_segment(b, y * stride, end * stride, stride, C, end == H)
            assert len(data) <= (end - y) * stride + 5, (name, y)
            choices.append(choice)
        if content == 'noise' and filters == 'none' and W * C >= 64:
            assert set(choices) == {len(model.tables())}, (name, choices)           # stored
        if content == 'zeros':
            assert len(model.tables()) not in choices, (name, choices)


def _adaptive_rows():
    """six rows of one channel, built so that each type wins once and the last row ties: (rows, the types expected)"""
    W = 16
    rng = np.random.default_rng(5)
    img = np.zeros((6, W), np.uint8)
    img[0] = [3, 253, 2, 254, 1, 255, 2, 254, 3, 253, 1, 255, 2, 254, 3, 253]      # small residuals as they are, large differences: none
    img[1] = 100 + np.arange(W)                                                     # a ramp: sub
    img[2] = img[1]                                                                 # a copy of the row above: up (sub leaves 1s)
    img[3] = rng.integers(0, 256, W)                                                # (a row for the next one to stand on)
    img[4] = rng.integers(0, 256, W)
    img[5] = 0
    return img


def test_adaptive_choice_and_tie():
    img = _adaptive_rows()
    _, types = model.filter_rows(img, 'adaptive')
    assert list(types[:3]) == [0, 1, 2], types
    # average and paeth: rows made from the predictor itself (plus a small residual for average)
    W = 24
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (1, W), dtype=np.int64)
    small = rng.integers(-1, 2, W)
    avg, pae = np.zeros(W, np.int64), np.zeros(W, np.int64)
    for x in range(W):
        left, up = (avg[x - 1] if x else 0), base[0, x]
        avg[x] = ((left + up) // 2 + small[x]) & 255
        a, b, c = (pae[x - 1] if x else 0), base[0, x], (base[0, x - 1] if x else 0)
        pae[x] = int(model._paeth(np.int64(a), np.int64(b), np.int64(c))) if x else 90          # the predictor itself: paeth costs 90
    for row, want in ((avg, 3), (pae, 4)):
        _, types = model.filter_rows(np.concatenate([base, row[None]]).astype(np.uint8), 'adaptive')
        assert types[1] == want, (types, want)
    # a tie: a first row of zeros costs nothing under every type -> the lowest; a constant first row ties none / up / (not sub)
    _, types = model.filter_rows(np.zeros((2, 9), np.uint8), 'adaptive')
    assert list(types) == [0, 0]
    _, types = model.filter_rows(np.full((1, 9), 7, np.uint8), 'adaptive')
    assert types[0] == 1                                                           # sub: 7 then zeros; none and up cost 63
    _, types = model.filter_rows(np.array([[5, 0, 0, 0]], np.uint8), 'adaptive')
    assert types[0] == 0                                                           # none, sub, up, paeth all cost 5 (sub: 5 + 5): the lowest


def test_tables_are_complete_within_the_limits_and_inflate():
    tabs = model.tables()
    assert len(tabs) == 15
    gen = model._generator()
    for (lit, dist, cl), t in zip(gen.tables(), tabs):
        assert len(lit) == 288 and lit[286:] == [0, 0] and len(dist) == 30 and len(cl) == 19
        assert all(1 <= n <= 15 for n in lit[:286]) and all(1 <= n <= 15 for n in dist) and all(0 <= n <= 7 for n in cl)
        for lens in (lit, dist, cl):
            assert sum(1 << (15 - n) for n in lens if n) == 1 << 15                 # Kraft sum exactly 1
    # a block of every literal, every length and every candidate distance symbol under each table inflates
    rng = np.random.default_rng(3)
    data = np.concatenate([np.arange(256), rng.integers(0, 4, 3000), np.zeros(700, np.int64), np.arange(256)]).astype(np.uint8)
    for i, t in enumerate(tabs):
        tokens = model.tokenize(data, 0, len(data), 300, 3)
        out = model.Bits()
        out.put(1, 1)
        out.bits.extend(t.header.bits)
        for tok in tokens:
            if tok[0] == 'lit':
                out.code(t.lit_codes[tok[1]], t.lit_lens[tok[1]])
            else:
                k, e = model._len_symbol(tok[1])
                j, f = model._dist_symbol(tok[2])
                out.code(t.lit_codes[257 + k], t.lit_lens[257 + k]), out.put(e, model.LEN_EXTRA[k])
                out.code(t.dist_codes[j], t.dist_lens[j]), out.put(f, model.DIST_EXTRA[j])
        out.code(t.lit_codes[256], t.lit_lens[256])
        assert zlib.decompress(out.tobytes(), wbits=-15) == data.tobytes(), i
        assert any(tok[0] == 'match' and tok[2] > 8 for tok in tokens) and any(tok[0] == 'match' and tok[1] == 258 for tok in tokens)


def test_the_generator_reproduces_the_constants_of_the_header():
    gen = model._generator()
    assert gen.header_block() == gen.generated_block()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'make_png_tables.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    src = open(os.path.join(ROOT, 'vqnerf_release_amd', 'csrc', 'png_plan.h')).read()
    assert int(re.search(r'kPngTables = (\d+);', src).group(1)) == len(model.tables()) - 1


def test_tokens_follow_the_stated_rules():
    row = cases.zero_run_row()
    f, _ = model.filter_rows(row.reshape(1, -1, 1), 'none')
    tokens = model.tokenize(f.reshape(-1), 0, f.size, f.shape[1], 1)
    matches = [t[1] for t in tokens if t[0] == 'match']
    assert matches == [3, 256, 257, 258, 258, 258], matches                        # runs of 4, 257, 258, 259 and 517 zeros
    assert all(t[2] == 1 for t in tokens if t[0] == 'match')
    # the source of a match may lie in the segment before; a dropped candidate (in front of the image) is never taken
    img = cases.image('same_rows', 3, 23, 3)
    f, _ = model.filter_rows(img, 'none')
    b, stride = f.reshape(-1), f.shape[1]
    assert model.tokenize(b, stride, 2 * stride, stride, 3) == [('match', stride, stride)]
    assert all(t[0] == 'lit' or t[2] < stride for t in model.tokenize(b, 0, stride, stride, 3))
    # the cap at the segment end
    z = np.zeros(600, np.uint8)
    assert model.tokenize(z, 300, 600, 100, 1)[:2] == [('match', 258, 1), ('match', 42, 1)]


def observed_sizes():
    out = {}
    for name, content, H, W, C, N, filters, rows in CASES:
        frames, filtered, files = cases.expected(content, H, W, C, N, filters, rows)
        pil = io.BytesIO()
        Image.fromarray(frames[0].reshape(H, W, C) if C > 1 else frames[0].reshape(H, W)).save(pil, format='PNG', compress_level=3)
        idat = model.chunks(files[0])[1][1]
        out[name] = {'filtered_bytes': int(filtered[0].size), 'model_zlib_bytes': len(idat),
                     'zlib_level3_bytes': len(zlib.compress(filtered[0].tobytes(), 3)), 'model_file_bytes': len(files[0]),
                     'pil_level3_file_bytes': len(pil.getvalue())}
    return out


if __name__ == '__main__':
    path = os.path.join(ROOT, 'profiles', 'observed_png_sizes.json')
    with open(path, 'w') as f:
        json.dump({'note': 'model bytes of the first image of each case of tests/png_cases.py against zlib.compress(filtered, 3) and '
                           'PIL compress_level=3; recorded, not asserted', 'cases': observed_sizes()}, f, indent=1)
    print('wrote', path)
