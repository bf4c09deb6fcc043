"""CPU: the float64 JPEG model (tests/jpeg_model.py), the yardstick of the device encoder, against PIL (libjpeg), the only
independent JPEG code on the machines this runs on.

* PIL opens the model's files at every size and subsampling, with every restart interval, and reports the tables of the IJG rule.
* The model's Huffman tables are the ones libjpeg writes by default (Annex K).
* '444': PIL's decoded pixels against a float decode of the model's own coefficients (float IDCT, samples rounded and limited to
  0 .. 255 as libjpeg limits them, float JFIF colour conversion, rounded).  libjpeg's integer IDCT and fixed-point colour conversion
  explain what is left: OBSERVED_DECODE levels at most over the case list, and twice that is asserted.
* Against PIL's own encoder at equal quality and subsampling, the PSNR of the model's file to the source may be lower by at most twice
  the largest shortfall observed at that size and subsampling (OBSERVED_SHORTFALL, dB; both files decoded by PIL); where the model was
  never observed to be worse it must not be worse.  (The 2 - 3 dB at '444' are the full-swing checkerboard, whose samples libjpeg
  limits after the inverse transform; at a single pixel one level is 3 dB.)
`python tests/test_jpeg_model.py` measures both again and writes profiles/observed_errors_jpeg.json."""
import io
import json
import os

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_cases as cases
from tests import jpeg_model as jm

SIZES = [(1, 1), (8, 8), (17, 23), (40, 56)]
CONTENTS = ['noise', 'gradient', 'disc', 'checker']
QUALITIES = [50, 75, 90, 100]
PIL_SUBSAMPLING = {'444': 0, '420': 2}
OBSERVED_DECODE = 3                                                  # levels, measured over SIZES x CONTENTS x QUALITIES at '444'
OBSERVED_SHORTFALL = {('444', 1, 1): 3.0103, ('444', 8, 8): 2.2725, ('444', 17, 23): 1.9993, ('444', 40, 56): 2.2725,
                      ('420', 1, 1): 3.0103, ('420', 8, 8): 0.3925, ('420', 17, 23): 0.1898, ('420', 40, 56): 0.0791}      # dB


def _decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return np.inf if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def float_decode(rgb, quality, subsampling):
    """what a decoder with a float IDCT makes of the model's coefficients of `rgb` ('444')"""
    coef, _ = jm.coefficients(rgb, quality, subsampling)
    ql, qc = jm.quant_tables(quality)
    planes = []
    for k, table in zip(('y', 'cb', 'cr'), (ql, qc, qc)):
        c = np.zeros(coef[k].shape)
        c[..., jm.ZIGZAG] = coef[k]
        c = (c * table).reshape(c.shape[0], c.shape[1], 8, 8)
        b = np.einsum('uy,abuv,vx->abyx', jm.DCT, c, jm.DCT) + 128
        planes.append(np.clip(np.rint(b.transpose(0, 2, 1, 3).reshape(c.shape[0] * 8, c.shape[1] * 8)), 0, 255))
    Y, Cb, Cr = planes
    out = np.stack([Y + 1.402 * (Cr - 128), Y - 0.344136286 * (Cb - 128) - 0.714136286 * (Cr - 128), Y + 1.772 * (Cb - 128)], -1)
    return np.clip(np.rint(out), 0, 255)[:rgb.shape[0], :rgb.shape[1]]


@pytest.mark.parametrize('sub', cases.SUBSAMPLINGS)
@pytest.mark.parametrize('H,W', SIZES)
def test_pil_opens_the_files_and_reports_the_ijg_tables(H, W, sub):
    for quality in (1, 50, 90, 100):
        for ri in (1, 3, None):
            x = cases.frame('noise', H, W, seed=quality)
            im = _decode(jm.encode(x, quality, sub, ri))
            assert im.size == (W, H) and im.mode == 'RGB' and np.asarray(im).shape == (H, W, 3)
            ql, qc = jm.quant_tables(quality)
            assert [list(im.quantization[0]), list(im.quantization[1])] == [ql.tolist(), qc.tolist()]
    # the rule against libjpeg's own scaling
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', quality=90)
    q = Image.open(buf).quantization
    ql, qc = jm.quant_tables(90)
    assert [list(q[0]), list(q[1])] == [ql.tolist(), qc.tolist()]


def _dht(data):
    out, i = {}, 2
    while data[i + 1] != 0xda:
        n = int.from_bytes(data[i + 2:i + 4], 'big')
        if data[i + 1] == 0xc4:
            s = data[i + 4:i + 2 + n]
            while s:
                k = sum(s[1:17])
                out[s[0]] = (list(s[1:17]), bytes(s[17:17 + k]))
                s = s[17 + k:]
        i += 2 + n
    return out


def test_huffman_tables_are_the_ones_libjpeg_writes():
    buf = io.BytesIO()
    Image.fromarray(cases.frame('noise', 16, 16)).save(buf, 'JPEG', quality=75)
    want = {0x00: (jm.DC_BITS[0], bytes(jm.DC_VALS)), 0x01: (jm.DC_BITS[1], bytes(jm.DC_VALS)), 0x10: (jm.AC_BITS[0], jm.AC_VALS[0]),
            0x11: (jm.AC_BITS[1], jm.AC_VALS[1])}
    assert _dht(buf.getvalue()) == want
    assert _dht(jm.encode(cases.frame('noise', 16, 16))) == want
    assert jm.AC_CODES[0][0xf0] == (0x7f9, 11) and jm.AC_CODES[1][0xf0] == (0x3fa, 10)            # ZRL
    assert jm.AC_CODES[0][0x00] == (0xa, 4) and jm.AC_CODES[1][0x00] == (0, 2)                    # EOB


def test_restart_intervals_stand_alone():
    """every interval but the last is followed by RSTm, m cycling; each decodes to the same pixels whatever Ri is"""
    x = cases.frame('noise', 17, 23)
    ref = np.asarray(_decode(jm.encode(x, 75, '444', 1)))
    for ri in (2, 3, 9, 100):
        assert np.array_equal(np.asarray(_decode(jm.encode(x, 75, '444', ri))), ref)
    scan = jm.entropy_encode(jm.coefficients(x, 75, '444')[0], 1, '444')
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xff and 0xd0 <= scan[i + 1] <= 0xd7]
    assert marks == [0xd0 + i % 8 for i in range(8)]                 # 9 intervals: the counter wraps


def test_zigzag63_block_codes_three_zrl_and_no_eob():
    x = cases.frame('zigzag63', 8, 8)
    coef, raw = jm.coefficients(x, 100, '444')
    y = coef['y'][0, 0]
    assert y[63] == 294 and not y[1:63].any() and np.abs(raw['y'][0, 0][1:63]).max() < 0.36
    w = jm._Bits()
    jm._block(w, y, int(y[0]), 0)                                    # DC difference 0: 2 bits; 3 ZRL of 11; code 0xE9 (16) + 9 bits
    assert 8 * len(bytes(w.out).replace(b'\xff\x00', b'\xff')) + w.n == 2 + 3 * 11 + jm.AC_CODES[0][0xe9][1] + 9


def measure():
    decode, shortfall = {}, {}
    for sub in cases.SUBSAMPLINGS:
        for H, W in SIZES:
            for content in CONTENTS:
                for q in QUALITIES:
                    x = cases.frame(content, H, W, seed=1)
                    a = np.asarray(_decode(jm.encode(x, q, sub)))
                    if sub == '444':
                        k = f'{content}-q{q}'
                        decode[k] = max(decode.get(k, 0), int(np.abs(a.astype(int) - float_decode(x, q, sub)).max()))
                    buf = io.BytesIO()
                    Image.fromarray(x).save(buf, 'JPEG', quality=q, subsampling=PIL_SUBSAMPLING[sub])
                    pm, pp = _psnr(a, x), _psnr(np.asarray(_decode(buf.getvalue())), x)
                    if np.isfinite(pm) and np.isfinite(pp):                 # (a file that decodes exactly has no PSNR: 1 x 1 only)
                        shortfall[(sub, H, W)] = max(shortfall.get((sub, H, W), -np.inf), float(pp - pm))
    return decode, shortfall


@pytest.fixture(scope='module')
def measured():
    return measure()


def test_pil_decode_is_within_what_a_float_decode_explains(measured):
    decode, _ = measured
    print('[observed] largest |PIL decode - float decode| per content and quality:', decode)
    assert max(decode.values()) <= 2 * OBSERVED_DECODE


def test_psnr_is_not_below_libjpegs_own_encoder(measured):
    _, shortfall = measured
    for key, s in shortfall.items():
        seen = OBSERVED_SHORTFALL[key]
        print(f'[observed] {key}: PIL encode is ahead by at most {s:.4f} dB (bound {2 * max(seen, 0):.4f})')
        assert s <= 2 * max(seen, 0.0), (key, s, seen)


if __name__ == '__main__':
    decode, shortfall = measure()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'observed_errors_jpeg.json')
    with open(path, 'w') as f:
        json.dump({'what': 'tests/test_jpeg_model.py: the float64 JPEG model against PIL (libjpeg)',
                   'pil_decode_minus_float_decode_levels_444': decode, 'asserted_levels': 2 * OBSERVED_DECODE,
                   'pil_encode_psnr_minus_model_psnr_db': {'-'.join(map(str, k)): v for k, v in shortfall.items()},
                   'asserted_db': {'-'.join(map(str, k)): 2 * max(v, 0.0) for k, v in OBSERVED_SHORTFALL.items()}}, f, indent=1)
    print('wrote', path)
