"""CPU: the Motion-JPEG AVI writer (decomp/nerfactor/util/mjpeg.py: AviWriter) fed with JPEG files of the float64 model
(tests/jpeg_model.py).  No independent AVI reader exists on the machines this runs on (no cv2, ffmpeg, imageio or av), so the check is a
struct-level walk of the RIFF tree written here from the AVI 1.0 layout: every size adds up, `dwTotalFrames` / `dwLength` are the frame
count, every `idx1` entry points at a `00dc` chunk of the stated length, and every chunk decodes with PIL to size_wh."""
import io
import struct

import pytest
from PIL import Image

from tests import jpeg_cases as cases
from tests import jpeg_model as jm
from vqnerf_release_amd.decomp.nerfactor.util import mjpeg


def _chunks(data, start, end):
    """[(fourcc, payload offset, size)] of the chunks in data[start:end]; chunks are padded to even length"""
    out, i = [], start
    while i < end:
        fourcc, size = data[i:i + 4], struct.unpack('<I', data[i + 4:i + 8])[0]
        out.append((fourcc, i + 8, size))
        i += 8 + size + (size & 1)
    assert i == end, (i, end)
    return out


def walk(data):
    """-> dict of what the file says; asserts that the tree is consistent"""
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    top = _chunks(data, 12, len(data))
    assert [c[0] for c in top] == [b'LIST', b'LIST', b'idx1']
    (_, hdrl_at, hdrl_n), (_, movi_at, movi_n), (_, idx_at, idx_n) = top
    assert data[hdrl_at:hdrl_at + 4] == b'hdrl' and data[movi_at:movi_at + 4] == b'movi'
    hdrl = _chunks(data, hdrl_at + 4, hdrl_at + hdrl_n)
    assert [c[0] for c in hdrl] == [b'avih', b'LIST'] and hdrl[0][2] == 56
    avih = struct.unpack('<14I', data[hdrl[0][1]:hdrl[0][1] + 56])
    assert data[hdrl[1][1]:hdrl[1][1] + 4] == b'strl'
    strl = _chunks(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [c[0] for c in strl] == [b'strh', b'strf'] and strl[0][2] == 56 and strl[1][2] == 40
    strh = struct.unpack('<4s4sIHHIIIIIIII4H', data[strl[0][1]:strl[0][1] + 56])
    strf = struct.unpack('<IiiHH4sIiiII', data[strl[1][1]:strl[1][1] + 40])
    frames = _chunks(data, movi_at + 4, movi_at + movi_n)
    assert all(c[0] == b'00dc' for c in frames)
    assert idx_n == 16 * len(frames)
    index = [struct.unpack('<4sIII', data[idx_at + 16 * i:idx_at + 16 * i + 16]) for i in range(len(frames))]
    for (fourcc, flags, off, size), (_, at, n) in zip(index, frames):
        assert fourcc == b'00dc' and flags == 0x10 and size == n
        assert movi_at + off == at - 8 and data[movi_at + off:movi_at + off + 4] == b'00dc'     # offsets count from the 'movi' fourcc
    return dict(usec=avih[0], flags=avih[3], total=avih[4], streams=avih[6], largest=avih[7], w=avih[8], h=avih[9], type=strh[0], handler=strh[1],
                scale=strh[6], rate=strh[7], length=strh[9], rect=strh[13:], bi=strf, frames=[data[at:at + n] for _, at, n in frames])


def _jpegs(H, W, n):
    return [jm.encode(cases.frame('noise' if i % 2 else 'disc', H, W, seed=i), 75, '420') for i in range(n)]


@pytest.mark.parametrize('n', [0, 1, 5])
def test_riff_tree_is_consistent_and_every_chunk_decodes(tmp_path, n):
    H, W = 17, 23
    jpegs = _jpegs(H, W, n)
    path = str(tmp_path / 'sub' / 'v.avi')
    with mjpeg.AviWriter(path, (W, H), fps=20) as avi:
        for j in jpegs:
            avi.write(j)
    d = walk(open(path, 'rb').read())
    assert d['total'] == n and d['length'] == n and d['streams'] == 1 and d['flags'] & 0x10
    assert (d['w'], d['h']) == (W, H) and d['rect'] == (0, 0, W, H)
    assert d['type'] == b'vids' and d['handler'] == b'MJPG' and (d['scale'], d['rate'], d['usec']) == (1, 20, 50000)
    assert d['bi'][:7] == (40, W, H, 1, 24, b'MJPG', W * H * 3)
    assert d['largest'] == max([len(j) for j in jpegs], default=0)
    assert d['frames'] == jpegs
    for f in d['frames']:
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (W, H)


def test_odd_length_chunks_are_padded(tmp_path):
    jpegs = _jpegs(8, 8, 6)
    odd = [j for j in jpegs if len(j) & 1] or [jpegs[0][:-2] + b'\x00' * (1 - (len(jpegs[0]) & 1)) + b'\xff\xd9']
    even = [j for j in jpegs if not len(j) & 1]
    seq = [odd[0], (even or odd)[0], odd[0]]
    assert len(seq[0]) & 1
    path = str(tmp_path / 'v.avi')
    avi = mjpeg.AviWriter(path, (8, 8), fps=12.5)
    for j in seq:
        avi.write(j)
    avi.close()
    avi.close()                                                      # closing twice is harmless
    data = open(path, 'rb').read()
    d = walk(data)                                                   # (the walk steps over the pad bytes and checks the index offsets)
    assert d['frames'] == seq and len(data) % 2 == 0
    assert (d['scale'], d['rate'], d['usec']) == (1000, 12500, 80000)
    with pytest.raises(ValueError, match='write after close'):
        avi.write(seq[0])


def test_refuses_to_pass_two_gib(tmp_path, monkeypatch):
    jpegs = _jpegs(8, 8, 3)
    assert mjpeg.AviWriter.MAX_BYTES == 2 ** 31 - 1
    path = str(tmp_path / 'v.avi')
    avi = mjpeg.AviWriter(path, (8, 8))
    avi.write(jpegs[0])
    room = avi.pos + (8 + len(jpegs[1]) + (len(jpegs[1]) & 1)) + 8 + 16 * 2      # the file as close() would leave it after frame 1
    monkeypatch.setattr(mjpeg.AviWriter, 'MAX_BYTES', room)
    avi.write(jpegs[1])                                                          # exactly at the limit: fits
    with pytest.raises(ValueError, match='past .* bytes'):
        avi.write(jpegs[2])
    avi.close()
    data = open(path, 'rb').read()
    assert len(data) == room and walk(data)['frames'] == jpegs[:2]               # the refused frame left no trace
