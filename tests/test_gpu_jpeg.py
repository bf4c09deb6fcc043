"""GPU: the device JPEG encoder (csrc/jpeg_encode.hip through decomp/nerfactor/util/mjpeg.py) against its float64 statement
(tests/jpeg_model.py) on the cases of tests/jpeg_cases.py.

1. Coefficients: equal to the model's wherever the model's unrounded |coef / q| is farther than 2e-3 from a half-integer (an f32 DCT of
   values up to 1024 is good to about 1e-4; inside the band either rounding is right); at most 1 % of a case's coefficients may fall
   into the band.
2. Bitstream: the scan of every frame equals model.entropy_encode(device coefficients, Ri) byte for byte (integer work: exact), and
   the file equals the model's header + that scan + EOI.
3. PIL (libjpeg) decodes every file to [H, W, 3].
4. Two runs give the same bytes; what the planner refuses raises ValueError with its reason and launches nothing; CPU tensors raise."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_cases as cases
from tests import jpeg_model as model
from tests.gpu_util import launches
from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.util import mjpeg

pytestmark = pytest.mark.gpu
BAND = 2e-3
CASES = cases.encoder_cases()


@pytest.mark.parametrize('name,content,H,W,N,quality,sub,ri', CASES, ids=[c[0] for c in CASES])
def test_encoder_against_the_model(name, content, H, W, N, quality, sub, ri):
    frames = cases.batch(content, H, W, N)
    enc = mjpeg.JpegEncoder(quality=quality, subsampling=sub, restart_interval=ri)
    dev = torch.tensor(frames).cuda()
    files, coef = enc.encode(dev, want_coefficients=True)
    alone = enc.coefficients(dev)
    Ri = cases.one_row(W, sub) if ri is None else ri
    assert len(files) == N
    n_all = n_band = 0
    for i in range(N):
        want, raw = model.coefficients(frames[i], quality, sub)
        got = {k: v[i].cpu().numpy() for k, v in coef.items()}
        for k in ('y', 'cb', 'cr'):
            assert got[k].shape == want[k].shape and got[k].dtype == np.int16, (k, got[k].shape, want[k].shape)
            assert np.array_equal(got[k], alone[k][i].cpu().numpy()), k          # .coefficients() is the same first kernel
            a = np.abs(raw[k])
            decided = np.abs(a - np.floor(a) - 0.5) > BAND
            n_all, n_band = n_all + decided.size, n_band + int((~decided).sum())
            bad = decided & (got[k] != want[k])
            assert not bad.any(), (name, i, k, int(bad.sum()), got[k][bad][:4], want[k][bad][:4], raw[k][bad][:4])
        if content == 'zigzag63':                                                # three ZRL codes and no EOB in every Y block
            y = got['y'].reshape(-1, 64)[0]
            assert y[63] != 0 and not y[1:63].any(), y
        scan = model.entropy_encode(got, Ri, sub)
        head = model.header(H, W, quality, sub, Ri)
        assert files[i][:len(head)] == head, (name, i, 'header')
        assert files[i][-2:] == b'\xff\xd9'
        assert files[i][len(head):-2] == scan, (name, i, len(files[i]) - len(head) - 2, len(scan))
        img = np.asarray(Image.open(io.BytesIO(files[i])).convert('RGB'))
        assert img.shape == (H, W, 3)
    print(f'{name}: {n_band} of {n_all} coefficients within {BAND} of a half-integer')
    assert n_band <= 0.01 * n_all, (name, n_band, n_all)
    assert enc.encode(dev) == files                                              # the same bytes again


def test_rst_counter_wraps():
    frames = cases.batch('noise', 17, 23, 1)
    f = mjpeg.JpegEncoder(75, '444', 1).encode(torch.tensor(frames).cuda())[0]
    g, _ = _C.jpeg_plan(1, 17, 23, 75, 444, 1)
    assert g['intervals'] == 9
    scan = f[g['header_bytes']:-2]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xff and 0xd0 <= scan[i + 1] <= 0xd7]
    assert marks == [0xd0 + i % 8 for i in range(8)]


@pytest.mark.parametrize('kwargs,shape,reason', [
    (dict(), (0, 8, 8, 3), 'at least one frame'),
    (dict(), (1, 0, 8, 3), 'zero side'),
    (dict(), (1, 8, 0, 3), 'zero side'),
    (dict(quality=0), (1, 8, 8, 3), 'quality is 1 .. 100'),
    (dict(quality=101), (1, 8, 8, 3), 'quality is 1 .. 100'),
    (dict(restart_interval=0), (1, 8, 8, 3), 'restart interval is 1 .. 65535'),
    (dict(restart_interval=65536), (1, 8, 8, 3), 'restart interval is 1 .. 65535'),
    (dict(subsampling='422'), (1, 8, 8, 3), 'unknown subsampling'),
    (dict(subsampling='best'), (1, 8, 8, 3), 'unknown subsampling'),
])
def test_refusals_raise_and_launch_nothing(kwargs, shape, reason):
    x = torch.zeros(shape, dtype=torch.uint8, device='cuda')
    with launches() as rec:
        with pytest.raises(ValueError, match=reason):
            mjpeg.JpegEncoder(**kwargs).encode(x)
        with pytest.raises(ValueError, match=reason):
            mjpeg.JpegEncoder(**kwargs).coefficients(x)
    assert not rec.names                                                         # no entry point was even called


def test_buffers_smaller_than_the_plan_are_refused():
    g, _ = _C.jpeg_plan(1, 16, 16, 75, 420, 1)
    x = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device='cuda')
    scratch = torch.full((g['scratch_bytes'],), 0xab, dtype=torch.uint8, device='cuda')
    out = torch.full((g['out_bytes'],), 0xab, dtype=torch.uint8, device='cuda')
    meta = torch.full((1, 2), -7, dtype=torch.int64, device='cuda')
    with pytest.raises(_C.VqnError, match='byte total of up to .* over the buffer'):
        _C.jpeg_encode(x, g, scratch, out[:-1], meta)
    with pytest.raises(_C.VqnError, match='scratch holds'):
        _C.jpeg_encode(x, g, scratch[:g['scratch_bytes'] - 16], out, meta)
    torch.cuda.synchronize()
    assert bool((scratch == 0xab).all()) and bool((out == 0xab).all()) and bool((meta == -7).all())      # nothing ran


def test_cpu_tensors_raise():
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(_C.VqnError, match='no CPU fallback'):
        mjpeg.JpegEncoder().encode(x)
    with pytest.raises(_C.VqnError, match='no CPU fallback'):
        mjpeg.JpegEncoder().coefficients(x)


def test_scratch_is_kept_and_never_shrunk():
    enc = mjpeg.JpegEncoder()
    big = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device='cuda')
    enc.encode(big)
    key = [k for k in _C._scratch_cache if k[2] == 'jpeg'][0]
    buf = _C._scratch_cache[key][0]
    enc.encode(big[:1, :8, :8].contiguous())
    assert _C._scratch_cache[key][0] is buf                                       # the smaller batch reuses it
    assert len(enc._plans) == 2
