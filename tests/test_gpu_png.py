"""GPU: the device PNG encoder (csrc/png_encode.hip through decomp/nerfactor/util/png.py) against its statement in numpy
(tests/png_model.py) on the cases of tests/png_cases.py.  Integer work on both sides: everything is compared exactly.

1. `filtered` equals the model's filtered stream.
2. Every file equals the model's byte for byte.
3. PIL decodes every file to the input, in the mode of its channel count.
4. Two calls give equal bytes; what the planner refuses raises ValueError with its reason and launches nothing; buffers smaller than
   the plan's are refused; CPU tensors raise; the scratch is kept and never shrunk."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_cases as cases
from tests.gpu_util import launches
from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.util import png

pytestmark = pytest.mark.gpu
CASES = cases.encoder_cases()
MODES = {1: 'L', 2: 'LA', 3: 'RGB', 4: 'RGBA'}


@pytest.mark.parametrize('name,content,H,W,C,N,filters,rows', CASES, ids=[c[0] for c in CASES])
def test_encoder_against_the_model(name, content, H, W, C, N, filters, rows):
    frames, want_filtered, want_files = cases.expected(content, H, W, C, N, filters, rows)
    enc = png.PngEncoder(filters=filters, rows_per_segment=cases.rows_of(rows, H))
    dev = torch.tensor(np.array(frames)).cuda()
    if C == 1:
        dev = dev[..., 0]                                                        # [N, H, W] is served too
    with launches() as rec:
        got_filtered = enc.filtered(dev)
        files = enc.encode(dev)
    assert rec.counts == {'vqn_png_encode': 2}, rec.counts
    assert tuple(got_filtered.shape) == (N, H, 1 + W * C) and got_filtered.dtype == torch.uint8
    got_filtered = got_filtered.cpu().numpy()
    bad = np.argwhere(got_filtered != want_filtered)
    assert not len(bad), (name, 'filtered', len(bad), bad[:4], got_filtered[tuple(bad[0])], want_filtered[tuple(bad[0])])
    assert len(files) == N
    for i in range(N):
        if files[i] != want_files[i]:
            first = next((k for k, (a, b) in enumerate(zip(files[i], want_files[i])) if a != b), min(len(files[i]), len(want_files[i])))
            raise AssertionError((name, i, 'file', len(files[i]), len(want_files[i]), first, files[i][first:first + 8].hex(),
                                  want_files[i][first:first + 8].hex()))
        img = Image.open(io.BytesIO(files[i]))
        assert img.mode == MODES[C] and img.size == (W, H)
        assert np.array_equal(np.asarray(img).reshape(H, W, C), frames[i])
    assert enc.encode(dev) == files                                              # the same bytes again


@pytest.mark.parametrize('kwargs,shape,reason', [
    (dict(), (0, 8, 8, 3), 'at least one image'),
    (dict(), (1, 0, 8, 3), 'zero side'),
    (dict(), (1, 8, 0, 3), 'zero side'),
    (dict(), (1, 8, 8, 5), '1 .. 4 channels'),
    (dict(filters='best'), (1, 8, 8, 3), 'unknown filter mode'),
    (dict(rows_per_segment=0), (1, 8, 8, 3), 'at least one row'),
    (dict(rows_per_segment=-2), (1, 8, 8, 3), 'at least one row'),
    (dict(rows_per_segment=3), (1, 4, 30000, 1), 'a segment of 3 rows is 90003 bytes'),
    (dict(), (1, 2, 65535, 1), 'a row of 65536 bytes'),
    (dict(), (1, 2, 16384, 4), 'a row of 65537 bytes'),
    (dict(), (65536, 1, 1, 1), 'at most 65535 images'),
])
def test_refusals_raise_and_launch_nothing(kwargs, shape, reason):
    x = torch.zeros(shape, dtype=torch.uint8, device='cuda')
    with launches() as rec:
        with pytest.raises(ValueError, match=reason):
            png.PngEncoder(**kwargs).encode(x)
        with pytest.raises(ValueError, match=reason):
            png.PngEncoder(**kwargs).filtered(x)
    assert not rec.names                                                         # no entry point was even called


def test_other_dtypes_and_ranks_raise():
    with pytest.raises(ValueError, match='expected a uint8'):
        png.PngEncoder().encode(torch.zeros((1, 8, 8, 3), device='cuda'))
    with pytest.raises(ValueError, match='expected a uint8'):
        png.PngEncoder().encode(torch.zeros((8, 8), dtype=torch.uint8, device='cuda'))


def test_buffers_smaller_than_the_plan_are_refused():
    g, _ = _C.png_plan(1, 16, 16, 3, 5, 2)
    x = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device='cuda')
    scratch = torch.full((g['scratch_bytes'],), 0xab, dtype=torch.uint8, device='cuda')
    out = torch.full((g['out_bytes'],), 0xab, dtype=torch.uint8, device='cuda')
    meta = torch.full((1, 2), -7, dtype=torch.int64, device='cuda')
    with pytest.raises(_C.VqnError, match='byte total of up to .* over the buffer'):
        _C.png_encode(x, g, scratch, out[:-1], meta)
    with pytest.raises(_C.VqnError, match='scratch holds'):
        _C.png_encode(x, g, scratch[:g['scratch_bytes'] - 16], out, meta)
    with pytest.raises(_C.VqnError, match='scratch holds'):
        _C.png_encode(x, g, scratch[:16 * 49 - 16])                              # the filtered stream alone: 16 rows of 49 bytes
    torch.cuda.synchronize()
    assert bool((scratch == 0xab).all()) and bool((out == 0xab).all()) and bool((meta == -7).all())      # nothing ran


def test_the_worst_case_fills_the_output_exactly():
    """noise under 'none' is stored segment by segment: the streams take every byte the planner sized `out` for"""
    frames = cases.batch('noise', 16, 16, 4, 2)
    enc = png.PngEncoder('none', 1)
    head, streams = enc.streams(torch.tensor(frames).cuda())
    g, _ = _C.png_plan(2, 16, 16, 4, 0, 1)
    assert sum(len(s) for s in streams) == g['out_bytes'] and len(head) == 33


def test_cpu_tensors_raise():
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(_C.VqnError, match='no CPU fallback'):
        png.PngEncoder().encode(x)
    with pytest.raises(_C.VqnError, match='no CPU fallback'):
        png.PngEncoder().filtered(x)


def test_scratch_is_kept_and_never_shrunk():
    enc = png.PngEncoder()
    big = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device='cuda')
    enc.encode(big)
    key = [k for k in _C._scratch_cache if k[2] == 'png'][0]
    buf = _C._scratch_cache[key][0]
    enc.encode(big[:1, :8, :8].contiguous())
    assert _C._scratch_cache[key][0] is buf                                       # the smaller batch reuses it
    assert len(enc._plans) == 2


def test_unaligned_pixels_take_the_byte_loads():
    """a view whose first byte is not 32-bit aligned: the same bytes as the aligned copy"""
    frames = cases.batch('disc', 16, 16, 4, 1)
    flat = torch.zeros(frames.size + 1, dtype=torch.uint8, device='cuda')
    flat[1:] = torch.tensor(frames).cuda().reshape(-1)
    view = flat[1:].view(1, 16, 16, 4)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    enc = png.PngEncoder()
    assert enc.encode(view) == enc.encode(torch.tensor(frames).cuda())
