"""Videos of frames that are on the device: baseline JPEG in HIP (csrc/jpeg_encode.hip), Motion-JPEG AVI files on the host.

The reference packs its fly-through frames with `cv2.VideoWriter(..., fourcc('M','J','P','G'), fps, size)` (cv2_render.py) after
writing every frame as an image file and reading it back.  Here the 8-bit frames never leave the device as pixels: `JpegEncoder`
turns a batch [N, H, W, 3] into N complete JPEG files with one device-to-host copy of the compacted bytes, `AviWriter` appends them as
`00dc` chunks of a RIFF AVI file (one `vids` / `MJPG` stream, `idx1` index, below 2 GiB: no OpenDML), and `VideoSink` holds one file
per stream name and hands the appends to the `AsyncWriter` pool in frame order.  There is no CPU fallback: a CPU tensor raises."""
import os
import struct

import torch

from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.util.device_codec import DeviceCodec


class JpegEncoder(DeviceCodec):
    """quality 1 .. 100 (IJG scaling of the Annex K tables), subsampling '420' (what OpenCV's MJPG writes) or '444',
    restart_interval in MCUs (None: one MCU row).  The format and the shape of the device work: csrc/jpeg_encode.hip."""

    def __init__(self, quality=75, subsampling='420', restart_interval=None):
        super().__init__('jpeg', _C.jpeg_encode)
        self.quality, self.subsampling, self.restart_interval = quality, subsampling, restart_interval

    def _plan(self, frames):
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError(f'JpegEncoder: expected a uint8 [N, H, W, 3] tensor, got {getattr(frames, "dtype", type(frames))} '
                             f'{tuple(getattr(frames, "shape", ()))}')
        key = tuple(int(s) for s in frames.shape[:3])

        def make():
            sub = int(self.subsampling) if str(self.subsampling).isdigit() else 0
            ri = self.restart_interval
            if ri is None:                                           # one MCU row
                mcu = 16 if sub == 420 else 8
                ri = max((key[2] + mcu - 1) // mcu, 1)
            return _C.jpeg_plan(*key, self.quality, sub, ri)
        return self._cached_plan(key, make)

    def coefficients(self, frames):
        """-> {'y', 'cb', 'cr': int16 [N, by, bx, 64]}: the quantised coefficients in zigzag order (the first kernel alone)"""
        g, _ = self._plan(frames)
        scratch, _ = self._run(frames, g, 'JpegEncoder.coefficients', first_only=True)
        return self._coefficient_views(scratch, g)

    @staticmethod
    def _coefficient_views(scratch, g):
        ends = {'y': (0, g['off_cb'], g['by_y'], g['bx_y']), 'cb': (g['off_cb'], g['off_cr'], g['by_c'], g['bx_c']),
                'cr': (g['off_cr'], g['off_slots'], g['by_c'], g['bx_c'])}
        return {k: scratch[a:b].view(torch.int16).view(g['n'], by, bx, 64).clone() for k, (a, b, by, bx) in ends.items()}

    def encode(self, frames, want_coefficients=False):
        """uint8 [N, H, W, 3] device tensor -> N complete files (header + scan + EOI) as bytes.  One read of the [N, 2] offsets and
        lengths, then one copy of exactly the bytes the batch came to."""
        g, header = self._plan(frames)
        scratch, scans = self._run(frames, g, 'JpegEncoder.encode')
        files = [header + scan + b'\xff\xd9' for scan in scans]
        return (files, self._coefficient_views(scratch, g)) if want_coefficients else files


class AviWriter:
    """A Motion-JPEG AVI file of frames size_wh = (W, H) at fps: RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh' vids / MJPG,
    'strf' BITMAPINFOHEADER } }, LIST 'movi' { '00dc' chunks, padded to even length }, 'idx1' }.  Sizes and frame counts are patched by
    close().  A write that would take the closed file past MAX_BYTES raises: AVI 1.0 sizes are 32 bits and readers stop at 2 GiB."""
    MAX_BYTES = 2 ** 31 - 1

    def __init__(self, path, size_wh, fps=20):
        self.path, (self.w, self.h), self.fps = path, (int(size_wh[0]), int(size_wh[1])), fps
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        self.f = open(path, 'wb')
        self.index, self.largest = [], 0
        self.f.write(self._head(0))
        self.movi = self.f.tell() - 4                                # where the 'movi' fourcc stands: idx1 offsets count from it
        self.pos = self.f.tell()

    def _rate(self):
        return (int(self.fps), 1) if float(self.fps).is_integer() else (int(round(self.fps * 1000)), 1000)

    def _head(self, movi_bytes):
        n = len(self.index)
        rate, scale = self._rate()
        avih = struct.pack('<14I', int(round(1e6 * scale / rate)), 0, 0, 0x10, n, 0, 1, self.largest, self.w, self.h, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', b'MJPG', 0, 0, 0, 0, scale, rate, 0, n, self.largest, 0xffffffff, 0,
                           0, 0, self.w, self.h)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.w, self.h, 1, 24, b'MJPG', (self.w * self.h * 3) & 0xffffffff, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        head = b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl + b'LIST' + struct.pack('<I', 4 + movi_bytes) + b'movi'
        riff = len(head) + movi_bytes + 8 + 16 * n
        return b'RIFF' + struct.pack('<I', riff) + head

    def write(self, jpeg_bytes):
        if self.f is None:
            raise ValueError(f'{self.path}: write after close')
        n = len(jpeg_bytes)
        chunk = 8 + n + (n & 1)
        if self.pos + chunk + 8 + 16 * (len(self.index) + 1) > self.MAX_BYTES:
            raise ValueError(f'{self.path}: frame {len(self.index)} would take the file past {self.MAX_BYTES} bytes; an AVI without '
                             'OpenDML extensions ends there (write shorter videos)')
        self.f.write(b'00dc' + struct.pack('<I', n) + jpeg_bytes + (b'\0' if n & 1 else b''))
        self.index.append((self.pos - self.movi, n))
        self.largest = max(self.largest, n)
        self.pos += chunk

    def close(self):
        if self.f is None:
            return
        self.f.write(b'idx1' + struct.pack('<I', 16 * len(self.index)))
        self.f.write(b''.join(struct.pack('<4sIII', b'00dc', 0x10, off, n) for off, n in self.index))
        self.f.seek(0)
        self.f.write(self._head(self.pos - self.movi - 4))
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class VideoSink:
    """One AVI file `<outdir>/<name>.avi` per stream name.  push({name: uint8 [H, W, 3] device tensor}) encodes the streams of a frame as
    ONE batch and queues the file appends on the AsyncWriter pool; the appends of a stream keep the order of the pushes.  close()
    waits for them and finishes the files."""

    def __init__(self, outdir, names, size_wh, fps, encoder, writer=None):
        from vqnerf_release_amd.decomp.nerfactor.util.vis import default_writer
        self.names = list(names)
        self.size_wh = (int(size_wh[0]), int(size_wh[1]))
        self.encoder, self.writer = encoder, writer or default_writer()
        self.files = {n: AviWriter(os.path.join(outdir, n + '.avi'), self.size_wh, fps) for n in self.names}
        self._last = None
        self.frames = 0

    def push(self, frames):
        if sorted(frames) != sorted(self.names):
            raise ValueError(f'VideoSink.push: streams {sorted(frames)} given, {sorted(self.names)} expected')
        want = (self.size_wh[1], self.size_wh[0], 3)
        for n in self.names:
            if tuple(frames[n].shape) != want:
                raise ValueError(f'VideoSink.push: stream {n!r} is {tuple(frames[n].shape)}, frames are {want}')
        jpegs = self.encoder.encode(torch.stack([frames[n] for n in self.names]))
        self._last = self.writer.submit(self._append, self._last, jpegs)
        self.frames += 1

    def _append(self, before, jpegs):
        if before is not None:
            before.result()                                          # frame order: the pool may run two appends at a time
        for n, b in zip(self.names, jpegs):
            self.files[n].write(b)

    def close(self):
        try:
            if self._last is not None:
                self._last.result()
        finally:
            for f in self.files.values():
                f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
