"""PNG files of images that are on the device: row filtering and DEFLATE in HIP (csrc/png_encode.hip), the chunk framing on the host.

The host path of the output code hands every 8-bit image to PIL on a worker thread (`vis.write_png`, 28 ms per 800 x 800 frame).
`PngEncoder` turns a batch [N, H, W, C] that is already on the device into N complete files with one read of the [N, 2] offsets and
lengths and one device-to-host copy of exactly the compressed bytes; what is left for a worker thread is the CRC-32 of the IDAT chunk
(`zlib.crc32`) and the file write.  Any PNG reader opens the files; they are lossless, so they decode to the pixels PIL's would.
The stream format -- segments of whole rows, one deflate block each under the cheapest of a set of prefabricated Huffman tables --
is stated in tests/png_model.py.  There is no CPU fallback: a CPU tensor raises."""
import struct
import zlib

import torch

from vqnerf_release_amd import _C

IEND = struct.pack('>I', 0) + b'IEND' + struct.pack('>I', zlib.crc32(b'IEND'))


def png_file(head, idat):
    """the 33 bytes in front of IDAT + the zlib stream of an image -> the file (the IDAT chunk's CRC is taken here, on the caller's
    thread: a writer thread of the output path)"""
    return head + struct.pack('>I', len(idat)) + b'IDAT' + idat + struct.pack('>I', zlib.crc32(b'IDAT' + idat)) + IEND


class PngEncoder:
    """filters: 'adaptive' (per row the type with the smallest sum of |residual|, libpng's heuristic) or 'none' | 'sub' | 'up' |
    'average' | 'paeth' for every row.  rows_per_segment: rows coded as one deflate block (None: as many as fit 8 KiB, at least one)."""

    def __init__(self, filters='adaptive', rows_per_segment=None):
        self.filters, self.rows_per_segment = filters, rows_per_segment
        self._plans = {}

    def _plan(self, images):
        if not torch.is_tensor(images) or images.dim() not in (3, 4) or images.dtype != torch.uint8:
            raise ValueError(f'PngEncoder: expected a uint8 [N, H, W, C] or [N, H, W] tensor, got {getattr(images, "dtype", type(images))} '
                             f'{tuple(getattr(images, "shape", ()))}')
        if images.dim() == 3:
            images = images[..., None]
        key = tuple(int(s) for s in images.shape)
        if key not in self._plans:
            rows = self.rows_per_segment
            if rows is None:
                rows = max(_C.PNG_SEGMENT_TARGET // (1 + key[2] * key[3]), 1)
            self._plans[key] = _C.png_plan(*key, _C.PNG_FILTERS.get(self.filters, -1), rows)      # ValueError with the planner's reason
        return images, self._plans[key]

    def filtered(self, images):
        """-> uint8 [N, H, stride]: the filtered stream (the first kernel alone)"""
        images, (g, _) = self._plan(images)
        _C.require_device(images, 'PngEncoder.filtered')
        images = images.contiguous()
        n_bytes = g['n'] * g['h'] * g['stride']
        scratch = _C._scratch('png', g['scratch_bytes'], images.device)
        _C.png_encode(images, g, scratch)
        return scratch[:n_bytes].view(g['n'], g['h'], g['stride']).clone()

    def streams(self, images):
        """-> (the 33 bytes in front of IDAT, [the zlib stream of every image]).  One read of the [N, 2] offsets and lengths, then one
        copy of exactly the bytes the batch came to."""
        images, (g, head) = self._plan(images)
        _C.require_device(images, 'PngEncoder.encode')
        images = images.contiguous()
        scratch = _C._scratch('png', g['scratch_bytes'], images.device)
        out = _C._scratch('png_out', g['out_bytes'], images.device)
        meta = torch.empty((g['n'], 2), dtype=torch.int64, device=images.device)
        _C.png_encode(images, g, scratch, out, meta)
        meta_h = meta.cpu()
        total = int(meta_h[-1, 0] + meta_h[-1, 1])
        data = out[:total].cpu().numpy().tobytes()
        return head, [data[o:o + n] for o, n in meta_h.tolist()]

    def encode(self, images):
        """uint8 [N, H, W, C] or [N, H, W] device tensor -> N complete files as bytes"""
        head, streams = self.streams(images)
        return [png_file(head, s) for s in streams]
