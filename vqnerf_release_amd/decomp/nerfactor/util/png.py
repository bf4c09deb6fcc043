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
from vqnerf_release_amd.decomp.nerfactor.util.device_codec import DeviceCodec

IEND = struct.pack('>I', 0) + b'IEND' + struct.pack('>I', zlib.crc32(b'IEND'))


def png_file(head, idat):
    """the 33 bytes in front of IDAT + the zlib stream of an image -> the file (the IDAT chunk's CRC is taken here, on the caller's
    thread: a writer thread of the output path)"""
    return head + struct.pack('>I', len(idat)) + b'IDAT' + idat + struct.pack('>I', zlib.crc32(b'IDAT' + idat)) + IEND


class PngEncoder(DeviceCodec):
    """filters: 'adaptive' (per row the type with the smallest sum of |residual|, libpng's heuristic) or 'none' | 'sub' | 'up' |
    'average' | 'paeth' for every row.  rows_per_segment: rows coded as one deflate block (None: as many as fit 8 KiB, at least one)."""

    def __init__(self, filters='adaptive', rows_per_segment=None):
        super().__init__('png', _C.png_encode)
        self.filters, self.rows_per_segment = filters, rows_per_segment

    def _plan(self, images):
        if not torch.is_tensor(images) or images.dim() not in (3, 4) or images.dtype != torch.uint8:
            raise ValueError(f'PngEncoder: expected a uint8 [N, H, W, C] or [N, H, W] tensor, got {getattr(images, "dtype", type(images))} '
                             f'{tuple(getattr(images, "shape", ()))}')
        if images.dim() == 3:
            images = images[..., None]
        key = tuple(int(s) for s in images.shape)

        def make():
            rows = self.rows_per_segment
            if rows is None:
                rows = max(_C.PNG_SEGMENT_TARGET // (1 + key[2] * key[3]), 1)
            return _C.png_plan(*key, _C.PNG_FILTERS.get(self.filters, -1), rows)
        return images, self._cached_plan(key, make)

    def filtered(self, images):
        """-> uint8 [N, H, stride]: the filtered stream (the first kernel alone)"""
        images, (g, _) = self._plan(images)
        n_bytes = g['n'] * g['h'] * g['stride']
        scratch, _ = self._run(images, g, 'PngEncoder.filtered', first_only=True)
        return scratch[:n_bytes].view(g['n'], g['h'], g['stride']).clone()

    def streams(self, images):
        """-> (the 33 bytes in front of IDAT, [the zlib stream of every image]).  One read of the [N, 2] offsets and lengths, then one
        copy of exactly the bytes the batch came to."""
        images, (g, head) = self._plan(images)
        return head, self._run(images, g, 'PngEncoder.encode')[1]

    def encode(self, images):
        """uint8 [N, H, W, C] or [N, H, W] device tensor -> N complete files as bytes"""
        head, streams = self.streams(images)
        return [png_file(head, s) for s in streams]
