"""What `mjpeg.JpegEncoder` and `png.PngEncoder` share on the host (on the device: csrc/codec_stream.h): the plans of the shapes seen, the
two scratch buffers, and the way a batch comes back: one read of the [N, 2] offsets and lengths, one copy of exactly its bytes."""
import torch

from vqnerf_release_amd import _C


class DeviceCodec:
    """tag: the scratch buffers are _C._scratch(tag) and (tag + '_out'), grown and never shrunk; entry: _C.jpeg_encode / png_encode"""

    def __init__(self, tag, entry):
        self._tag, self._entry = tag, entry
        self._plans = {}

    def _cached_plan(self, key, make):
        """the plan of a batch shape, made once (make() raises ValueError with the planner's reason)"""
        if key not in self._plans:
            self._plans[key] = make()
        return self._plans[key]

    def _run(self, x, g, what, first_only=False):
        """x: the batch, g: its plan -> (the scratch, [the bytes of every item of the batch]; None when first_only: the first kernel
        alone runs and leaves its result in front of the scratch).  A CPU tensor raises under the name `what`."""
        _C.require_device(x, what)
        x = x.contiguous()
        scratch = _C._scratch(self._tag, g['scratch_bytes'], x.device)
        if first_only:
            self._entry(x, g, scratch)
            return scratch, None
        out = _C._scratch(self._tag + '_out', g['out_bytes'], x.device)
        meta = torch.empty((g['n'], 2), dtype=torch.int64, device=x.device)
        self._entry(x, g, scratch, out, meta)
        meta_h = meta.cpu()
        total = int(meta_h[-1, 0] + meta_h[-1, 1])
        data = out[:total].cpu().numpy().tobytes()
        return scratch, [data[o:o + n] for o, n in meta_h.tolist()]
