"""Output path of the reflectance models: what `Model.vis_batch` writes per view
(decomp/nerfvq_nfr3/nerfactor/models/vq_nfr.py:988-1134, `_vis_embed` :1140-1152, `util/light.py:30-50`), restated for
device-resident result dicts with an asynchronous writer.

Same files per view directory as the reference: `<key>.png` for every image-like entry (rgb / diff / normal composited over
the white or black background with the thresholded ground-truth alpha; albedo / spec / rough / ks / basecolor as they are,
plus `<key>.npy`), `<key>_<probe>.png` per relighting probe, `embed_map.png`, `pred_edit_mask.png` (an edit's selection),
`<key>.npy` for xyz (and z / embed under `full_vis_path`), `metadata.json` (`id`, and `psnr` of the written 8-bit gt_rgb / pred_rgb when ground truth exists); once per
run `pred_light.png`, `np_light.npy` (and `vq_embed.npy` under `full_vis_path`).

What is different on purpose: nothing is written on the calling thread.  The tensors of a view leave the device through
pinned buffers on a side stream, and PNG / NPY encoding runs on worker threads (`AsyncWriter`), so a 16-probe relighting
pass does not stall the kernels behind ~20 PNG encodes per view.  `writer.flush()` joins.

`vis_batch(png='device')` goes one step further for views whose tensors are on the device: every 8-bit image the host path would
write is formed there (`view_files` says which entry becomes which file and `view_image` forms it, for numpy arrays and torch
tensors alike: one table and one statement, which the host writer and the device writer both loop over), all 3-channel images of the view are PNG-encoded as one batch and
all 1-channel images as another (util/png.py, csrc/png_encode.hip), and only the compressed bytes and the `.npy` arrays cross to the
host; the worker threads take the IDAT CRC and write.  The files decode to the same pixels.  `pred_light.png` stays on the host path.

Third-party arithmetic restated (xiuminglib, not in the reference tree): `xm.io.img.write_arr(arr, path, clip=True)` clips to
[0, 1] and casts `arr * 255` to uint8 (truncation); `xm.metric.PSNR('uint8')` = 10 log10(1 / mean((a/255 - b/255)^2)).
"""
import json
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

_EMBED_COLOURS = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255],
                           [128, 0, 0], [0, 128, 0], [0, 0, 128], [128, 128, 0], [128, 0, 128], [0, 128, 128],
                           [255, 128, 128], [128, 255, 128], [128, 128, 255], [255, 255, 128], [255, 128, 255],
                           [128, 255, 255]], np.uint8)           # vq_nfr.py:1141-1146 (handed to cv2.imwrite, i.e. B, G, R)
_EMBED_LUT = np.concatenate([np.zeros((1, 3), np.uint8), _EMBED_COLOURS[:, ::-1]])       # code -> R, G, B of embed_map.png; 0 = background


# ---- the 8-bit images of a view: every statement once, for host arrays (numpy) and device tensors (torch) alike ----------------------
def to_uint8(arr01):
    """clip to [0, 1], times 255, truncating cast"""
    if torch.is_tensor(arr01):
        return (torch.clamp(arr01, 0.0, 1.0) * 255.0).to(torch.uint8)
    return (np.clip(arr01, 0.0, 1.0) * 255.0).astype(np.uint8)


def alpha_blend(a, alpha, b):
    """a * alpha + b * (1 - alpha), alpha [H,W] broadcast over channels (util/img.py:78-97)."""
    if a.ndim == 3 and alpha.ndim == 2:
        alpha = alpha[:, :, None]
    return a * alpha + b * (1.0 - alpha)


def composite(v, alpha, white_bg):
    """v [H,W,3] over the white or black background with alpha [H,W] (already thresholded), in f32, not yet clipped"""
    xp = torch if torch.is_tensor(v) else np
    return alpha_blend(v, alpha, xp.ones_like(v) if white_bg else xp.zeros_like(v))


def threshold_alpha(alpha, alpha_thres):
    """the stricter compositing alpha of vis_batch (vq_nfr.py:1039-1042): values below the threshold become 0.  numpy or torch."""
    xp = torch if torch.is_tensor(alpha) else np
    return xp.where(alpha < alpha_thres, xp.zeros_like(alpha), alpha)


def composite_uint8(v, alpha, white_bg):
    """The 8-bit image vis_batch writes for a colour entry, and the frame decomp/video.py encodes: the same f32 operations in the same
    order (multiply, multiply, add, clamp, times 255, truncating cast), so the PNG and the video frame hold the same bytes."""
    return to_uint8(composite(v, alpha, white_bg))


def relit_names(key, n_maps, probe_names, olat_names, olat_first_n):
    """[(index, light name)] of the relit images vis_batch writes for `pred_rgb_probes` / `pred_rgb_olat` with n_maps conditions: every
    probe; of the OLAT maps the top half of the light grid only (vq_nfr.py:1049-1057)"""
    names = olat_names if key == 'pred_rgb_olat' else probe_names
    return [(i, lname) for i, lname in enumerate(names[:n_maps]) if not (key == 'pred_rgb_olat' and i >= olat_first_n)]


def psnr_uint8(a, b):
    mse = np.mean((a.astype(np.float64) / 255.0 - b.astype(np.float64) / 255.0) ** 2)
    return float('inf') if mse == 0 else float(10.0 * np.log10(1.0 / mse))


def write_png(path, img_uint8):
    from PIL import Image
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    Image.fromarray(img_uint8).save(path, compress_level=3)


def embed_map(embed):
    """Code index image (0 = background, 1..18 = codes) -> the colour map of `_vis_embed`, RGB order of the written file."""
    if torch.is_tensor(embed):
        e = torch.round(embed).to(torch.int64)
        return torch.as_tensor(_EMBED_LUT, device=embed.device)[torch.where((e >= 1) & (e <= 18), e, torch.zeros_like(e))]
    e = np.rint(embed).astype(np.int64)
    return _EMBED_LUT[np.where((e >= 1) & (e <= 18), e, 0)]


def embed_labels(rgb, device):
    """The inverse of embed_map: embed_map.png (uint8 [H, W, 3], RGB) -> int32 labels [H * W] on the device, 0 for a colour that is
    no code's."""
    px = torch.as_tensor(rgb, device=device).reshape(-1, 3).to(torch.int32)
    pal = torch.as_tensor(_EMBED_LUT[1:], device=device).to(torch.int32)
    hit = (px[:, None, :] == pal[None]).all(-1)
    return torch.where(hit.any(1), hit.to(torch.int32).argmax(1).to(torch.int32) + 1, torch.zeros((), dtype=torch.int32, device=device))


def view_hw(to_vis):
    """(H, W) of a `to_vis` dict, whose 'hw' is [2] or one row per pixel"""
    hw = to_vis['hw']
    return tuple(int(x) for x in (hw[0] if hw.ndim == 2 else hw).tolist())


def light_names(model):
    """(probe names, OLAT names, olat_first_n) of a model: the lights its relit images are named after (see relit_names)"""
    light_res = getattr(model, 'light_res', (16, 32))
    return list(getattr(model, 'novel_probes', {}) or {}), list(getattr(model, 'novel_olat', {}) or {}), int(np.prod(light_res)) // 2


class AsyncWriter:
    """Device -> pinned host copies on a side stream + a pool of encoder threads.  submit() returns at once; flush() waits
    for everything submitted so far and re-raises the first worker error."""

    def __init__(self, n_threads=8):
        self.pool = ThreadPoolExecutor(max_workers=n_threads)       # leaf jobs: one PNG / NPY file each
        self.views = ThreadPoolExecutor(max_workers=2)              # per-view coordinators (they wait on leaf jobs: own pool)
        self.futures = []
        self.lock = threading.Lock()
        self.stream = None

    def fetch(self, tensors):
        """{k: device tensor} -> (host dict of pinned tensors, event or None); the copies are asynchronous."""
        dev = next((v.device for v in tensors.values() if torch.is_tensor(v) and v.is_cuda), None)
        if dev is None:
            return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in tensors.items()}, None
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        host = {}
        with torch.cuda.stream(self.stream):
            for k, v in tensors.items():
                if torch.is_tensor(v) and v.is_cuda:
                    v = v.detach()
                    v.record_stream(self.stream)
                    buf = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                    buf.copy_(v, non_blocking=True)
                    host[k] = buf
                else:
                    host[k] = v.detach() if torch.is_tensor(v) else v
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return host, ev

    def submit(self, fn, *args):
        f = self.views.submit(fn, *args)
        with self.lock:
            self.futures.append(f)
        return f

    def flush(self):
        with self.lock:
            fs, self.futures = self.futures, []
        for f in fs:
            f.result()


_default_writer = None


def default_writer():
    global _default_writer
    if _default_writer is None:
        _default_writer = AsyncWriter()
    return _default_writer


def _view_shape(k, shape, hw):
    """the image shape of entry k whose rows have `shape` (vq_nfr.py:1021-1034)"""
    if k in ('pred_rgb_olat', 'pred_rgb_probes'):
        return hw + (shape[1], 3)
    if k.endswith(('rgb', 'albedo', 'normal', 'diff', 'spec', 'xyz', 'basecolor')):
        return hw + (3,)
    if k.endswith(('occu', 'depth', 'disp', 'alpha', 'rough', 'embed', 'ks')):
        return hw
    if k.endswith(('z',)):
        return hw + (shape[1],)
    if k.endswith('edit_mask'):                                  # the selection of fast_render(edit_select=...), 0 / 1
        return hw
    raise NotImplementedError(k)


def _shape_views(host, hw):
    """Rows back to images (vq_nfr.py:1021-1034)."""
    out = {}
    for k, v in host.items():
        if v is None:
            continue
        a = v.numpy() if torch.is_tensor(v) else np.asarray(v)
        a = a.astype(np.float32, copy=False) if a.dtype.kind == 'f' else a.astype(np.float32)
        out[k] = a.reshape(_view_shape(k, a.shape, hw))
    return out


OVER_BG, AS_IS, NORMAL, EMBED = 'over the background', 'as it is', 'normal', 'embed map'


def view_files(shapes, mode, simp, full_vis, probe_names, olat_names, olat_first_n):
    """The files of one view (vq_nfr.py:1043-1110), for {key: image shape} in the order of the dict:
    ([(file stem, key, index of the light or None, kind)] of the PNGs, [(key, 'outdir' | 'full_vis_path')] of the .npy arrays).
    The one statement of the per-key rule: the host writer and the device writer both loop over it.  The order of the ladder is
    behaviour."""
    images, arrays = [], []
    for k, shape in shapes.items():
        if k in ('pred_rgb_olat', 'pred_rgb_probes'):
            images += [(k + '_' + lname, k, i, OVER_BG) for i, lname in relit_names(k, shape[2], probe_names, olat_names, olat_first_n)]
        elif k.endswith(('rgb', 'diff')):
            images.append((k, k, None, OVER_BG))
        elif k.endswith(('albedo', 'spec', 'rough', 'ks', 'basecolor')):
            arrays.append((k, 'outdir'))
            images.append((k, k, None, AS_IS))
        elif k.endswith(('embed',)):
            if full_vis:
                arrays.append((k, 'full_vis_path'))
            images.append(('embed_map', k, None, EMBED))
        elif k.endswith(('z',)) and full_vis:                     # (catches '...xyz' too when full_vis is on, as the reference does)
            arrays.append((k, 'full_vis_path'))
        elif k.endswith(('xyz',)):
            arrays.append((k, 'outdir'))
        elif k.endswith('normal'):
            images.append((k, k, None, NORMAL))
        elif k.endswith('edit_mask'):
            images.append((k, k, None, AS_IS))
        elif k.endswith(('z',)):
            pass                                                 # latent codes are only dumped under full_vis
        elif mode != 'render' and not simp:
            images.append((k, k, None, AS_IS))
    return images, arrays


def view_image(v, light, kind, alpha, white_bg):
    """the 8-bit image of one row of view_files' table from the entry v, shaped as an image (numpy or torch); alpha: thresholded"""
    if light is not None:
        v = v[:, :, light, :]
    if kind == EMBED:
        return embed_map(v)
    if kind == NORMAL:
        v = (v + 1.0) / 2.0
    return to_uint8(v if kind == AS_IS else composite(v, alpha, white_bg))


def _scored(mode, simp):
    """does metadata.json of such a pass carry the scores of gt_rgb against pred_rgb (where both exist)"""
    return not simp and mode not in ('test', 'render')


def write_metadata(outdir, id_, mode, simp, gt_u8, pred_u8, scores):
    """metadata.json of a view: gt_u8 / pred_u8 the written 8-bit gt_rgb / pred_rgb or None, scores the device's (util/metric.py) or None"""
    if simp:
        return
    meta = {'id': id_}
    if _scored(mode, simp) and gt_u8 is not None and pred_u8 is not None:
        meta['psnr'] = psnr_uint8(np.asarray(gt_u8), np.asarray(pred_u8))
        if scores is not None:                                   # the device's scores of the same two images
            from vqnerf_release_amd.decomp.nerfactor.util.metric import KEYS
            meta.update(zip(KEYS, scores.tolist()))
    with open(os.path.join(outdir, 'metadata.json'), 'w') as f:
        json.dump(meta, f)


def _save_arrays(d, arrays, outdir, full_vis_path, pool_submit):
    return [pool_submit(np.save, os.path.join(full_vis_path if where == 'full_vis_path' else outdir, k + '.npy'), d[k]) for k, where in arrays]


def _write_view(host, event, hw, id_, outdir, mode, white_bg, lights, alpha_thres, simp, full_vis_path, pool_submit, scores=None):
    """a worker's share of the host path: the view's images formed in numpy, PIL and np.save on the pool"""
    if event is not None:
        event.synchronize()
    d = _shape_views(host, hw)
    os.makedirs(outdir, exist_ok=True)
    alpha = threshold_alpha(d['gt_alpha'], alpha_thres)
    images, arrays = view_files({k: v.shape for k, v in d.items()}, mode, simp, full_vis_path is not None, *lights)
    jobs = _save_arrays(d, arrays, outdir, full_vis_path, pool_submit)
    written = {}
    for stem, k, light, kind in images:
        written[stem] = view_image(d[k], light, kind, alpha, white_bg)
        jobs.append(pool_submit(write_png, os.path.join(outdir, stem + '.png'), written[stem]))
    write_metadata(outdir, id_, mode, simp, written.get('gt_rgb'), written.get('pred_rgb'), scores)
    for j in jobs:
        j.result()


def _write_bytes(path, head, stream):
    """a worker's share of a device-encoded PNG: the IDAT CRC and the file"""
    from vqnerf_release_amd.decomp.nerfactor.util.png import png_file
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(png_file(head, stream))


_png_encoder = None


def _write_view_device(host, event, hw, id_, outdir, mode, simp, arrays, full_vis_path, files, pool_submit, scores=None):
    """a worker's share of the device path: the fetched arrays through np.save, the encoded streams into their files"""
    if event is not None:
        event.synchronize()
    pair = [host.pop(k, None) for k in ('_gt_rgb_u8', '_pred_rgb_u8')]
    d = _shape_views(host, hw)
    os.makedirs(outdir, exist_ok=True)
    jobs = _save_arrays(d, arrays, outdir, full_vis_path, pool_submit)
    jobs += [pool_submit(_write_bytes, os.path.join(outdir, stem + '.png'), head, stream) for stem, head, stream in files]
    write_metadata(outdir, id_, mode, simp, pair[0], pair[1], scores)
    for j in jobs:
        j.result()


def _vis_batch_device(model, data_dict, hw, id_, outdir, mode, alpha_thres, simp, full_vis_path, writer, scores):
    """the view's images formed (view_files, view_image on device tensors) and PNG-encoded on the device; the bytes, the .npy arrays and
    metadata.json through the writer"""
    global _png_encoder
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.decomp.nerfactor.util.png import PngEncoder
    d = {}
    for k, v in data_dict.items():
        if v is None:
            continue
        if not torch.is_tensor(v):
            raise _C.VqnError(f"vis_batch(png='device'): entry {k!r} is a {type(v).__name__}, not a device tensor")
        _C.require_device(v, "vis_batch(png='device')")
        d[k] = v.detach().to(torch.float32).reshape(_view_shape(k, tuple(v.shape), hw))
    alpha = threshold_alpha(d['gt_alpha'], alpha_thres)
    table, arrays = view_files({k: v.shape for k, v in d.items()}, mode, simp, full_vis_path is not None, *light_names(model))
    images = [(stem, view_image(d[k], light, kind, alpha, bool(model.white_bg))) for stem, k, light, kind in table]
    if _png_encoder is None:
        _png_encoder = PngEncoder()
    files = []
    for rank in (3, 2):                                          # all [H,W,3] images as one batch, all [H,W] images as another
        group = [(stem, img) for stem, img in images if img.dim() == rank]
        if group:
            head, streams = _png_encoder.streams(torch.stack([img for _, img in group]))
            files += [(stem, head, s) for (stem, _), s in zip(group, streams)]
    written = dict(images)
    fetch = {k: data_dict[k] for k, _ in arrays}
    if _scored(mode, simp) and 'gt_rgb' in written and 'pred_rgb' in written:
        fetch['_gt_rgb_u8'], fetch['_pred_rgb_u8'] = written['gt_rgb'], written['pred_rgb']
    if scores is not None:
        fetch['_scores'] = scores
    host, ev = writer.fetch(fetch)
    scores = host.pop('_scores', None)
    if full_vis_path is not None:
        os.makedirs(full_vis_path, exist_ok=True)
    writer.submit(_write_view_device, host, ev, hw, id_, outdir, mode, simp, arrays, full_vis_path, files, writer.pool.submit, scores)
    return writer


def vis_light_uint8(light, h=None):
    """[h0,w0,3] probe -> uint8 image, optionally resized to height h with antialiased bilinear filtering (light.py:30-50)."""
    t = torch.as_tensor(light, dtype=torch.float32).detach().cpu()
    if h is not None and h != t.shape[0]:
        w = int(round(t.shape[1] * h / t.shape[0]))
        t = torch.nn.functional.interpolate(t.permute(2, 0, 1)[None], size=(h, w), mode='bilinear', align_corners=False,
                                            antialias=True)[0].permute(1, 2, 0)
    return to_uint8(t.numpy())


def _device_scores(data_dict, hw, white_bg, alpha_thres):
    """psnr, mse, psnr_luma, ssim, ssim_luma (float64 [5], on the device) of gt_rgb against pred_rgb, both composited as
    the written PNGs are (`composite`: the same f32 operations in the same order; the kernel quantises as to_uint8)"""
    from vqnerf_release_amd.decomp.nerfactor.util import metric
    alpha = threshold_alpha(data_dict['gt_alpha'].detach().to(torch.float32).reshape(hw), alpha_thres)
    pair = [composite(data_dict[k].detach().to(torch.float32).reshape(hw + (3,)), alpha, white_bg)[None] for k in ('gt_rgb', 'pred_rgb')]
    return metric.image_metrics_raw(pair[0], pair[1]).view(torch.float64)[0, :len(metric.KEYS)]


def vis_batch(model, data_dict, outdir, mode='train', light_vis_h=256, alpha_thres=0.8, simp=False, full_vis_path=None,
              writer=None, metrics=False, png='host'):
    """Model.vis_batch (vq_nfr.py:988-1134).  data_dict: the `to_vis` dict of `call` / `fast_render` / `vis_mat` (device
    tensors with N = H*W rows, plus 'hw' [N,2] and 'id').  Returns the AsyncWriter the files were queued on.
    metrics: where `metadata.json` gets its `psnr` (ground truth exists, not `simp`, not a test / render pass), also score the
    two images on the device before they are fetched (util/metric.py) and write `psnr`, `mse`, `psnr_luma`, `ssim`, `ssim_luma`
    there; `psnr` is then the device's value.  Off (the default): every file is what it was.
    png: 'host' (the default): PIL on the writer's threads, every file byte for byte what it was.  'device': the 8-bit images are formed
    and PNG-encoded on the device (device tensors only; the files decode to the same pixels, the .npy files and metadata.json are the
    same bytes); `pred_light.png` is written by the host path either way."""
    model._validate_mode(mode)
    if png not in ('host', 'device'):
        raise ValueError(f"vis_batch: png is 'host' or 'device', got {png!r}")
    writer = writer or default_writer()
    if mode == 'vali':
        root = os.path.dirname(outdir.rstrip('/'))
        light_png = os.path.join(root, 'pred_light.png')
        if not os.path.exists(light_png):                        # the same for every view: once
            os.makedirs(root or '.', exist_ok=True)
            light = model.light.detach().cpu()
            write_png(light_png, vis_light_uint8(light, light_vis_h))
            np.save(os.path.join(root, 'np_light.npy'), light.numpy())
        if full_vis_path is not None and hasattr(model, 'get_codebook'):
            os.makedirs(full_vis_path, exist_ok=True)
            np.save(os.path.join(full_vis_path, 'vq_embed.npy'), model.get_codebook().detach().cpu().numpy())
    if mode == 'train':                                          # randomly sampled rays do not form an image
        return writer
    data_dict = dict(data_dict)
    hw = view_hw(data_dict)
    del data_dict['hw']
    id_ = data_dict.pop('id')
    if isinstance(id_, (list, tuple)):
        id_ = id_[0]
    if isinstance(id_, bytes):
        id_ = id_.decode()
    scores = None
    if metrics and _scored(mode, simp) and all(data_dict.get(k) is not None for k in ('gt_rgb', 'pred_rgb', 'gt_alpha')):
        scores = _device_scores(data_dict, hw, bool(model.white_bg), alpha_thres)
    if png == 'device':
        return _vis_batch_device(model, data_dict, hw, str(id_), outdir, mode, alpha_thres, simp, full_vis_path, writer, scores)
    host, ev = writer.fetch({k: v for k, v in dict(data_dict, **({} if scores is None else {'_scores': scores})).items() if v is not None})
    scores = host.pop('_scores', None)
    if full_vis_path is not None:
        os.makedirs(full_vis_path, exist_ok=True)
    writer.submit(_write_view, host, ev, hw, str(id_), outdir, mode, bool(model.white_bg), light_names(model), alpha_thres, simp, full_vis_path,
                  writer.pool.submit, scores)
    return writer
