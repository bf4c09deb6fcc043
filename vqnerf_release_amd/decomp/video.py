"""Fly-through videos of a scene: the loop of the reference's decomp/nerfvq_nfr3/nerfactor/gen_video.py (modes `recon`, `relight`, `edit`)
over the views of datasets/video_nfr.py, with its cv2_render.py folded in: every frame of every stream is composited to 8 bits on the
device, encoded there as baseline JPEG (csrc/jpeg_encode.hip) and appended to that stream's Motion-JPEG AVI file
(decomp/nerfactor/util/mjpeg.py).  The reference writes each frame as PNG files, reads them back and hands them to cv2.VideoWriter.

Streams, all in `outroot`, `<scene>` in front:
  recon    `_rgb`                              model.fast_render(batch)
  relight  `_rgb`, `_<light>` per probe (and per OLAT map of the top half of the light grid, where the model renders them) from
           model.fast_render(relight_olat=True, relight_probes=True, opt_scale); with vq_model `_vq_<light>` from its fast_render
  edit     the streams of relight after the material replacement `dst`.  With `selection` (a material_edit.Selection) the rows are picked
           on the device by vq_model.fast_render(edit_select=...) as decomp/edit.run does, the stage-3 model takes the same rows, and
           the masks are written the way the reference's window writes them (outroot/auto_sel/test_{i:03d}.npy, bool [H, W, 3], and
           auto_sel/dst.json); with `mask_dir` such files are read instead (gen_video.py:219-240) and `dst` defaults to its dst.json
           (both directions through decomp/view_tree.py, which edit.run writes through as well).
A frame of a stream is exactly the 8-bit image `vis_batch` writes for the same key (util/vis.py: composite_uint8 over the configured
background with the thresholded alpha).  frames=True also writes those per-frame directories through vis_batch: outroot/test_{i:03d}/
for the stage-3 model and outroot/vq/test_{i:03d}/ for the VQ model (the reference lets the second model overwrite the first one's
files of the same name).  Not here: the reference's `vq_dcomps` / `gen_comps` modes (train_nfr.render_views over the video dataset
writes those components), the environment-map inset, audio, and sharding: one AVI is one ordered stream."""
import os

import torch

from vqnerf_release_amd.decomp import view_tree
from vqnerf_release_amd.decomp.nerfactor.util import material_edit, mjpeg, vis

MODES = ('recon', 'relight', 'edit')
ALPHA_THRES = 0.8                    # vis_batch's default: the frames are the images it writes


def stream_names(scene, mode, probe_names=(), olat_names=(), olat_first_n=0, ref_olat=False, vq=False, vq_olat=False):
    """[(stream name, model tag 'ref' | 'vq', to_vis key, index of the light or None)] in the order the streams are encoded.
    ref_olat / vq_olat: the model renders the OLAT maps (the stage-3 model never does; the VQ model with `render_olat`)."""
    if mode not in MODES:
        raise ValueError(f'mode is one of {MODES}, got {mode!r}')
    out = [(f'{scene}_rgb', 'ref', 'pred_rgb', None)]
    if mode == 'recon':
        return out
    for tag, has, olat, pre in (('ref', True, ref_olat, f'{scene}_'), ('vq', vq, vq_olat, f'{scene}_vq_')):
        if not has:
            continue
        if olat:
            out += [(pre + n, tag, 'pred_rgb_olat', i) for i, n in vis.relit_names('pred_rgb_olat', len(olat_names), probe_names, olat_names, olat_first_n)]
        out += [(pre + n, tag, 'pred_rgb_probes', i) for i, n in vis.relit_names('pred_rgb_probes', len(probe_names), probe_names, olat_names, olat_first_n)]
    names = [o[0] for o in out]
    if len(set(names)) != len(names):
        raise ValueError(f'two streams share a name: {sorted(n for n in set(names) if names.count(n) > 1)}')
    return out


def frames_of(to_vis, streams, tag, white_bg, alpha_thres=ALPHA_THRES):
    """{stream name: uint8 [H, W, 3] device tensor} of the streams of model `tag` from its `to_vis`"""
    H, W = vis.view_hw(to_vis)
    alpha = vis.threshold_alpha(to_vis['gt_alpha'].detach().to(torch.float32).reshape(H, W), alpha_thres)
    out = {}
    for name, t, key, i in streams:
        if t != tag:
            continue
        v = to_vis[key].detach().to(torch.float32)
        v = v.reshape(H, W, 3) if i is None else v.reshape(H, W, v.shape[1], 3)[:, :, i, :]
        out[name] = vis.composite_uint8(v, alpha, white_bg)
    return out


@torch.no_grad()
def run(model, dataset, outroot, mode, vq_model=None, opt_scale=None, selection=None, dst=None, mask_dir=None, fps=20, quality=75,
        frames=False, scene=None, writer=None, png='host'):
    """-> {stream name: path of its AVI file}.  model: the stage-3 model; dataset: datasets/video_nfr.py; see the module text.
    png: how the per-frame files of frames=True are encoded ('host' or 'device': vis.vis_batch)."""
    if mode not in MODES:
        raise ValueError(f'mode is one of {MODES}, got {mode!r}')
    if mode == 'edit':
        if (selection is None) == (mask_dir is None):
            raise ValueError('an edit takes either a selection or a mask_dir')
        if selection is not None and not isinstance(selection, material_edit.Selection):
            raise ValueError(f'selection is a material_edit.Selection, got {type(selection).__name__}')
        if selection is not None and vq_model is None:
            raise ValueError('a selection is made on the codes of the VQ model: give vq_model')
        if dst is None and mask_dir is not None:
            dst = view_tree.read_dst(mask_dir)
        if dst is None:
            raise ValueError('an edit needs the material dst')
    elif selection is not None or mask_dir is not None or dst is not None:
        raise ValueError(f'selection, mask_dir and dst belong to mode edit, not {mode!r}')
    scene = scene or os.path.basename(os.path.normpath(outroot))
    writer = writer or vis.default_writer()
    probes, olats, first_n = vis.light_names(model)
    vq_olat = bool(vq_model is not None and getattr(vq_model, 'render_olat', False))
    streams = stream_names(scene, mode, probes, olats, first_n, ref_olat=False, vq=vq_model is not None and mode != 'recon', vq_olat=vq_olat)
    relit = dict(relight_olat=True, relight_probes=True) if mode != 'recon' else {}
    white_bg = bool(model.white_bg)
    files = sorted(dataset.files)
    sink = None
    sel_dir = os.path.join(outroot, 'auto_sel')
    if mode == 'edit' and selection is not None:
        view_tree.write_dst(sel_dir, dst)
    try:
        for i, f in enumerate(files):
            batch = dataset.view(f)
            n = batch[5].shape[0]
            kw = dict(relit)
            vq_kw = dict(relit, ref_batch=True)
            if mode != 'recon' and opt_scale is not None:
                # the edit kernel reads the scale on the host; without an edit the models multiply by it on the device
                kw['opt_scale'] = vq_kw['opt_scale'] = opt_scale if mode == 'edit' else \
                    torch.as_tensor(opt_scale, dtype=torch.float32, device=batch[5].device).reshape(1, 3)
            vq_vis = None
            if mode == 'edit':
                if selection is not None:
                    props = None
                    if 'rgb' in selection.needs():
                        props = {'rgb': model.fast_render(batch, mode='test')[0]['rgb']}
                    pred, _, _, vq_vis = vq_model.fast_render(batch, mode='test', edit_material=dst, edit_select=selection, edit_props=props,
                                                              gen_embed=True, **vq_kw)
                    rows = (pred['edit_mask'][:, 0] != 0).to(torch.uint8)
                    host, ev = writer.fetch({'mask': pred['edit_mask']})
                    writer.submit(view_tree.write_selection, os.path.join(sel_dir, view_tree.frame_view(i) + '.npy'),
                                  host['mask'].numpy().reshape(vis.view_hw(vq_vis)), ev)
                else:
                    rows = view_tree.read_selection(os.path.join(mask_dir, view_tree.frame_view(i) + '.npy'), n)
                    rows = torch.as_tensor(rows, device=batch[5].device).to(torch.uint8)
                    if vq_model is not None:
                        _, _, _, vq_vis = vq_model.fast_render(batch, mode='test', edit_material=dst, edit_rows=rows, **vq_kw)
                kw.update(edit_material=dst, edit_rows=rows)
            elif mode == 'relight' and vq_model is not None:
                _, _, _, vq_vis = vq_model.fast_render(batch, mode='test', **vq_kw)
            _, _, _, to_vis = model.fast_render(batch, mode='test', **kw)
            images = frames_of(to_vis, streams, 'ref', white_bg)
            if vq_vis is not None:
                images.update(frames_of(vq_vis, streams, 'vq', white_bg))
            if sink is None:
                H, W = next(iter(images.values())).shape[:2]
                sink = mjpeg.VideoSink(outroot, [s[0] for s in streams], (W, H), fps, mjpeg.JpegEncoder(quality=quality), writer=writer)
            sink.push(images)
            if frames:
                name = view_tree.frame_view(i)
                model.vis_batch(to_vis, os.path.join(outroot, name), mode='test', writer=writer, png=png)
                if vq_vis is not None:
                    vq_model.vis_batch(vq_vis, os.path.join(outroot, 'vq', name), mode='test', writer=writer, png=png)
    finally:
        if sink is not None:
            sink.close()
    writer.flush()
    return {s[0]: os.path.join(outroot, s[0] + '.avi') for s in streams}
