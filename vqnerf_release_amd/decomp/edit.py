"""Material editing over the views of a scene: select a material by its VQ code (optionally narrowed by bounds on other per-pixel
properties), replace it, and re-render every view under the original or a new light -- the loop of the reference's
decomp/nerfvq_nfr3/nerfactor/offline_edit.py:183-205 (with edit.py:213-230 for a new light) with the selection made on the device
(decomp/nerfactor/util/material_edit.py) where the reference reads masks a PyQt window wrote (ui4_offline.py `map_f`).

  run                 per view: vq_model.fast_render(edit_select=...) makes the mask and the edited stage-2 render in one pass; the same
                      mask goes to the stage-3 model; both write into outroot/<name>/ through the asynchronous vis_batch; the mask is
                      also written as the UI writes it (outroot/auto_sel/<name>.npy, bool [H, W, 3], and auto_sel/dst.json), so that
                      the reference's own scripts could consume it (those file forms, like the walk over the view directories, the
                      loaders and the size check of the file form below, are decomp/view_tree.py's);
  select_views        the file form of `map_f`: the same selection from the files of rendered views, evaluated on the device;
  compute_rgb_scales  offline_edit.py:52-120: the per-channel scale that matches predicted albedo (+ spec) to the ground truth.

One deviation from the reference: its `mat` property reads the SOURCE view's files for every view (ui4_offline.py:295-297), a slip;
here every view tests its own values.  Not here: the polling server around edit.py's loop (status.json), the PyQt window, its preset
table of named materials, and cv2 resizing of masks (a size mismatch raises)."""
import os

import numpy as np
import torch

from vqnerf_release_amd import parallel
from vqnerf_release_amd.decomp import view_tree
from vqnerf_release_amd.decomp.nerfactor.util import img as imgutil
from vqnerf_release_amd.decomp.nerfactor.util import material_edit, vis
from vqnerf_release_amd.decomp.nerfactor.util.segmentation import _UNIT8

_FILES = {'rgb': 'pred_rgb.png', 'diff': 'pred_albedo.png', 'spec': 'pred_spec.png', 'rough': 'pred_rough.png'}       # ui4_offline.py:28-31


def write_preview(model, dst, outroot, relight_probes=True, ims=128, spp=4):
    """outroot/dst_preview_{probe}.png: the replacement material `dst` as a lit sphere under the model's light (`light`) and, with
    relight_probes, its novel probes (decomp/nerfactor/util/material_balls.py).  A part of dst the edit leaves alone (first component
    negative) has no value of its own: it is shown as 0 (diff, spec) or 1 (rough).  -> the paths written."""
    from vqnerf_release_amd.decomp.nerfactor.util import material_balls
    row = material_balls.material_row({k: (dst[k] if not np.asarray(dst[k], np.float64).reshape(-1)[0] < 0 else
                                           ([1.0] if k == 'rough' else [0.0, 0.0, 0.0])) for k in ('diff', 'spec', 'rough')})
    out = model.material_balls(probes=relight_probes, ims=ims, spp=spp, rows=torch.as_tensor(row, device=model.lxyz.device)[None],
                               want_f32=False, want_u8=True)
    os.makedirs(outroot, exist_ok=True)
    paths = [os.path.join(outroot, f'dst_preview_{name}.png') for name in out['names']]
    for path, image in zip(paths, out['u8'][0].cpu().numpy()):
        vis.write_png(path, image)
    return paths


@torch.no_grad()
def run(vq_model, dataset, outroot, selection, dst, ref_model=None, ref_dataset=None, opt_scale=None, relight_probes=True, dst_env=None,
        view_name=view_tree.batch_view, writer=None, num_p=None, p_i=None, png='host', preview=False):
    """Every view of `dataset` (sharded as in train_nfr.render_views: process p_i of num_p takes views p_i, p_i + num_p, ...):
    vq_model.fast_render(edit_select=selection, edit_material=dst, opt_scale, relight_probes | dst_env) -> the mask and the edited
    stage-2 render; with ref_model (and ref_dataset, the same views with the stage-3 inputs; not under dst_env, as in edit.py:225-230)
    ref_model.fast_render(edit_rows=that mask, opt_scale).  Files: outroot/<name>/ by vis_batch (pred_edit_mask.png and embed_map.png
    among them; the two models write the files both know with the same content), outroot/auto_sel/<name>.npy and auto_sel/dst.json.  If a condition
    names rgb, a plain render of the view comes first (the stage-3 model's if given, else the stage-2 model's `call`) and feeds it.
    png is handed to vis_batch ('device': the PNGs are encoded on the device).  preview=True also writes outroot/dst_preview_{probe}.png,
    the ball of the replacement row (write_preview), before the first view is relit.
    -> (writer, {name: selected pixels}), the counts read from the device once, at the end."""
    if not isinstance(selection, material_edit.Selection):
        raise ValueError(f'selection is a material_edit.Selection, got {type(selection).__name__}')
    if (ref_model is None) != (ref_dataset is None):
        raise ValueError('ref_model and ref_dataset are given together')
    if num_p is None:
        num_p, p_i = parallel.world_size(), parallel.rank()
    writer = writer or vis.default_writer()
    files = sorted(dataset.files)
    ref_files = sorted(ref_dataset.files) if ref_dataset is not None else None
    if ref_files is not None and len(ref_files) != len(files):
        raise ValueError(f'the two datasets differ in their views: {len(files)} and {len(ref_files)}')
    sel_dir = os.path.join(outroot, 'auto_sel')
    if p_i == 0:
        view_tree.write_dst(sel_dir, dst)
        if preview:
            write_preview(vq_model, dst, outroot, relight_probes=relight_probes)
    os.makedirs(sel_dir, exist_ok=True)
    needs_rgb = 'rgb' in selection.needs()
    names, counts = [], []
    for i, f in enumerate(files):
        if i % num_p != p_i:
            continue
        name = view_name(i)
        batch = dataset.view(f)
        ref_batch = ref_dataset.view(ref_files[i]) if ref_dataset is not None else None
        props = None
        if needs_rgb:
            plain = ref_model.fast_render(ref_batch, mode='test')[0] if ref_model is not None else vq_model.call(batch, mode='test')[0]
            props = {'rgb': plain['rgb']}
        pred, _, _, to_vis = vq_model.fast_render(batch, mode='test', opt_scale=opt_scale, relight_probes=relight_probes and dst_env is None,
                                                  dst_env=dst_env, ref_batch=True, gen_embed=True, edit_material=dst, edit_select=selection,
                                                  edit_props=props)
        picked = pred['edit_mask']
        outdir = os.path.join(outroot, name)
        if ref_model is not None and dst_env is None:
            rows = (picked[:, 0] != 0).to(torch.uint8)
            _, _, _, ref_vis = ref_model.fast_render(ref_batch, mode='test', opt_scale=opt_scale, edit_material=dst, edit_rows=rows)
            ref_model.vis_batch(ref_vis, outdir, mode='test', writer=writer, png=png)
        vq_model.vis_batch(to_vis, outdir, mode='test', writer=writer, png=png)
        host, ev = writer.fetch({'mask': picked})
        writer.submit(view_tree.write_selection, os.path.join(sel_dir, name + '.npy'), host['mask'].numpy().reshape(vis.view_hw(to_vis)), ev)
        names.append(name)
        counts.append(picked.sum())
    totals = torch.stack(counts).tolist() if counts else []
    return writer, {n: int(c) for n, c in zip(names, totals)}


# ---- the file form -------------------------------------------------------------------------------------------------------------
def view_props(view_dir, selection, device='cuda'):
    """the files of one rendered view the selection names -> ({prop: float32 [H * W, ch]}, int32 labels or None, (H, W)); bytes become
    floats through the / 255 host table of util/segmentation.py (correctly rounded, where a device division may not be)"""
    unit = torch.as_tensor(_UNIT8, device=device)
    props, shapes = {}, {}
    for p in selection.needs():
        if p == 'xyz':
            path = os.path.join(view_dir, 'xyz.npy')
            path = path if os.path.exists(path) else os.path.join(view_dir, 'pred_xyz.npy')                  # ui4_offline.py:305-306
            a = np.load(path).astype(np.float32)
            shapes[path], props[p] = a.shape[:2], torch.as_tensor(a, device=device).reshape(-1, 3)
        else:
            path = os.path.join(view_dir, _FILES[p])
            a = view_tree.read_image(path, 'L' if p == 'rough' else 'RGB')
            shapes[path] = a.shape[:2]
            props[p] = unit[torch.as_tensor(a, device=device).long()].reshape(-1, 1 if p == 'rough' else 3)
    labels = None
    if selection.codes is not None:
        path = os.path.join(view_dir, 'embed_map.png')
        a = view_tree.read_image(path)
        shapes[path], labels = a.shape[:2], vis.embed_labels(a, device)
    return props, labels, view_tree.check_sizes(view_dir, shapes)


def select_views(pred_root, selection, dst=None, src_view=None, device='cuda'):
    """The file form of `map_f`: for every view directory of pred_root (`batch*` / `test*`) the selection from embed_map.png,
    pred_rgb.png, pred_albedo.png, pred_spec.png, pred_rough.png and xyz.npy (else pred_xyz.npy) -- only the ones the selection names
    -- evaluated on the device.  Writes pred_root/../auto_sel/<basename of pred_root>/<view>.npy (bool [H, W, 3]), dst.json there when
    dst is given, and edit_mask.png of `src_view` (a view's name), as the UI does (ui4_offline.py:267-271, :333-338).
    -> {view: selected pixels}, read from the device once, at the end."""
    if not isinstance(selection, material_edit.Selection):
        raise ValueError(f'selection is a material_edit.Selection, got {type(selection).__name__}')
    pred_root = pred_root.rstrip('/')
    sel_dir = os.path.join(os.path.dirname(pred_root), 'auto_sel', os.path.basename(pred_root))
    os.makedirs(sel_dir, exist_ok=True)
    if dst is not None:
        view_tree.write_dst(sel_dir, dst)
    views, counts = view_tree.view_dirs(pred_root, view_tree.EDIT_VIEWS), []
    if src_view is not None and src_view not in views:
        raise ValueError(f'src_view {src_view!r} is not a view of {pred_root}')
    for v in views:
        props, labels, hw = view_props(os.path.join(pred_root, v), selection, device)
        res = material_edit.select(props, selection, embed=labels)
        m = view_tree.write_selection(os.path.join(sel_dir, v + '.npy'), res['mask'].cpu().numpy().reshape(hw))
        if v == src_view:
            vis.write_png(os.path.join(sel_dir, 'edit_mask.png'), (np.where(m, 1.0, 0.0) * 255).astype(np.uint8))
        counts.append(res['selected'])
    totals = torch.stack(counts).tolist() if counts else []
    return {v: int(c) for v, c in zip(views, totals)}


def compute_rgb_scales(pred_root, gt_root, vis_root, with_spec=False, device='cuda'):
    """offline_edit.py:52-120.  Per view directory batch<i> of pred_root: prediction = pred_albedo.png + pred_spec.png, ground truth =
    vis_root/val_<i:03d>/albedo.png (+ metal.png when with_spec: the reference's list of scenes is the caller's business), alpha =
    gt_root/val_<i:03d>/rgba.png; both sides through linear2srgb; the per-channel ratio of the alpha-weighted means, ground truth over
    prediction, per view; then the mean over views.  float64 on the device -> float64 [3] (device).  The reference resizes the ground
    truth to the prediction; here a size mismatch raises, as in metric_eval."""
    dev = torch.device(device)
    load = lambda path, mode='RGB': torch.as_tensor(view_tree.read_image(path, mode), device=dev).to(torch.float64) / 255.0
    ratios = []
    for name in view_tree.view_dirs(pred_root, view_tree.BATCH_VIEWS):
        view = view_tree.gt_view(name)
        pred = load(os.path.join(pred_root, name, 'pred_albedo.png')) + load(os.path.join(pred_root, name, 'pred_spec.png'))
        gt = load(os.path.join(vis_root, view, 'albedo.png'))
        if with_spec:
            gt = gt + load(os.path.join(vis_root, view, 'metal.png'))
        alpha = load(os.path.join(gt_root, view, 'rgba.png'), 'RGBA')[..., 3]
        view_tree.check_sizes(name, {'prediction': pred.shape[:2], 'ground truth': gt.shape[:2], 'alpha': alpha.shape})
        gt, pred = imgutil.linear2srgb(gt), imgutil.linear2srgb(pred)
        a = alpha[..., None]
        ratios.append(((gt * a).sum((0, 1)) / a.sum()) / ((pred * a).sum((0, 1)) / a.sum()))
    if not ratios:
        raise ValueError(f'{pred_root}: no view directory batch<i>')
    return torch.stack(ratios).mean(0)
