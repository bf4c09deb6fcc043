"""Which materials did the codebook find?  Every VQ code of a trained stage-2 model as a lit sphere -- under the model's own light and
then under each of its novel probes -- with the codes' usage over a set of views.  The spheres are the reference's
decomp/nerfvq_nfr3/brdf/renderer.py SphereRenderer on the device (decomp/nerfactor/util/material_balls.py, csrc/material_balls.hip:
one launch for all codes and probes); the reference itself never shows a code's material on its own.

  run   outdir/materials/ball_{code:02d}_{probe}.png   one ball per code and probe (`light` is the model's own)
        outdir/materials/palette_{probe}.png           the contact sheet, codes ordered by usage (by index without views)
        outdir/materials.json                          per code: albedo, f0, rough, rank, and with views its share of their foreground points

Usage is counted on the device from the `embed` plane of `vis_mat` (the 1-based code of every foreground row) and read once.  The
driver takes the model, as decomp/edit.py and decomp/video.py do (a stage-3 model stands for the stage-2 model it was loaded from)."""
import json
import os

import torch

from vqnerf_release_amd.decomp.nerfactor.util import vis


def _stage2(model):
    return model if hasattr(model, 'vis_mat') else model._stage2


@torch.no_grad()
def usage(model, views, mode='test'):
    """int64 [K] device tensor: the foreground points of `views` (an iterable of view batches) that carry each code"""
    coder = _stage2(model)
    K = coder.num_embed
    counts = torch.zeros((K + 1,), dtype=torch.int64, device=coder.lxyz.device)
    for batch in views:
        embed = coder.vis_mat(batch, mode=mode)[0]['embed']                       # [n, 1]: 1 + code on foreground rows, 0 elsewhere
        counts += torch.bincount(embed.reshape(-1).to(torch.int64), minlength=K + 1)[:K + 1]
    return counts[1:]


def _write(path, data):
    with open(path, 'wb') as f:
        f.write(data)


@torch.no_grad()
def run(model, outdir, views=None, ims=128, spp=4, png=None, probes=True, cols=None, mode='test'):
    """-> the record written to outdir/materials.json.  views: None (codes in index order, no shares) or an iterable of view batches
    (the validation views) whose foreground points are counted per code.  png: None / 'host' (PIL on the host) or 'device' (the PNGs
    are encoded on the device by util/png.PngEncoder, as in the other drivers)."""
    if png not in (None, 'host', 'device'):
        raise ValueError(f"png is None, 'host' or 'device', got {png!r}")
    rows = model.material_rows()
    K = rows.shape[0]
    order, counts = list(range(K)), None
    if views is not None:
        counts = usage(model, views, mode)
        order = torch.argsort(counts, descending=True, stable=True).tolist()
        counts = counts.tolist()
    out = model.material_balls(probes=probes, ims=ims, spp=spp, rows=rows, order=order, cols=cols, want_f32=False, want_u8=True)
    names, u8, sheet = out['names'], out['u8'], out['sheet']
    mat_dir = os.path.join(outdir, 'materials')
    os.makedirs(mat_dir, exist_ok=True)
    ball_paths = [os.path.join(mat_dir, f'ball_{k:02d}_{name}.png') for k in range(K) for name in names]
    sheet_paths = [os.path.join(mat_dir, f'palette_{name}.png') for name in names]
    if png == 'device':
        from vqnerf_release_amd.decomp.nerfactor.util.png import PngEncoder
        enc = PngEncoder()
        for paths, images in ((ball_paths, u8.reshape(-1, ims, ims, 3)), (sheet_paths, sheet)):
            for path, data in zip(paths, enc.encode(images)):
                _write(path, data)
    else:
        for paths, images in ((ball_paths, u8.reshape(-1, ims, ims, 3).cpu().numpy()), (sheet_paths, sheet.cpu().numpy())):
            for path, image in zip(paths, images):
                vis.write_png(path, image)
    rank = {code: r for r, code in enumerate(order)}
    total = sum(counts) if counts is not None else 0
    rows_h = rows.cpu().tolist()
    record = {'probes': names, 'ims': int(ims), 'spp': int(spp), 'order': order, 'codes': []}
    for k in range(K):
        code = {'code': k, 'albedo': rows_h[k][0:3], 'f0': rows_h[k][3:6], 'rough': rows_h[k][6], 'rank': rank[k]}
        if counts is not None:
            code['points'] = int(counts[k])
            code['share'] = counts[k] / total if total else 0.0
        record['codes'].append(code)
    with open(os.path.join(outdir, 'materials.json'), 'w') as f:
        json.dump(record, f, indent=1)
    return record
