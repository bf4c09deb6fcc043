"""Old against new, bit for bit, for a change that must not move a result of the device codecs or of the kernels that took their wave
primitives from csrc/wave.h: two builds of the library -- `--old` (e.g. the parent commit's) and `--new` (default: the tree's) -- are
loaded through VQN_LIB in a fresh child process each, on the same seeded inputs, and the sha256 of every output is compared:

  * JpegEncoder.encode / .coefficients   every case of tests/jpeg_cases.py: the files and the three coefficient planes
  * PngEncoder.encode / .filtered        every case of tests/png_cases.py: the files and the filtered stream
  * _C.image_metrics                     uint8 and float32 pairs, with and without alpha, C in {1, 3}, sizes of IMAGE_HW
  * _C.segmentation_counts               the colour form and the label form, with and without a selection, n in SEG_N
  * _C.material_select_edit              a code set with conditions and an edit: mask, counts, edited tensors, n in MATEDIT_N
  * _C.weight_norm_fwd / _bwd            layer lists of WN_LAYERS

Expected verdict: byte-equal.  Writes {verdict, n_arrays, n_cases, cases, different, missing} as JSON (--out).

    python scripts/compare_codec_kernels.py --old /tmp/libvqnerf_hip_parent.so --out /tmp/codec_same_bits.json"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.compare_train_kernels import sha  # noqa: E402

IMAGE_HW = ((11, 11), (43, 75), (64, 64))
SEG_N = (1, 4097, 70001)
MATEDIT_N = (1, 1025, 40000)
WN_LAYERS = ([(1, 1)], [(3, 39), (256, 256), (257, 100)], [(256, 295), (1, 256), (64, 63)])


def sha_bytes(b):
    return hashlib.sha256(b).hexdigest()


def child(out_path):
    import numpy as np
    import torch
    from tests import jpeg_cases, png_cases
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.decomp.nerfactor.util import mjpeg, png
    from vqnerf_release_amd.decomp.nerfactor.util.metric import gaussian_window
    H = {}

    for name, content, h, w, n, quality, sub, ri in jpeg_cases.encoder_cases():
        enc = mjpeg.JpegEncoder(quality=quality, subsampling=sub, restart_interval=ri)
        dev = torch.tensor(jpeg_cases.batch(content, h, w, n)).cuda()
        files, coef = enc.encode(dev, want_coefficients=True)
        H[f'jpeg/{name}/files'] = sha_bytes(b''.join(files))
        for k, t in enc.coefficients(dev).items():
            H[f'jpeg/{name}/alone_{k}'] = sha(t)
            H[f'jpeg/{name}/coef_{k}'] = sha(coef[k])

    for name, content, h, w, c, n, filters, rows in png_cases.encoder_cases():
        enc = png.PngEncoder(filters=filters, rows_per_segment=png_cases.rows_of(rows, h))
        dev = torch.tensor(png_cases.batch(content, h, w, c, n)).cuda()
        H[f'png/{name}/files'] = sha_bytes(b''.join(enc.encode(dev)))
        H[f'png/{name}/filtered'] = sha(enc.filtered(dev))

    window = gaussian_window()
    for h, w in IMAGE_HW:
        for c in (1, 3):
            rng = np.random.default_rng([h, w, c])
            a8 = torch.tensor(rng.integers(0, 256, (3, h, w, c), dtype=np.uint8)).cuda()
            b8 = torch.tensor(rng.integers(0, 256, (3, h, w, c), dtype=np.uint8)).cuda()
            af, bf = (a8.float() / 255.0).contiguous(), (b8.float() / 255.0).contiguous()
            alpha = torch.tensor(rng.uniform(0, 1, (h, w)).astype(np.float32)).cuda()
            for form, (x, y) in (('u8', (a8, b8)), ('f32', (af, bf))):
                H[f'image_metrics/{h}x{w}x{c}/{form}/plain'] = sha(_C.image_metrics(x, y, window))
                H[f'image_metrics/{h}x{w}x{c}/{form}/alpha'] = sha(_C.image_metrics(x, y, window, alpha=alpha, alpha_thres=0.5))

    for n in SEG_N:
        rng = np.random.default_rng(n)
        pal_gt = rng.integers(0, 256, (5, 3), dtype=np.uint8)
        pal_pd = rng.integers(0, 256, (64, 3), dtype=np.uint8)
        lg, lp = rng.integers(0, 6, n), rng.integers(0, 65, n)                  # 0: a colour of no palette row
        stray = np.array([[1, 2, 3]], np.uint8)
        gt = torch.tensor(np.concatenate([stray, pal_gt])[lg]).cuda()
        pd = torch.tensor(np.concatenate([stray, pal_pd])[lp]).cuda()
        alpha = torch.tensor(rng.uniform(0, 1, n).astype(np.float32)).cuda()
        H[f'seg/n{n}/rgb/all'] = sha(_C.segmentation_counts(gt, pd, gt_palette=pal_gt, pd_palette=pal_pd))
        H[f'seg/n{n}/rgb/alpha'] = sha(_C.segmentation_counts(gt, pd, sel=alpha, alpha_thres=0.3, gt_palette=pal_gt, pd_palette=pal_pd))
        lgt, lpd = torch.tensor(lg.astype(np.int32)).cuda(), torch.tensor(lp.astype(np.int32)).cuda()
        mask = torch.tensor((rng.uniform(0, 1, n) < 0.7).astype(np.uint8)).cuda()
        H[f'seg/n{n}/labels/all'] = sha(_C.segmentation_counts(lgt, lpd, n_gt=5, n_pd=64))
        H[f'seg/n{n}/labels/mask'] = sha(_C.segmentation_counts(lgt, lpd, sel=mask, n_gt=5, n_pd=64))

    for n in MATEDIT_N:
        rng = np.random.default_rng(n)
        rough = torch.tensor(rng.uniform(0, 1, (n, 1)).astype(np.float32)).cuda()
        diff = torch.tensor(rng.uniform(0, 1, (n, 3)).astype(np.float32)).cuda()
        spec = torch.tensor(rng.uniform(0, 1, (n, 3)).astype(np.float32)).cuda()
        embed = torch.tensor(rng.integers(0, 65, n).astype(np.int32)).cuda()
        mask, counts, out = _C.material_select_edit(n, [None, None, None, None, rough], embed=embed, terms=[(4, 0, -1, 0.2, 0.8, 0)], n_conds=1,
                                                    codes=list(range(0, 65, 2)), edit=(diff, spec, rough), dst=[0.1 * i for i in range(1, 8)],
                                                    opt_scale=[0.5, 1.5, 2.0])
        H[f'matedit/n{n}/mask'], H[f'matedit/n{n}/counts'] = sha(mask), sha(counts)
        for i, t in enumerate(t for t in out if t is not None):
            H[f'matedit/n{n}/out{i}'] = sha(t)

    for li, layers in enumerate(WN_LAYERS):
        gen = torch.Generator(device='cuda').manual_seed(li)
        v = [torch.randn(r, c, device='cuda', generator=gen) for r, c in layers]
        g = [torch.randn(r, 1, device='cuda', generator=gen) for r, c in layers]
        dw = [torch.randn(r, c, device='cuda', generator=gen) for r, c in layers]
        w, dv, dg = [torch.empty_like(t) for t in v], [torch.empty_like(t) for t in v], [torch.empty_like(t) for t in g]
        _C.weight_norm_fwd(v, g, w)
        _C.weight_norm_bwd(v, g, dw, dv, dg)
        for i in range(len(layers)):
            H[f'weight_norm/{li}/w{i}'], H[f'weight_norm/{li}/dv{i}'], H[f'weight_norm/{li}/dg{i}'] = sha(w[i]), sha(dv[i]), sha(dg[i])
    torch.cuda.synchronize()
    with open(out_path, 'w') as f:
        json.dump(H, f, indent=0, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', required=True)
    ap.add_argument('--new', default=os.path.join(ROOT, 'vqnerf_release_amd', 'lib', 'libvqnerf_hip.so'))
    ap.add_argument('--out', default=os.path.join(tempfile.gettempdir(), 'codec_same_bits.json'))
    ap.add_argument('--child')
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    got = {}
    for which, lib in (('old', args.old), ('new', args.new)):
        env = dict(os.environ, VQN_LIB=os.path.abspath(lib))
        path = args.out + f'.{which}.json'
        subprocess.run([sys.executable, os.path.abspath(__file__), '--old', args.old, '--child', path], env=env, cwd=ROOT, check=True, timeout=240)
        got[which] = json.load(open(path))
    keys = sorted(set(got['old']) | set(got['new']))
    missing = [k for k in keys if k not in got['old'] or k not in got['new']]
    different = [k for k in keys if k not in missing and got['old'][k] != got['new'][k]]
    verdict = 'byte-equal' if not missing and not different else 'DIFFERENT'
    cases = sorted({k.rsplit('/', 1)[0] for k in keys})
    res = dict(old=os.path.basename(args.old), new=os.path.basename(args.new), verdict=verdict, n_arrays=len(keys), n_cases=len(cases),
               different=different, missing=missing, cases=cases)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(verdict=verdict, n_arrays=len(keys), n_cases=len(cases), different=different[:20], missing=missing[:20])))
    return 0 if verdict == 'byte-equal' else 1


if __name__ == '__main__':
    sys.exit(main())
