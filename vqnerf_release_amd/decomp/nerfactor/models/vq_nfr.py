"""Stage-2 VQ reflectance model: mirror of decomp/nerfvq_nfr3/nerfactor/models/vq_nfr.py
(nets :135-164, init_z :183-195, fast_embed :209-256, fast_render :262-398, vis_mat :400-465, vq_test :467-532,
call :534-692, _render :694-733, light/gamma/get_codebook :735-769, heads :771-828, compute_loss :876-986).
The vis/HTML/video half of the reference file (:988-1302) is out of scope.

Execution paths as in models/nfr_unit.py: fused HIP kernels when no autograd graph is needed, torch statements of
the same arithmetic on the GPU when it is.  The nearest-code search and the EMA statistics are HIP in both
(networks/vq_layers.py)."""
import os

import numpy as np
import torch
import torch.nn as nn

import vqnerf_release_amd

from vqnerf_release_amd.decomp.nerfactor.models.nfr_unit import BrdfModel, fg_rows, ks_split, scatter_rows, take_rows
from vqnerf_release_amd.decomp.nerfactor.networks import mlp
from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.networks.vq_layers import LazyKwargs, LazyResult, VectorQuantizerEMA, l2_normalize_rows
from vqnerf_release_amd.decomp.nerfactor.util import img as imgutil, material_edit, math as mathutil


class _CodebookPrep(torch.autograd.Function):
    """get_codebook(): clip_preserve_gradient(raw, 0, 1) then safe_l2_normalize(axis=0), one launch forward, one backward."""

    @staticmethod
    def forward(ctx, raw):
        x = raw.detach().contiguous()
        ctx.save_for_backward(x)
        return _C.codebook_prep(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return _C.codebook_prep(x, g.float().contiguous())


class _SimSmooth(torch.autograd.Function):
    """weight * (-log(min over code pairs of their distance)) (vq_nfr.py:955-968) on the normalised codebook [D, K]."""

    @staticmethod
    def forward(ctx, cb, weight):
        c = cb.detach().contiguous()
        out4 = _C.sim_smooth_fwd(c, weight)
        ctx.save_for_backward(c, out4)
        ctx.weight = weight
        return out4[0]

    @staticmethod
    def backward(ctx, g):
        c, out4 = ctx.saved_tensors
        return _C.sim_smooth_bwd(c, out4, g.float().reshape(1).contiguous(), ctx.weight), None


class FusedTrainLoss(torch.autograd.Function):
    """The per-point terms of `compute_loss` in train mode (vq_nfr.py:906-981) as one launch forward (`vqn_decomp_loss_fwd`) and one
    backward (`vqn_decomp_loss_bwd`) instead of ~90 + ~120 framework launches.  -> terms [N,5] = rgb, vqrgb, chromaticity,
    chr_smooth, lambert."""

    @staticmethod
    def forward(ctx, rgb_pred, vq_rgb, rgb_gt, z_vq, spec, rough, nerf, w):
        c = lambda t: None if t is None else t.detach().float().contiguous()
        args = (c(rgb_pred), c(vq_rgb), c(rgb_gt), c(z_vq), c(spec), c(rough))
        ctx.args, ctx.nerf, ctx.w = args, nerf, w
        return _C.decomp_loss_fwd(*args, nerf, w)

    @staticmethod
    def backward(ctx, g_terms):
        g_pred, g_vq, g_z, g_spec = _C.decomp_loss_bwd(*ctx.args, ctx.nerf, ctx.w, g_terms.float().contiguous())
        return g_pred, g_vq, None, g_z, g_spec, None, None, None


class _LossTotal(torch.autograd.Function):
    """loss[i] = ((rgb + vqrgb) + vqloss) [+ chromaticity] [+ chr_smooth] [+ sim_smooth] [+ lambert], the reference's order
    (vq_nfr.py:906-981), one launch; backward: the incoming [N] adjoint to the used columns, its sum to the two scalars."""

    @staticmethod
    def forward(ctx, terms, vqloss, sim, use_chr, use_smooth, use_lambert):
        ctx.use = (bool(use_chr), bool(use_smooth), bool(use_lambert))
        ctx.has_sim = sim is not None
        key = (str(terms.device),) + ctx.use
        if key not in _LossTotal._cols:           # (made outside any capture: a host-to-device copy cannot be recorded)
            _LossTotal._cols[key] = torch.tensor([1.0, 1.0, float(ctx.use[0]), float(ctx.use[1]), float(ctx.use[2])], device=terms.device)
        ctx.cols = _LossTotal._cols[key]
        return _C.loss_total(terms.detach().float().contiguous(), vqloss.detach().float().reshape(1).contiguous(),
                             None if sim is None else sim.detach().float().reshape(1).contiguous(), *ctx.use)

    @staticmethod
    def backward(ctx, g):
        gs = g.sum()
        return g[:, None] * ctx.cols[None, :], gs, (gs if ctx.has_sim else None), None, None, None

    _cols = {}


class Model(BrdfModel):
    def __init__(self, config, debug=False):
        self.no_brdf_chunk = config.getboolean('DEFAULT', 'no_brdf_chunk', fallback=True)
        self.seed = config.getint('DEFAULT', 'random_seed', fallback=0)
        self.nfr_ckpt = config.get('DEFAULT', 'nfr_model_ckpt', fallback='')
        super().__init__(config, debug=debug)
        self.brdf_chunk_size = self.config.getint('DEFAULT', 'brdf_chunk_size', fallback=50000)
        self._codebook = None

    def _init_net(self):
        self.num_embed = self.config.getint('DEFAULT', 'num_embed')
        commitment_cost = self.config.getfloat('DEFAULT', 'commitment_cost')
        z = self.z_dim
        vq_head = lambda out: mlp.Network([z, z // 2, out], act=['relu'] * 2 + ['sigmoid'], skip_at=[1])
        net = {'diff_vq': vq_head(3), 'spec_vq': vq_head(3), 'rough_vq': vq_head(1)}    # spec_vq has 3 outputs (vq_nfr.py:143)
        net.update(self._encoder_nets())          # in the reference these five come from the stage-1 checkpoint (:148-155)
        net.update(self._standard_nets('main'))
        self.vq_layer = VectorQuantizerEMA(embedding_dim=z, num_embeddings=self.num_embed,
                                           commitment_cost=commitment_cost, seed=self.seed)
        return net

    def load_stage1(self, nfr_model):
        """Stage hand-off (vq_nfr.py:148-155): share the stage-1 encoder and heads."""
        for dst, src in (('fine_enc', 'fine_enc'), ('bottleneck', 'bottleneck'), ('diff_main', 'diff_out'),
                         ('spec_main', 'spec_out'), ('rough_main', 'rough_out')):
            self.net[dst].load_state_dict(nfr_model.net[src].state_dict())
        if nfr_model._light is not None:
            self.set_light(nfr_model._light.detach().clone())

    # ------------------------------------------------------------------ codebook
    def set_codebook(self, cluster_center):
        """cluster_center [K, z_dim] (k-means centres, the layout of output/cluster/<scene>.npy) -> _codebook [z_dim, K]."""
        cb = torch.as_tensor(cluster_center, dtype=torch.float32).t().contiguous()
        assert tuple(cb.shape) == (self.z_dim, self.num_embed), tuple(cb.shape)
        self._codebook = nn.Parameter(cb.to(self.lxyz.device))

    def get_codebook(self):
        if self._codebook is None:
            path = self.config.get('DEFAULT', 'cluster_center_path')
            self.set_codebook(np.load(path))
        if self.fuse_codebook and self._codebook.is_cuda and self._codebook.dtype == torch.float32:
            return _CodebookPrep.apply(self._codebook)              # the two steps below and their autograd: one launch each way
        cb = mathutil.clip_preserve_gradient(self._codebook, 0.0, 1.0)
        return mathutil.safe_l2_normalize(cb, axis=0)

    fuse_codebook = True       # get_codebook() / the code-separation term on vqn_codebook_prep / vqn_sim_smooth_* (device tensors)

    # ------------------------------------------------------------------ reference-named pieces
    def _pred_enc_at(self, pts):
        return self._pred_bias_at(pts)

    def _pred_diff_at(self, z, vq=False):
        return self._albedo_affine(self._head('diff_vq' if vq else 'diff_main', z))

    def _pred_spec_at(self, z, vq=False):
        return self._head('spec_vq' if vq else 'spec_main', z)

    def _pred_rough_at(self, z, vq=False):
        return self._head('rough_vq' if vq else 'rough_main', z)

    def _thres(self, thres, device):
        if thres is None:
            return None
        return torch.as_tensor(thres, dtype=torch.float32, device=device).reshape(1, self.num_embed)

    fuse_quantise = True       # inference without a graph: normalise + assign + straight-through + loss + usage in one kernel

    def _quantise(self, z_enc, mode, thres, roll=None, want_indices=True):
        """vq_nfr.py:575-578: z_norm = l2_normalize(z_enc), vq_layer(z_norm, codebook).  Two device paths with bit-identical
        `quantize` / indices: the fused kernel when neither a graph nor the EMA statistics are needed, else the sequence
        vqn_l2_normalize_rows -> vqn_vq_assign -> vqn_vq_ste_loss (-> vqn_vq_ema_stats)."""
        codebook = self.get_codebook()
        th = self._thres(thres, z_enc.device)
        on_kernels = z_enc.is_cuda and z_enc.shape[1] % 4 == 0
        if self.fuse_quantise and on_kernels and mode != 'train' and z_enc.shape[1] <= 256 and not self._needs_graph(z_enc):
            vq = self.vq_layer.infer_from_raw(z_enc, codebook, thres=th, roll=roll)
        elif (self.fuse_quantise and on_kernels and mode == 'train' and z_enc.shape[1] <= 256 and z_enc.dtype == torch.float32
              and self.train_backend == 'hip' and os.environ.get('VQN_VQ_TRAIN_FUSED', '1') != '0'):
            vq = self.vq_layer(z_enc, codebook, is_training=True, thres=th, roll=roll, raw=True)     # (round 4: one pass instead of four)
        else:
            z_norm = l2_normalize_rows(z_enc) if on_kernels else mathutil.safe_l2_normalize(z_enc, axis=1)
            vq = self.vq_layer(z_norm, codebook, is_training=(mode == 'train'), thres=th, roll=roll)
        # (the 1-based code map: `call` turns it off in a training step, where the int64 addition was one launch nobody read; the other
        #  entry points read it in every mode)
        return vq, vq['quantize'], vq['loss'], (vq['encoding_indices'] + 1 if want_indices else None)

    fuse_front = True          # inference, K <= 64, no code dropout: encoder -> heads -> VQ step -> VQ heads in ONE launch

    def _cb_frags(self, cb):
        """MFMA fragments + |c|^2 of the (clipped) codebook for the fused front kernel, rebuilt when the parameter changes."""
        # (the parameter object by identity: set_codebook installs a new one, whose storage may land where a freed one's was)
        key = vqnerf_release_amd.WeightsStamp([self._codebook], (str(cb.device), vqnerf_release_amd.weights_epoch()))
        if getattr(self, '_frags_key', None) != key:
            self._frags, self._frags_key = _C.vq_codebook_frags(cb), key
        return self._frags

    def _fused_front(self, pts, mode, thres, full_vis):
        """Everything of `call` between the inputs and the shading in one launch (`vqn_mlp_chain_vq_fwd`): z and the quantised rows
        stay in LDS.  Returns None when the path does not apply (training, code dropout, K > 16, split-precision mode, non-standard
        heads), else (z_enc | None, basecolor, ks, rough, vq, z_vq | None, vq_loss, embed_ind, (vq_albedo, vq_spec, vq_rough), redo)
        with `redo()` -> (z_enc, z_vq) through the separate launches (bit-identical) for whoever asks for the rows later."""
        names_m = [h + '_main' for h in self.HEADS]
        names_v = [h + '_vq' for h in self.HEADS]
        if not (self.fuse_front and self.fuse_quantise and mode != 'train' and thres is None and self.num_embed <= 64
                and self.z_dim == 256 and self.matrix_mode == 'f32' and pts.is_cuda):
            return None
        if not (self._fused(pts) and self._can_fuse_enc_heads(names_m) and self._plan_fits_two_workgroups(names_m)
                and all(self._is_std_head(self.net[n]) and self.net[n].widths[1] <= 128 for n in names_v)):
            return None
        plan_b = self._head_program(names_v, self.z_dim)
        if plan_b.n_waves != 4:
            return None
        plan_a = self._enc_heads_program(names_m)
        wa, da = self._program_pack('enc+heads:' + ','.join(names_m), plan_a, ['fine_enc', 'bottleneck'] + names_m)
        wb, db = self._program_pack('heads:%s:%d:' % (self.matrix_mode, self.z_dim) + ','.join(names_v), plan_b, names_v)
        cb = self.get_codebook().detach().contiguous()
        want_z = bool(full_vis or self.check_numerics)
        want_ste = bool(self.check_numerics or (mode == 'vali' and self.config.getfloat('DEFAULT', 'mat_sloss_weight', fallback=0.0) > 0))
        x = pts.detach().float().contiguous()
        (z, d, s_, r), (vd, vs, vr), idx, ste, e_latent, counts = _C.mlp_chain_vq_fwd(
            da, wa, [self.z_dim] + [self.net[n].widths[-1] for n in names_m], db, wb, [self.net[n].widths[-1] for n in names_v],
            x, self._cb_frags(cb), self.num_embed, want_z=want_z, want_ste=want_ste)
        K = self.num_embed
        redo_box = {}

        def redo():
            if not redo_box:
                ze = self._fused_enc(x)
                redo_box['z'] = ze
                redo_box['zq'] = self.vq_layer.infer_from_raw(ze, cb)['quantize']
            return redo_box['z'], redo_box['zq']

        def perplexity():
            avg = counts / max(idx.numel(), 1)
            return torch.exp(-torch.sum(avg * torch.log(avg + 1e-10)))
        vq = LazyResult({'loss': self.vq_layer.commitment_cost * e_latent, 'encoding_indices': idx},
                        {'quantize': (lambda: ste if ste is not None else redo()[1]), 'perplexity': perplexity,
                         'encodings': lambda: torch.nn.functional.one_hot(idx, K).to(torch.float32),
                         'distances': lambda: _C.vq_assign(_C.l2_normalize_rows(redo()[0]), cb, want_quant=False, want_dist=True)[2]})
        num = self._numerics
        if z is not None:
            z = num(z, 'Z')
        return (z, num(self._albedo_affine(d), 'Albedo'), num(s_, 'Specular'), num(r, 'Roughness'), vq, ste, vq['loss'], idx + 1,
                (num(self._albedo_affine(vd), 'Albedo'), num(vs, 'Specular'), num(vr, 'Roughness')), redo)

    # ------------------------------------------------------------------ entry points
    def init_z(self, batch):
        id_, hw, _, _, _, alpha, pred_alpha, xyz = batch[:8]
        mask = fg_rows(alpha)
        return {'id': id_, 'hw': hw, 'z_pred': self._pred_enc_at(take_rows(mask, xyz))}

    def init_mat(self, z_pred):
        basecolor, ks, rough = self._all_heads(z_pred, 'main')
        return torch.cat([(1 - ks) * basecolor, ks * basecolor, rough], -1)

    def fast_embed(self, batch, mode='train', thres=None, ref_batch=True):
        self._validate_mode(mode)
        id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz = batch[:8]
        mask = fg_rows(alpha)
        n = alpha.shape[0]
        xyz_m = take_rows(mask, xyz)
        _, _, _, embed_ind = self._quantise(self._pred_enc_at(xyz_m), mode, thres)
        pred, gt = {'alpha': pred_alpha}, {'alpha': alpha}
        to_vis = {'id': id_, 'hw': hw, 'embed': scatter_rows(mask, embed_ind[:, None], n), 'xyz': scatter_rows(mask, xyz_m, n),
                  'pred_alpha': pred_alpha, 'gt_alpha': alpha}
        return pred, gt, {'mode': mode}, to_vis

    def vq_test(self, batch, mode='vali', thres=None):
        id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal, lvis = self._unpack(batch)
        mask = fg_rows(alpha)
        rayo, rgb_m, xyz_m, normal_m = take_rows(mask, rayo), take_rows(mask, rgb), take_rows(mask, xyz), take_rows(mask, normal)
        lvis_m = self.fg_lvis(lvis, mask, xyz_m)
        vq, z_vq, vq_loss, _ = self._quantise(self._pred_enc_at(xyz_m), mode, thres)
        usage = (vq['encodings'].max(0, keepdim=True)[0] > 0).to(torch.float32)
        vq_albedo, vq_spec, vq_rough = self._all_heads(z_vq, 'vq')
        vq_rgb = self._shade_or_render(xyz_m, normal_m, rayo, lvis_m, [(vq_albedo, vq_spec, vq_rough)])['rgb'][0]
        loss_kwargs = {'vqloss': vq_loss, 'vqrgb': vq_rgb, 'mode': mode, 'gtc': rgb_m, 'rgb': vq_rgb, 'usage': usage}
        return {'alpha': pred_alpha}, {'alpha': alpha}, loss_kwargs, {'id': id_, 'hw': hw}

    def _shade_or_render(self, xyz, normal, rayo, lvis, materials, split=False, light=None, probes=False):
        """dict(rgb=[per set], normal, rgb_diff, rgb_spec[, rgb_probes]) -- fused kernel without a graph, torch with."""
        if self._fused(xyz, *[t for m in materials for t in m]):
            pr = None
            maps = list(self.novel_probes.values()) if probes is True else list(probes or [])
            if maps:
                pr = torch.stack([torch.as_tensor(lp, dtype=torch.float32, device=xyz.device).reshape(-1, 3) for lp in maps], 0)
            return self._shade(xyz, normal, rayo, lvis, materials, split=split, light=light, probes=pr)
        if self.train_backend == 'hip' and xyz.is_cuda and not split and not probes:
            return self._shade_train(xyz, normal, rayo, lvis, materials, light=light)
        surf2l = self._calc_ldir(xyz)
        surf2c = self._calc_vdir(rayo, xyz)
        n_pred = self._normal_correct(normal, surf2c)
        out = {'rgb': [], 'normal': n_pred, 'rgb_diff': None, 'rgb_spec': None}
        for i, (a, s, r) in enumerate(materials):
            brdf, brdf_s, brdf_d = self._eval_brdf_at(surf2l, surf2c, n_pred, a, s, r)
            rgb, _, rp = self._render(brdf, surf2l, n_pred, lvis, relight_probes=(probes if i == 0 else False), light=light)
            out['rgb'].append(rgb)
            if probes and i == 0:
                out['rgb_probes'] = rp
            if split and i == 0:
                out['rgb_diff'] = self._render(brdf_d, surf2l, n_pred, lvis)[0]
                out['rgb_spec'] = self._render(brdf_s, surf2l, n_pred, lvis)[0]
        return out

    def call(self, batch, mode='train', thres=None, full_vis=False, roll=None):
        self._validate_mode(mode)
        id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal, lvis = self._unpack(batch)
        # `assume_foreground`: the caller guarantees alpha > 0 on every row (outer_sample's batches are), so no boolean
        # gather / scatter -- and no host sync -- is needed
        mask = None if (self.assume_foreground and mode == 'train') else fg_rows(alpha)      # (validation views do have background rows)
        n = alpha.shape[0]
        rayo, rgb_m, xyz_m, normal_m = take_rows(mask, rayo, rgb, xyz, normal)
        lvis_m = self.fg_lvis(lvis, mask, xyz_m)

        front = self._fused_front(xyz_m, mode, thres, full_vis)
        redo = None
        if front is not None:                                 # inference: encoder, heads, VQ step and VQ heads in ONE launch
            z_enc, basecolor, ks, rough, vq, z_vq, vq_loss, embed_ind, (vq_albedo, vq_spec, vq_rough), redo = front
        else:
            z_enc, basecolor, ks, rough = self.enc_and_heads(xyz_m, 'main')       # (one launch on the inference path)
            vq, z_vq, vq_loss, embed_ind = self._quantise(z_enc, mode, thres, roll=roll, want_indices=(mode != 'train'))
            if mode == 'train':                               # codebook is moved by the EMA, outside the optimiser (:582-583)
                with torch.no_grad():
                    self._codebook.copy_(vq['update'])
            if mode == 'train':
                # (the loss's smoothness term reads z_vq too: it takes the rows from the heads' node -- see _all_heads(keep_input))
                vq_albedo, vq_spec, vq_rough, z_vq = self._all_heads(z_vq, 'vq', keep_input=True)
            else:
                vq_albedo, vq_spec, vq_rough = self._all_heads(z_vq, 'vq')

        spec, albedo = ks_split(ks, basecolor)
        sh = self._shade_or_render(xyz_m, normal_m, rayo, lvis_m, [(albedo, spec, rough), (vq_albedo, vq_spec, vq_rough)],
                                   split=(mode != 'train'))
        rgb_pred, vq_rgb, normal_pred = sh['rgb'][0], sh['rgb'][1], sh['normal']

        loss_kwargs = {'vqloss': vq_loss, 'vqrgb': vq_rgb, 'mode': mode, 'gtc': rgb_m, 'rgb': rgb_pred, 'spec': spec,
                       'rough': rough, 'z': z_vq, 'embed': self._codebook}
        if z_vq is None:              # the fused launch kept the quantised rows on the chip: produced on first access (never by `**`)
            del loss_kwargs['z']
            loss_kwargs = LazyKwargs(loss_kwargs, {'z': lambda: redo()[1]})
        srgb = (lambda t: imgutil.linear2srgb(t)) if self.data_type == 'nerf' else (lambda t: t)
        # (train mode: the displayed colour is for visualisation only -- the loss reads loss_kwargs['rgb'], vq_nfr.py:876-905 -- so it
        # is taken from the detached render: one fused launch instead of the torch statement + its never-used autograd records)
        rgb_disp = srgb(rgb_pred.detach() if mode == 'train' else rgb_pred)
        pred = {'rgb': scatter_rows(mask, rgb_disp, n), 'normal': scatter_rows(mask, normal_pred, n),
                'albedo': scatter_rows(mask, albedo, n), 'alpha': pred_alpha, 'spec': scatter_rows(mask, spec, n),
                'rough': scatter_rows(mask, rough, n), 'ks': scatter_rows(mask, ks, n)}
        if mode != 'train':
            pred['rgb_diff'] = scatter_rows(mask, sh['rgb_diff'], n)
            pred['rgb_spec'] = scatter_rows(mask, sh['rgb_spec'], n)
        gt = {'rgb': scatter_rows(mask, rgb_m, n), 'normal': scatter_rows(mask, normal_m, n), 'alpha': alpha}
        to_vis = {'id': id_, 'hw': hw}
        if full_vis:
            to_vis['enc_z'] = scatter_rows(mask, z_enc if z_enc is not None else redo()[0], n)
        if mode != 'train':
            pred['embed'] = scatter_rows(mask, embed_ind[:, None], n)
            pred['vq_rgb'] = scatter_rows(mask, srgb(vq_rgb), n)
            pred['vq_albedo'] = scatter_rows(mask, vq_albedo, n)
            pred['vq_spec'] = scatter_rows(mask, vq_spec, n)
            pred['vq_rough'] = scatter_rows(mask, vq_rough, n)
        for k, v in pred.items():
            to_vis['pred_' + k] = v
        for k, v in gt.items():
            to_vis['gt_' + k] = v
        return pred, gt, loss_kwargs, to_vis

    # The reference ACCEPTS `relight_olat` and then never renders the OLAT maps: its `_render` ends in
    # `return rgb, None, rgb_probes` (vq_nfr.py:733), so `pred` holds no 'rgb_olat' there whatever the flag says (:349, :385).
    # That is the default here.  `render_olat = True` opts into rendering them (upstream NeRFactor's behaviour) in the same
    # shading pass as the probes.
    render_olat = False

    def fast_render(self, batch, mode='train', relight_olat=False, relight_probes=False, opt_scale=None, edit_mask=None,
                    edit_material=None, ref_batch=False, dst_env=None, gen_embed=False, thres=None, vis_scale=False, edit_select=None,
                    edit_rows=None, edit_props=None):
        """edit_select (a material_edit.Selection): the edited rows are picked in place from this call's own pre-edit albedo / spec /
        rough, xyz and code index (the quantiser step runs as under gen_embed, honouring `thres`) on the foreground rows; a condition on
        rgb / rgb_scale reads edit_props={'rgb': [n, 3]} from the caller; pred['edit_mask'] (float [n, 1], 0 on the background) is the
        selection.  edit_rows: a uint8 [n] device mask over all rows, applied as edit_mask is.  Either way selection, edit and the
        opt_scale scaling are ONE launch of csrc/material_edit.hip (opt_scale is then read on the host: pass host values to avoid a
        synchronisation).  With both left at None the body runs exactly as it did without them."""
        self._validate_mode(mode)
        kernel_edit = material_edit.check_edit_keywords(edit_mask, edit_material, edit_select, edit_rows, edit_props)
        relight_olat = bool(relight_olat and self.render_olat)
        id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal = batch[:9]
        lvis = batch[-1] if self.data_type == 'nerf' else None
        mask = fg_rows(alpha)
        n = alpha.shape[0]
        rayo, rgb_m, xyz_m, normal_m = take_rows(mask, rayo), take_rows(mask, rgb), take_rows(mask, xyz), take_rows(mask, normal)
        lvis_m = self.fg_lvis(lvis, mask, xyz_m)
        if edit_mask is not None:
            edit_mask = (take_rows(mask, edit_mask)[..., 0:1] > 0).to(torch.float32)
        z_enc, basecolor, ks, rough = self.enc_and_heads(xyz_m, 'main')
        if gen_embed or edit_select is not None:
            _, _, _, embed_ind = self._quantise(z_enc, mode, thres)
        spec, albedo = ks_split(ks, basecolor)
        scaled = (opt_scale is not None) and (not vis_scale)
        picked = None
        if kernel_edit:
            picked, albedo, spec, rough, s_albedo, s_spec = material_edit.edit_rows_of_a_view(
                mask, albedo, spec, rough, xyz_m, embed_ind if edit_select is not None else None, edit_material, edit_select, edit_rows,
                edit_props, opt_scale if scaled else None)
        if edit_mask is not None:
            upd = lambda src, v: src * (1 - edit_mask) + edit_mask * torch.as_tensor([v], dtype=torch.float32, device=src.device)
            if not edit_material['diff'][0] < 0:
                albedo = upd(albedo, edit_material['diff'])
            if not edit_material['spec'][0] < 0:
                spec = upd(spec, edit_material['spec'])
            if not edit_material['rough'][0] < 0:
                rough = upd(rough, edit_material['rough'])
        if not kernel_edit:
            s_albedo, s_spec = (albedo * opt_scale, spec * opt_scale) if scaled else (albedo, spec)
        light = None if dst_env is None else self.novel_probes[dst_env]
        # every relighting condition of this call -- OLAT maps first, then the probes -- goes through ONE shading pass
        n_olat = len(self.novel_olat) if relight_olat else 0
        maps = (list(self.novel_olat.values()) if relight_olat else []) + (list(self.novel_probes.values()) if relight_probes else [])
        sh = self._shade_or_render(xyz_m, normal_m, rayo, lvis_m, [(s_albedo, s_spec, rough)], light=light, probes=maps or False)
        rgb_pred = sh['rgb'][0]
        srgb = (lambda t: imgutil.linear2srgb(t)) if self.data_type == 'nerf' else (lambda t: t)
        if (opt_scale is not None) and vis_scale:
            basecolor = imgutil.linear2srgb(basecolor) * opt_scale
            spec = imgutil.linear2srgb(spec) * opt_scale
        pred = {'alpha': pred_alpha, 'basecolor': scatter_rows(mask, basecolor, n), 'albedo': scatter_rows(mask, albedo, n),
                'spec': scatter_rows(mask, spec, n), 'rough': scatter_rows(mask, rough, n)}
        if gen_embed:
            pred['embed'] = scatter_rows(mask, embed_ind[:, None], n)
        if picked is not None:
            pred['edit_mask'] = scatter_rows(mask, picked.to(torch.float32)[:, None], n)
        if dst_env is not None:
            pred['rgb'] = scatter_rows(mask, srgb(rgb_pred), n)
        if relight_olat and n_olat > 0:
            pred['rgb_olat'] = scatter_rows(mask, srgb(sh['rgb_probes'][:, :n_olat]), n)
        if relight_probes and len(maps) > n_olat:
            pred['rgb_probes'] = scatter_rows(mask, srgb(sh['rgb_probes'][:, n_olat:]), n)
        gt = {'rgb': scatter_rows(mask, rgb_m, n), 'alpha': alpha}
        to_vis = {'id': id_, 'hw': hw}
        for k, v in pred.items():
            to_vis['pred_' + k] = v
        for k, v in gt.items():
            to_vis['gt_' + k] = v
        return pred, gt, {'mode': mode, 'gtc': rgb_m}, to_vis

    # ------------------------------------------------------------------ the codebook's materials on their own
    @torch.no_grad()
    def material_rows(self):
        """float32 [K, 7] = albedo[3], spec (f0)[3], rough[1] of every code: the VQ heads evaluated on the K prepared codes (the
        columns of get_codebook(), which are the rows `quantize` holds for a point that sits on its code) through the same
        `_all_heads(z_vq, 'vq')` that `call` runs, so row k is what the VQ branch gives a point quantised to code k."""
        codes = self.get_codebook().detach().t().contiguous()
        albedo, spec, rough = self._all_heads(codes, 'vq')
        return torch.cat([albedo, spec.expand(-1, 3), rough], -1).contiguous()

    materials_slab = 1 << 18   # points per pass of materials_at (a point's 256-wide rows are 1 KiB each way)

    @torch.no_grad()
    def materials_at(self, xyz, thres=None, mode='test'):
        """The materials at points xyz [N, 3] alone (a point's material depends on nothing else) -> dict of device tensors:
        code int32 [N] (0-based: `embed` of vis_mat / fast_embed is code + 1); basecolor [N, 3], ks [N, 1], rough [N, 1] from the
        main heads (vis_mat's albedo is (1 - ks) * basecolor, its spec ks * basecolor); vq_albedo [N, 3], vq_spec [N, 3 | 1],
        vq_rough [N, 1] from the VQ heads on the quantised row, as `call` shows them (that row is the straight-through x + (q - x),
        equal to the code q to an ulp, so they agree with material_rows()[code] to rounding, not bit for bit).  The same
        kernels as `call` and vis_mat: the fused front (one launch) where it applies, else encoder, quantiser step and the two head
        families as separate launches; the rows are bit-identical either way.  In slabs of materials_slab points; no host read."""
        self._validate_mode(mode)
        _C.require_device(xyz, 'materials_at')
        x = xyz.detach().reshape(-1, 3).float().contiguous()
        n, dev = x.shape[0], x.device
        if n == 0:
            raise _C.VqnError('materials_at: no points')
        out = None
        for s in range(0, n, self.materials_slab):
            pts = x[s: s + self.materials_slab]
            front = self._fused_front(pts, mode, thres, False)
            if front is not None:
                _, basecolor, ks, rough, vq, _, _, _, vq_heads, _ = front
            else:
                z_enc = self._pred_enc_at(pts)
                vq, z_vq, _, _ = self._quantise(z_enc, mode, thres, want_indices=False)
                basecolor, ks, rough = self._all_heads(z_enc, 'main')
                vq_heads = self._all_heads(z_vq, 'vq')
            rows = {'code': vq['encoding_indices'].reshape(-1).to(torch.int32), 'basecolor': basecolor, 'ks': ks, 'rough': rough,
                    'vq_albedo': vq_heads[0], 'vq_spec': vq_heads[1], 'vq_rough': vq_heads[2]}
            if out is None:
                out = {k: torch.empty((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev) for k, v in rows.items()}
            for k, v in rows.items():
                out[k][s: s + pts.shape[0]] = v
        return out

    def vis_mat(self, batch, mode='train', opt_scale=None, ref_batch=False, thres=None):
        self._validate_mode(mode)
        id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz = batch[:8]
        mask = fg_rows(alpha)
        n = alpha.shape[0]
        z_enc = self._pred_enc_at(take_rows(mask, xyz))
        _, _, _, embed_ind = self._quantise(z_enc, mode, thres)
        basecolor, ks, rough = self._all_heads(z_enc, 'main')
        pred = {'alpha': pred_alpha, 'albedo': scatter_rows(mask, (1 - ks) * basecolor, n),
                'spec': scatter_rows(mask, ks * basecolor, n), 'rough': scatter_rows(mask, rough, n),
                'embed': scatter_rows(mask, embed_ind[:, None], n)}
        gt = {'alpha': alpha}
        to_vis = {'id': id_, 'hw': hw}
        for k, v in pred.items():
            to_vis['pred_' + k] = v
        to_vis['gt_alpha'] = alpha
        return pred, gt, {'mode': mode}, to_vis

    # ------------------------------------------------------------------ loss
    @staticmethod
    def _rgb2chromaticity(rgb):
        den = torch.sqrt((rgb * rgb).sum(-1, keepdim=True))
        return mathutil.divide_no_nan(rgb, den * torch.ones_like(rgb))

    fuse_train_loss = True     # train mode on the device: the per-point loss terms and their gradients as two launches (FusedTrainLoss)

    def _sim_smooth(self, cfg):
        """Code-separation term (vq_nfr.py:955-968) -- a scalar over the K x K code distances, torch statement."""
        cbn = self.get_codebook()
        if self.fuse_codebook and cbn.is_cuda and 2 <= cbn.shape[1] <= 256:
            return _SimSmooth.apply(cbn, float(cfg('sim_loss_weight')))
        cb = cbn.t()
        K = cb.shape[0]
        eye = torch.eye(K, dtype=cb.dtype, device=cb.device)
        # the diagonal is exactly 0 and masked below; "+ eye" only keeps d sqrt / dx finite there (TF's SqrtGrad
        # yields 0 for a 0 incoming gradient, torch would give 0 * inf)
        dist = torch.sqrt(((cb[:, None, :] - cb[None, :, :]) ** 2).sum(-1) + eye) * (1 - eye)
        masked = dist * (1 - eye) + eye * dist.max()
        return cfg('sim_loss_weight') * (-torch.log(masked.min()))

    def _compute_loss_train_fused(self, rgb_gt, rgb_pred, vq_rgb, kwargs, cfg):
        """The train branch of compute_loss (vq_nfr.py:906-986) with the per-point terms on `FusedTrainLoss`; same dict keys, same
        values (tests/test_gpu_decomp.py: against the torch statement and, through it, the oracle)."""
        w = {'rgb': cfg('combine_weight'), 'chr': max(cfg('chromaticity_loss_weight'), 0.0), 'smooth': max(cfg('mat_sloss_weight'), 0.0),
             'alpha': cfg('chr_alpha'), 'thres': cfg('chr_thres'), 'lambert': max(cfg('lambert_weight'), 0.0)}
        z_vq = kwargs.pop('z') if w['smooth'] > 0 else None
        spec, rough = (kwargs.pop('spec'), kwargs.pop('rough')) if w['lambert'] > 0 else (None, None)
        terms = FusedTrainLoss.apply(rgb_pred, vq_rgb, rgb_gt, z_vq, spec, rough, self.data_type == 'nerf', w)
        wq = cfg('vq_loss_weight')                         # (1.0 in the reference's config: x * 1.0 is x exactly -- not worth two launches)
        ld = {'rgb': terms[:, 0], 'vqrgb': terms[:, 1], 'vqloss': kwargs.pop('vqloss') if wq == 1.0 else wq * kwargs.pop('vqloss')}
        # the per-point total in the reference's own order, ONE launch (vqn_loss_total; seven framework launches before)
        if w['chr'] > 0:
            ld['chromaticity'] = terms[:, 2]
        if w['smooth'] > 0:
            ld['chr_smooth'] = terms[:, 3]
        sim = None
        if cfg('sim_loss_weight') > 0:
            sim = ld['sim_smooth'] = self._sim_smooth(cfg)
        if w['lambert'] > 0:
            ld['lambert'] = terms[:, 4]
        loss = _LossTotal.apply(terms, ld['vqloss'], sim, w['chr'] > 0, w['smooth'] > 0, w['lambert'] > 0)
        ld['loss'] = loss
        return self._numerics(loss, 'Loss'), ld

    def compute_loss(self, pred, gt, **kwargs):
        cfg = lambda k: self.config.getfloat('DEFAULT', k)
        mse = lambda a, b: ((a - b) ** 2).mean(-1)
        mode = kwargs.pop('mode')
        rgb_gt, rgb_pred = kwargs.pop('gtc'), kwargs.pop('rgb')
        if mode == 'train' and self.fuse_train_loss and self.train_backend == 'hip' and rgb_pred.is_cuda:
            return self._compute_loss_train_fused(rgb_gt, rgb_pred, kwargs.pop('vqrgb'), kwargs, cfg)
        if self.data_type == 'nerf':
            linear_gt, srgb_pred = imgutil.srgb2linear(rgb_gt), imgutil.linear2srgb(rgb_pred)
        else:
            linear_gt, srgb_pred = rgb_gt, rgb_pred
        ld = {}
        vq_rgb = kwargs.pop('vqrgb')
        if mode != 'train':
            ld['rgb'] = mse(rgb_gt, srgb_pred)
            ld['vqrgb'] = mse(rgb_gt, imgutil.linear2srgb(vq_rgb))
            ld['chromaticity'] = mse(self._rgb2chromaticity(linear_gt), self._rgb2chromaticity(vq_rgb))
            return ld['rgb'] + ld['vqrgb'] + ld['chromaticity'], ld
        ld['rgb'] = cfg('combine_weight') * mse(linear_gt, rgb_pred)
        ld['vqrgb'] = mse(linear_gt, vq_rgb)
        ld['vqloss'] = cfg('vq_loss_weight') * kwargs.pop('vqloss')
        loss = ld['rgb'] + ld['vqrgb'] + ld['vqloss']
        schr_gt = self._rgb2chromaticity(rgb_gt)
        if cfg('chromaticity_loss_weight') > 0:
            ld['chromaticity'] = cfg('chromaticity_loss_weight') * mse(self._rgb2chromaticity(linear_gt),
                                                                        self._rgb2chromaticity(vq_rgb))
            loss = loss + ld['chromaticity']
        if cfg('mat_sloss_weight') > 0:                       # pairs [p, p_neighbour] are interleaved (train_nfr.py:447-448)
            z_vq = kwargs.pop('z')
            e = torch.sqrt(((schr_gt[::2] - schr_gt[1::2]) ** 2).sum(-1))
            e = torch.where(e > cfg('chr_thres'), e, torch.zeros_like(e))
            sl = torch.exp(-cfg('chr_alpha') * e) * (1.0 - (z_vq[::2] * z_vq[1::2]).sum(-1))
            ld['chr_smooth'] = cfg('mat_sloss_weight') * torch.stack([sl, sl], -1).reshape(-1)
            loss = loss + ld['chr_smooth']
        if cfg('sim_loss_weight') > 0:                        # keep the code vectors apart (:955-968)
            cb = self.get_codebook().t()
            K = cb.shape[0]
            eye = torch.eye(K, dtype=cb.dtype, device=cb.device)
            # the diagonal is exactly 0 and masked below; "+ eye" only keeps d sqrt / dx finite there (TF's SqrtGrad
            # yields 0 for a 0 incoming gradient, torch would give 0 * inf)
            dist = torch.sqrt(((cb[:, None, :] - cb[None, :, :]) ** 2).sum(-1) + eye) * (1 - eye)
            masked = dist * (1 - eye) + eye * dist.max()
            ld['sim_smooth'] = cfg('sim_loss_weight') * (-torch.log(masked.min()))
            loss = loss + ld['sim_smooth']
        if cfg('lambert_weight') > 0:
            spec, rough = kwargs.pop('spec'), kwargs.pop('rough')
            r = rough.detach()
            r = torch.where(r < 0.5, torch.zeros_like(r), 2 * r - 1.0)
            ld['lambert'] = cfg('lambert_weight') * spec.max(-1)[0] * r[:, 0]
            loss = loss + ld['lambert']
        ld['loss'] = loss
        return self._numerics(loss, 'Loss'), ld
