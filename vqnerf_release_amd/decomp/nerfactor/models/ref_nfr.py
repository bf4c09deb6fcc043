"""Stage-3 residual-baking model: mirror of decomp/nerfvq_nfr3/nerfactor/models/ref_nfr.py (nets :137-159, call :176-300,
fast_render :303-418, _pred_ref_at :487-496, compute_loss :584-610; vis / HTML are out of scope).

The encoder (`fine_enc`, `bottleneck`) and the specular head come frozen from the stage-2 vq_nfr model; a new `rgb_enc`
(3 -> 256 -> 256 -> 256) embeds the per-point reference colour and the diffuse / roughness heads read [z_xyz ; z_ref]
(512 wide).  Same kernels as the other stages: `vqn_mlp_chain_fwd` programs (incl. a 512-wide head program and a
3-feature raw-input program) and the fused shading forward / backward."""
import torch

from vqnerf_release_amd.decomp import packing
from vqnerf_release_amd import _C
from vqnerf_release_amd.decomp.nerfactor.models.nfr_unit import BrdfModel, fg_rows, scatter_rows, take_rows
from vqnerf_release_amd.decomp.nerfactor.networks import mlp
from vqnerf_release_amd.decomp.nerfactor.util import img as imgutil, material_edit


class Model(BrdfModel):
    def __init__(self, config, debug=False):
        self.no_brdf_chunk = config.getboolean('DEFAULT', 'no_brdf_chunk', fallback=True)
        self.vqnfr_ckpt = config.get('DEFAULT', 'vqnfr_model_ckpt', fallback='')
        super().__init__(config, debug=debug)

    def _init_net(self):
        z = self.z_dim
        net = self._encoder_nets()
        net['spec_out'] = mlp.Network([z, z // 2, 1], act=['relu'] * 2 + ['sigmoid'], skip_at=[1])
        net['rgb_enc'] = mlp.Network([z, z, z], act=[None, 'relu', 'sigmoid'])
        net['diff_out'] = mlp.Network([z, z // 2, 3], act=['relu'] * 2 + ['sigmoid'], skip_at=[1])
        net['rough_out'] = mlp.Network([z, z // 2, 1], act=['relu'] * 2 + ['sigmoid'], skip_at=[1])
        return net

    def build_nets(self, device=None, seed=None):
        gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
        d_xyz = getattr(self.embedder['xyz'], 'out_dims', 3)
        d_in = {'fine_enc': d_xyz, 'bottleneck': self.config.getint('DEFAULT', 'mlp_width'), 'spec_out': self.z_dim, 'rgb_enc': 3,
                'diff_out': 2 * self.z_dim, 'rough_out': 2 * self.z_dim}
        for name, net in self.net.items():
            net.build(d_in[name], device=device, generator=gen)
        self.register_trainable()
        return self

    def load_stage2(self, vq_model):
        """Stage hand-off (ref_nfr.py:141-146): frozen encoder + specular head of the vq_nfr model, and its light."""
        for dst, src in (('fine_enc', 'fine_enc'), ('bottleneck', 'bottleneck'), ('spec_out', 'spec_main')):
            self.net[dst].load_state_dict(vq_model.net[src].state_dict())
            for p in self.net[dst].parameters():
                p.requires_grad_(False)
        if vq_model._light is not None:
            self.set_light(vq_model.light.detach().clone())       # what stage 2 saved to np_light.npy: the clipped light
        # for material_rows (this model has no codebook of its own); past nn.Module's registration: stage 2 is no submodule of stage 3,
        # its parameters are not this model's
        self.__dict__['_stage2'] = vq_model

    _stage2 = None

    def material_rows(self):
        """float32 [K, 7]: the code materials of the stage-2 model whose frozen encoder this one carries (vq_nfr.Model.material_rows).
        Stage 3 itself has no per-code material: its albedo and roughness also read the per-pixel reference colour."""
        if self._stage2 is None:
            raise ValueError('material_rows: no stage-2 model attached (load_stage2 attaches it)')
        return self._stage2.material_rows()

    def materials_at(self, xyz, thres=None, mode='test'):
        """The materials at points xyz [N, 3] alone: those of the stage-2 model whose frozen encoder this one carries
        (vq_nfr.Model.materials_at), as material_rows.  Stage 3's own albedo and roughness also read the per-pixel reference colour,
        which a point of a mesh does not have."""
        if self._stage2 is None:
            raise ValueError('materials_at: no stage-2 model attached (load_stage2 attaches it)')
        return self._stage2.materials_at(xyz, thres=thres, mode=mode)

    def set_light(self, arr):
        """The stage-3 light is a CONSTANT: the reference loads the light stage 2 wrote (`np_light.npy`) into a plain tensor
        (ref_nfr.py:70-87), not a variable -- it gets no gradient and `loss_kwargs['env']` is None (:263, `self._light`)."""
        super().set_light(arr)
        self._light.requires_grad_(False)

    @property
    def light(self):
        if self._light is None:
            BrdfModel.light.fget(self)                            # `light_path` / `light_init_val` of the config
            self._light.requires_grad_(False)
        return self._light                                        # used as loaded: no clip (ref_nfr.py:87, :424)

    def _frozen_ctx(self, names, x):
        """torch.no_grad() when none of the named nets' parameters (nor the input) wants a gradient, else a null context"""
        import contextlib
        # (device tensors on the HIP backend only: the no-graph path IS the HIP inference kernels; CPU parameters -- the gloo tests -- and the
        #  torch backend keep the framework statement)
        if (torch.is_grad_enabled() and x.is_cuda and self.train_backend == 'hip' and not x.requires_grad
                and not any(p.requires_grad for n in names for p in self.net[n].parameters())):
            return torch.no_grad()
        return contextlib.nullcontext()

    def _stage3_engine(self, ref, z_xyz):
        """The exact-split training engine for rgb_enc -> z_ref -> {diff_out, rough_out}([z_xyz ; z_ref]) (decomp/refl_train.py, zx form), or None
        when this is not a HIP training call, z_xyz wants an adjoint (the encoder is being trained: the interpreted programs take it), or the
        nets are outside the kernels' shapes."""
        import os
        if not (self._train_hip(ref) and not self._fused(ref) and os.environ.get('VQN_REFL_TRAIN', self.REFL_TRAIN_DEFAULT) == 'x3'):
            return None
        if z_xyz.requires_grad or ref.requires_grad or z_xyz.shape[1] != self.z_dim:
            return None
        key = ('stage3', str(ref.device))
        if key not in self._engines:
            from vqnerf_release_amd.decomp.refl_train import ReflStackEngine
            enc, heads = [self.net['rgb_enc']], [self.net['diff_out'], self.net['rough_out']]
            ok = ReflStackEngine.supports(enc, heads, self.z_dim, 3, zx=True)
            self._engines[key] = ReflStackEngine(enc, 0, heads, self.z_dim, ref.device, zx=True) if ok else None
        eng = self._engines[key]
        return eng if (eng is not None and any(p.requires_grad for p in eng.params())) else None

    def _pred_ref_at(self, ref):
        if self._fused(ref):
            if 'ref' not in self._plans:
                b = packing.ChainBuilder('raw', 3)
                net = self.net['rgb_enc']
                b.mlp('rgb_enc', net.widths, net.act, net.skip_at, b.input, out_slot=0, small_last=False)
                self._plans['ref'] = b.build()
            wbuf, desc = self._program_pack('ref', self._plans['ref'], ['rgb_enc'])
            return self._numerics(_C.mlp_chain_fwd(desc, wbuf, ref.detach().float().contiguous(), [self.z_dim])[0], 'Z_ref')
        return self._numerics(self.net['rgb_enc'](ref), 'Z_ref')

    def call(self, batch, mode='train', relight_olat=False, relight_probes=False, save_z=False, opt_scale=None, bias_weight=None):
        self._validate_mode(mode)
        id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal, ref = batch[:10]
        lvis = batch[10] if self.data_type == 'nerf' else None
        mask = None if (self.assume_foreground and mode == 'train') else fg_rows(alpha)       # (see nfr_unit.Model.call)
        n = alpha.shape[0]
        rayo, rgb_m, xyz_m, normal_m, ref_m = take_rows(mask, rayo), take_rows(mask, rgb), take_rows(mask, xyz), take_rows(mask, normal), take_rows(mask, ref)
        lvis_m = self.fg_lvis(lvis, mask, xyz_m)
        # the parts that come FROZEN from stage 2 (load_stage2: encoder, specular head) need no graph: in a training call they run on the
        # inference kernels (one fused chain launch each), not on the training programs with everything kept for a backward
        with self._frozen_ctx(['fine_enc', 'bottleneck'], xyz_m):
            z_xyz = self._pred_bias_at(xyz_m)
        with self._frozen_ctx(['spec_out'], z_xyz):
            ks = self._head('spec_out', z_xyz)
        eng = self._stage3_engine(ref_m, z_xyz) if mode == 'train' else None
        if eng is not None:
            # rgb_enc + the two 512-wide heads on the dedicated exact-split kernels (round 5; the interpreted tile programs before)
            from vqnerf_release_amd.decomp.refl_train import ReflStackZxFunction
            z_ref, d, r = ReflStackZxFunction.apply(eng, ref_m, z_xyz, *eng.params())
            self._numerics(z_ref, 'Z_ref')
            basecolor, rough = self._numerics(self._albedo_affine(d), 'Albedo'), self._numerics(r, 'Roughness')
        else:
            z_bias = torch.cat([z_xyz, self._pred_ref_at(ref_m)], -1)
            basecolor = self._albedo_affine(self._head('diff_out', z_bias))
            rough = self._head('rough_out', z_bias)
        spec, albedo = ks * basecolor, (1 - ks) * basecolor
        if (opt_scale is not None) and (mode == 'test'):
            albedo, spec = albedo * opt_scale, spec * opt_scale
        if self._fused(xyz_m, albedo, spec, rough):
            pr = None
            if relight_probes and len(self.novel_probes) > 0:
                pr = torch.stack([torch.as_tensor(lp, dtype=torch.float32, device=xyz_m.device).reshape(-1, 3)
                                  for lp in self.novel_probes.values()], 0)
            sh = self._shade(xyz_m, normal_m, rayo, lvis_m, [(albedo, spec, rough)], split=(mode != 'train'), probes=pr)
        elif self.train_backend == 'hip' and xyz_m.is_cuda and mode == 'train':
            sh = self._shade_train(xyz_m, normal_m, rayo, lvis_m, [(albedo, spec, rough)])
        else:
            surf2l, surf2c = self._calc_ldir(xyz_m), self._calc_vdir(rayo, xyz_m)
            n_pred = self._normal_correct(normal_m, surf2c)
            brdf, brdf_s, brdf_d = self._eval_brdf_at(surf2l, surf2c, n_pred, albedo, spec, rough)
            r0, _, rp = self._render(brdf, surf2l, n_pred, lvis_m, relight_probes=relight_probes)
            sh = {'rgb': [r0], 'normal': n_pred, 'rgb_probes': rp, 'rgb_diff': None, 'rgb_spec': None}
            if mode != 'train':
                sh['rgb_diff'] = self._render(brdf_d, surf2l, n_pred, lvis_m)[0]
                sh['rgb_spec'] = self._render(brdf_s, surf2l, n_pred, lvis_m)[0]
        rgb_pred, normal_pred = sh['rgb'][0], sh['normal']
        loss_kwargs = {'mode': mode, 'env': None, 'gtc': rgb_m, 'rgb': rgb_pred}
        srgb = (lambda t: imgutil.linear2srgb(t)) if self.data_type == 'nerf' else (lambda t: t)
        pred = {'rgb': scatter_rows(mask, srgb(rgb_pred), n), 'normal': scatter_rows(mask, normal_pred, n),
                'albedo': scatter_rows(mask, albedo, n), 'alpha': pred_alpha, 'spec': scatter_rows(mask, spec, n),
                'rough': scatter_rows(mask, rough, n), 'ks': scatter_rows(mask, ks, n), 'basecolor': scatter_rows(mask, basecolor, n)}
        if mode != 'train':
            pred['rgb_spec'], pred['rgb_diff'] = scatter_rows(mask, sh['rgb_spec'], n), scatter_rows(mask, sh['rgb_diff'], n)
        if relight_probes and sh.get('rgb_probes') is not None:
            pred['rgb_probes'] = scatter_rows(mask, srgb(sh['rgb_probes']), n)
        gt = {'rgb': scatter_rows(mask, rgb_m, n), 'normal': scatter_rows(mask, normal_m, n), 'alpha': alpha}
        to_vis = {'id': id_, 'hw': hw}
        for k, v in pred.items():
            to_vis['pred_' + k] = v
        for k, v in gt.items():
            to_vis['gt_' + k] = v
        return pred, gt, loss_kwargs, to_vis

    def fast_render(self, batch, mode='train', relight_olat=False, relight_probes=False, opt_scale=None, edit_mask=None,
                    edit_material=None, edit_rows=None):
        """ref_nfr.py:303-418 (the `pd_test` / `pd_vq` passes of test.py:216-300): `rgb` from the UNscaled materials under the
        model light, the probe renders from the materials scaled by `opt_scale` -- one shading pass: when both are asked for,
        the scaled set rides as material set 0 (the one the kernel relights) and the unscaled one as set 1.
        edit_rows: a uint8 [n] device mask over all rows (the one vq_nfr's fast_render(edit_select=...) returns), applied as edit_mask
        is, in one launch of csrc/material_edit.hip together with the opt_scale scaling."""
        self._validate_mode(mode)
        kernel_edit = material_edit.check_edit_keywords(edit_mask, edit_material, None, edit_rows, None)
        id_, hw, rayo, rayd, rgb, alpha, pred_alpha, xyz, normal, ref = batch[:10]
        lvis = batch[10] if self.data_type == 'nerf' else None
        mask = fg_rows(alpha)
        n = alpha.shape[0]
        rayo, rgb_m, xyz_m, normal_m, ref_m = take_rows(mask, rayo), take_rows(mask, rgb), take_rows(mask, xyz), take_rows(mask, normal), take_rows(mask, ref)
        lvis_m = self.fg_lvis(lvis, mask, xyz_m)
        if edit_mask is not None:
            edit_mask = (take_rows(mask, edit_mask)[..., 0:1] > 0).to(torch.float32)
        z_xyz = self._pred_bias_at(xyz_m)
        ks = self._head('spec_out', z_xyz)
        z_bias = torch.cat([z_xyz, self._pred_ref_at(ref_m)], -1)
        basecolor = self._albedo_affine(self._head('diff_out', z_bias))
        rough = self._head('rough_out', z_bias)
        spec, albedo = ks * basecolor, (1 - ks) * basecolor
        if edit_mask is not None:
            upd = lambda src, v: src * (1 - edit_mask) + edit_mask * torch.as_tensor([v], dtype=torch.float32, device=src.device)
            if not edit_material['diff'][0] < 0:
                albedo = upd(albedo, edit_material['diff'])
            if not edit_material['spec'][0] < 0:
                spec = upd(spec, edit_material['spec'])
            if not edit_material['rough'][0] < 0:
                rough = upd(rough, edit_material['rough'])
        maps = list(self.novel_probes.values()) if relight_probes else []
        if kernel_edit:
            _, albedo, spec, rough, s_albedo, s_spec = material_edit.edit_rows_of_a_view(
                mask, albedo, spec, rough, None, None, edit_material, None, edit_rows, None, opt_scale if (opt_scale is not None and maps) else None)
        sets = [(albedo, spec, rough)]
        if opt_scale is not None and maps:
            sets = [(s_albedo, s_spec, rough) if kernel_edit else (albedo * opt_scale, spec * opt_scale, rough), (albedo, spec, rough)]
        if self._fused(xyz_m, albedo, spec, rough):
            pr = torch.stack([torch.as_tensor(lp, dtype=torch.float32, device=xyz_m.device).reshape(-1, 3) for lp in maps], 0) if maps else None
            sh = self._shade(xyz_m, normal_m, rayo, lvis_m, sets, probes=pr)
        else:
            surf2l, surf2c = self._calc_ldir(xyz_m), self._calc_vdir(rayo, xyz_m)
            n_pred = self._normal_correct(normal_m, surf2c)
            sh = {'rgb': [], 'rgb_probes': None}
            for i, (a, s_, r) in enumerate(sets):
                brdf, _, _ = self._eval_brdf_at(surf2l, surf2c, n_pred, a, s_, r)
                r0, _, rp = self._render(brdf, surf2l, n_pred, lvis_m, relight_probes=(maps if (maps and i == 0) else False))
                sh['rgb'].append(r0)
                if i == 0:
                    sh['rgb_probes'] = rp
        rgb_pred = sh['rgb'][-1]
        loss_kwargs = {'mode': mode, 'env': None, 'gtc': rgb_m, 'rgb': rgb_pred}
        srgb = (lambda t: imgutil.linear2srgb(t)) if self.data_type == 'nerf' else (lambda t: t)
        pred = {'rgb': scatter_rows(mask, srgb(rgb_pred), n), 'alpha': pred_alpha}
        if maps and sh.get('rgb_probes') is not None:
            pred['rgb_probes'] = scatter_rows(mask, srgb(sh['rgb_probes']), n)
        gt = {'rgb': scatter_rows(mask, rgb_m, n), 'normal': scatter_rows(mask, normal_m, n), 'alpha': alpha}
        to_vis = {'id': id_, 'hw': hw}
        for k, v in pred.items():
            to_vis['pred_' + k] = v
        for k, v in gt.items():
            to_vis['gt_' + k] = v
        return pred, gt, loss_kwargs, to_vis

    def compute_loss(self, pred, gt, **kwargs):
        mode = kwargs.pop('mode')
        rgb_gt, rgb_pred = kwargs.pop('gtc'), kwargs.pop('rgb')
        linear_gt = imgutil.srgb2linear(rgb_gt) if self.data_type == 'nerf' else rgb_gt
        loss = ((linear_gt - rgb_pred) ** 2).mean(-1)
        if mode != 'train':
            return loss                                     # ref_nfr.py:606 returns the bare tensor in vali mode
        return self._numerics(loss, 'Loss'), {'rgb': loss, 'loss': loss}
