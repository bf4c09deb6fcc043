"""Training passes of the fused NeuS networks as tile programs for csrc/tile_vm.hip (+ csrc/wgrad.hip).

The reference gets these from autograd: `loss.backward()` through SDFNetwork / RenderingNetwork
(geo/NeuS-ours2/models/fields.py:72-107,147-172), with `create_graph=True` in SDFNetwork.gradient (fields.py:100-106)
so that the eikonal term and the normal-dependent colour differentiate through d sdf / dx.  Here, per 32-point tile:

  forward   e = posenc(x);  u_{l+1} = softplus(W_l in_l + b_l)   (in_l = u_l, or [u_l ; e]/sqrt2 at the skip layer)
            out = W_L u_L + b_L = [sdf ; feat]
            reverse sweep  g^_l = (W_{l+1}^T g^_{l+1}) * softplus'(a_l)  ->  n = J_posenc^T e_bar          (= d sdf / dx)
            colour net on [x, posenc(view), n, feat]
  backward  colour reverse sweep -> d/d feat, d/d n;   v = d loss / d n (compositing + eikonal + colour)
            tangent pass along v:  u'_{l+1} = softplus'(a_l) * (W_l in'_l),  source S_l = g^_l * (W_l in'_l) * softplus''/softplus'
            reverse sweep          a_bar_l = (W_{l+1}^T a_bar_{l+1}) * softplus'(a_l) + S_l
  weights   dW_l = a_bar_l (x) in_l + g^_l (x) in'_l   (contractions over points: csrc/wgrad.hip),  db_l = sum a_bar_l
(the adjoint of the tangent stream IS the forward's reverse sweep, which is why g^_l is saved rather than recomputed).
"""
import os
import math

import numpy as np
import torch

from vqnerf_release_amd import _C
from vqnerf_release_amd.geo import packing
from vqnerf_release_amd.geo.packing import FlatLayout, GatherPack
from vqnerf_release_amd.tile_program import (Program, _f2i, _shift, build_static_packs, K_LD_POSENC, K_LD_POSENC_JVP, K_LD_T, K_LD_VEC,
                                             K_LD_EXTRAS, K_ST_VEC, K_POSENC_VJP, EPI_MUL_DACT, EPI_TANGENT, EPI_BWD2, ACT_NONE, ACT_RELU,
                                             ACT_SOFTPLUS, ACT_SIGMOID)
from vqnerf_release_amd.wgrad import wgrad_mode, wgrad_executor          # (wgrad_mode: also reached as train_programs.wgrad_mode)
# Not used here: the names that tests written against this module's earlier layout take from it (the same objects as in their homes)
from vqnerf_release_amd.tile_program import K_GEMM, DESC_INTS                          # noqa: F401
from vqnerf_release_amd.wgrad import WGRAD_ENTRY, BATCHED_WGRAD, WgradBatch            # noqa: F401

# forward of the full-size training engine: 'x3' = the exact-split render kernel (bf16 piece triples, products to 2^-24: f32-level
# saved tensors, 6.4 ms per 2560-ray step), 'fused' = the f32-input MFMA one (8.1 ms), 'prog' = the interpreted program (9.3 ms);
# VQN_TRAIN_FWD overrides.  x3 is the default since every training test -- the reference's gradient goldens at the unchanged 5e-3 bound,
# the torch-autograd comparisons, the graph replays -- passes under it (the gate VERDICT r02 set for the bf16x3 contraction).
TRAIN_FWD_DEFAULT = 'x3'
TRAIN_COARSE_DEFAULT = 'x3'       # the no-grad up-sampling SDF passes of a training render: 'x3' (the step's x3 packs) | 'f32'; VQN_TRAIN_COARSE
TRAIN_BWD_DEFAULT = 'x3'          # the backward likewise: 'x3' 6.8 ms, 'fused' (f32-input MFMA) 8.6 ms, 'prog' 9.8 ms; same gate, same result


class NeusTrainEngine:
    """Programs, packs and launches for one (SDFNetwork, RenderingNetwork) pair."""

    def __init__(self, sdf_net, col_net, n_split=256):
        self.sdf_net, self.col_net = sdf_net, col_net
        d = sdf_net.dims
        self.nL = len(d) - 2                                   # hidden layers 0..nL-1, final layer nL
        skips = [l for l in sdf_net.skip_in if 0 < l < self.nL + 1]
        assert len(skips) <= 1 and sdf_net.d_in == 3 and sdf_net.multires > 0
        self.skip = skips[0] if skips else -1
        self.E = d[0]
        self.mr = sdf_net.multires
        self.scale = float(sdf_net.scale)
        self.out = [(d[l + 1] - d[0] if (l + 1) == self.skip else d[l + 1]) for l in range(self.nL + 1)]
        self.inn = [d[l] for l in range(self.nL + 1)]
        assert self.skip != self.nL, 'skip into the last layer is not supported'
        self.F = self.out[self.nL]                             # 257 = sdf + features
        c = col_net
        assert c.mode == 'idr' and c.multires_view > 0 and c.dims[-1] == 3
        self.nC = len(c.dims) - 2                              # colour hidden layers 0..nC-1, final nC
        self.mrv = c.multires_view
        self.X = 3 + (3 + 6 * self.mrv) + 3                    # extras: pts, posenc(view), normals
        assert c.dims[0] == self.X + (self.F - 1)
        self.cout = [c.dims[l + 1] for l in range(self.nC + 1)]
        self.cin = [c.dims[l] for l in range(self.nC + 1)]
        self.squeeze = bool(c.squeeze_out)
        self._flat_layout = self._layout()       # the ONE layout of the flat source vector: flat_weights() and every gather index into it
        self.n_split = int(os.environ.get('VQN_GEO_WGRAD_SPLIT', n_split))      # partial blocks of the contractions over the point tiles
        self._fused_dev = {}           # per device: gather indices + descriptors of the fused forward's packs
        self._bwd_dev = {}             # per device: gather index + descriptor of the fused backward's pack
        self._x3_pack = None           # library-built packs of the exact-split forward (vqn_neus_pack_create, engine 2)
        self._bwd_x3_dev = {}          # per device: gather indices + descriptor of the exact-split backward's packs
        self._x3_prepared = None       # prepare_step() packed these weights already (their key)
        for name, build in (('prog_fwd', self._build_forward), ('prog_cbwd', self._build_colour_backward),
                            ('prog_sbwd', self._build_sdf_backward)):
            prog = build()
            assert prog.total_rows * 1024 <= 160 * 1024, f'{name}: {prog.total_rows} KB of LDS'
            setattr(self, name, prog.materialize())
        self._dev = {}

    # tensor tables -------------------------------------------------------------------------------
    def _tiles(self, f):
        return (f + 31) // 32

    def _tensor_specs(self):
        """name -> ('vec', width) | ('t', feature tiles)"""
        s = {'X': ('vec', 3), 'DIRS': ('vec', 3), 'ONES': ('vec', 1), 'SDF': ('vec', 1), 'N': ('vec', 3), 'RGB': ('vec', 3),
             'DOUT': ('vec', 3), 'GNCOL': ('vec', 3), 'V': ('vec', 3), 'GS': ('vec', 1),
             'E': ('t', self._tiles(self.E)), 'ED': ('t', self._tiles(self.E)), 'OUTF': ('t', self._tiles(self.F)),
             'GOUTF': ('t', self._tiles(self.F)), 'EXTR': ('t', self._tiles(self.X)), 'DC%d' % self.nC: ('t', 1)}
        for l in range(self.nL):
            for nm in ('U%d' % (l + 1), 'UD%d' % (l + 1), 'GH%d' % l, 'S%d' % l, 'AB%d' % l):
                s[nm] = ('t', self._tiles(self.out[l]))
        for l in range(self.nC):
            s['C%d' % (l + 1)] = ('t', self._tiles(self.cout[l]))
            s['DC%d' % l] = ('t', self._tiles(self.cout[l]))
        return s

    # the tensor lists of the fused kernels (vqn_neus_train_fwd[_x3], vqn_neus_train_bwd[_x3]): their order is the kernels' ABI
    def _saved_forward(self, T):
        return [T['E'], T['OUTF'], T['EXTR']] + [T['U%d' % (l + 1)] for l in range(self.nL)] + [T['GH%d' % l] for l in range(self.nL)] \
            + [T['C%d' % (l + 1)] for l in range(self.nC)]

    def _saved_backward(self, T):
        return self._saved_forward(T)[3:]                        # the forward's list without E, OUTF, EXTR

    def _outs_backward(self, T):
        return [T['DC%d' % l] for l in range(self.nC + 1)] + [T['GOUTF'], T['ED']] + [T['UD%d' % (l + 1)] for l in range(self.nL)] \
            + [T['AB%d' % l] for l in range(self.nL)]

    # programs --------------------------------------------------------------------------------------
    def _names(self):
        return list(self._tensor_specs().keys())

    def _sdf_fwd_cols(self, l, prev, emb):
        """column maps of W_l for K = [prev (, emb at the skip layer)]"""
        if l == 0:
            return [emb], [(self.E, 0)]
        if l == self.skip:
            return [prev, emb], [(self.out[l - 1], 0), (self.E, self.out[l - 1])]
        return [prev], [(self.inn[l], 0)]

    def _build_forward(self):
        P = Program(self._names())
        nL, nC = self.nL, self.nC
        rE = P.alloc(self.E, [])
        P.op(K_LD_POSENC, P.t('X'), P.row(rE), self.mr, self.E, P.t('E'), _f2i(self.scale))
        prev = None
        for l in range(nL):
            segs, cols = self._sdf_fwd_cols(l, prev, rE)
            prev = P.gemm(('W', l), (self.out[l], self.inn[l]), segs, cols, self.out[l], live=[rE], act=ACT_SOFTPLUS,
                          bias_key=('b', l), store='U%d' % (l + 1))
        rU = prev
        rOUT = P.gemm(('W', nL), (self.F, self.inn[nL]), [rU], [(self.inn[nL], 0)], self.F, live=[], bias_key=('b', nL), store='OUTF')
        P.op(K_ST_VEC, P.row(rOUT), 0, 1, P.t('SDF'), ACT_NONE, _f2i(1.0 / self.scale))
        # reverse sweep for n = d sdf / dx.  rOUT is NOT kept in LDS meanwhile (it is re-read from OUTF for the colour net):
        # that keeps the program under 80 KB, i.e. two workgroups per CU.
        rONE = P.alloc(1, [])
        P.op(K_LD_VEC, P.t('ONES'), P.row(rONE), 1, _f2i(1.0), -1, 0)
        g = P.gemm(('WT_sdfrow',), (self.out[nL - 1], 1), [rONE], [(1, 0)], self.out[nL - 1], live=[],
                   epi=EPI_MUL_DACT, act=ACT_SOFTPLUS, aux1='U%d' % nL, store='GH%d' % (nL - 1))
        rEB, have_eb = None, False
        for l in range(nL - 1, 0, -1):
            # adjoint of in_l = W_l^T g^_l ; its u-part times softplus'(a_{l-1}) is g^_{l-1}
            if l == self.skip:
                rEB = P.gemm(('WT_e', l), (self.E, self.out[l]), [g], [(self.out[l], 0)], self.E, live=[g])
                have_eb = True
            keep = [g] + ([rEB] if have_eb else [])
            g = P.gemm(('WT_u', l), (self.out[l - 1], self.out[l]), [g], [(self.out[l], 0)], self.out[l - 1], live=keep,
                       epi=EPI_MUL_DACT, act=ACT_SOFTPLUS, aux1='U%d' % l, store='GH%d' % (l - 1))
        if have_eb:
            P.gemm(('WT_e', 0), (self.E, self.out[0]), [g], [(self.out[0], 0)], self.E, live=[], dst=rEB, accumulate=True)
        else:
            rEB = P.gemm(('WT_e', 0), (self.E, self.out[0]), [g], [(self.out[0], 0)], self.E, live=[g])
        P.op(K_POSENC_VJP, P.row(rEB), P.t('X'), P.t('N'), self.mr, _f2i(self.scale))
        # colour network on [pts, posenc(view), normals, feat]
        rOUT = P.alloc(self.F, [], tiles=self._tiles(self.F))
        P.op(K_LD_T, P.t('OUTF'), P.row(rOUT), rOUT.rows)
        rEX = P.alloc(self.X, [rOUT])
        P.op(K_LD_EXTRAS, P.t('X'), P.t('DIRS'), P.t('N'), P.row(rEX), self.mrv, P.t('EXTR'), self.X)
        prev = P.gemm(('Wc', 0), (self.cout[0], self.cin[0]), [rOUT, rEX], [_shift(1, self.F, self.X), (self.X, 0)], self.cout[0],
                      live=[], act=ACT_RELU, bias_key=('bc', 0), store='C1')
        for l in range(1, nC):
            prev = P.gemm(('Wc', l), (self.cout[l], self.cin[l]), [prev], [(self.cin[l], 0)], self.cout[l], live=[], act=ACT_RELU,
                          bias_key=('bc', l), store='C%d' % (l + 1))
        rRGB = P.gemm(('Wc', nC), (3, self.cin[nC]), [prev], [(self.cin[nC], 0)], 3, live=[],
                      act=ACT_SIGMOID if self.squeeze else ACT_NONE, bias_key=('bc', nC))
        P.op(K_ST_VEC, P.row(rRGB), 0, 3, P.t('RGB'), ACT_NONE, _f2i(1.0))
        return P.finalize()

    def _build_colour_backward(self):
        P = Program(self._names())
        nC = self.nC
        rD = P.alloc(3, [], tiles=1)
        P.op(K_LD_VEC, P.t('DOUT'), P.row(rD), 3, _f2i(1.0), P.t('DC%d' % nC), 0)
        for l in range(nC, 0, -1):                            # delta_{l-1} = (Wc_l^T delta_l) * relu'(c_l)
            rD = P.gemm(('WcT', l), (self.cin[l], self.cout[l]), [rD], [(self.cout[l], 0)], self.cin[l], live=[],
                        epi=EPI_MUL_DACT, act=ACT_RELU, aux1='C%d' % l, store='DC%d' % (l - 1))
        # adjoints of the colour-net inputs: [sdf(=0) ; feat] in OUTF feature order, and the extras (normals at X-3..X-1)
        P.gemm(('WcT0_feat',), (self.F, self.cout[0]), [rD], [(self.cout[0], 0)], self.F, live=[rD], store='GOUTF', want_dst=False)
        rGX = P.gemm(('WcT0_extra',), (self.X, self.cout[0]), [rD], [(self.cout[0], 0)], self.X, live=[rD])
        P.op(K_ST_VEC, P.row(rGX), self.X - 3, 3, P.t('GNCOL'), ACT_NONE, _f2i(1.0))
        return P.finalize()

    def _build_sdf_backward(self):
        P = Program(self._names())
        nL = self.nL
        rED = P.alloc(self.E, [])
        P.op(K_LD_POSENC_JVP, P.t('X'), P.t('V'), P.row(rED), self.mr, self.E, P.t('ED'), _f2i(self.scale))
        prev = None
        for l in range(nL):                                   # tangent pass (no bias)
            segs, cols = self._sdf_fwd_cols(l, prev, rED)
            prev = P.gemm(('W', l), (self.out[l], self.inn[l]), segs, cols, self.out[l], live=[rED], epi=EPI_TANGENT, act=ACT_SOFTPLUS,
                          aux1='U%d' % (l + 1), aux2='GH%d' % l, store='UD%d' % (l + 1), store2='S%d' % l)
        # adjoint of u_L from the final layer: W_L[1:]^T g_feat + W_L[0]^T g_sdf / scale
        rGO = P.alloc(self.F, [])
        P.op(K_LD_T, P.t('GOUTF'), P.row(rGO), rGO.rows)
        rGS = P.alloc(1, [rGO])
        P.op(K_LD_VEC, P.t('GS'), P.row(rGS), 1, _f2i(1.0 / self.scale), -1, 0)
        ab = P.gemm(('WT_last',), (self.out[nL - 1], self.F), [rGO, rGS], [_shift(1, self.F, 1), (1, 0)], self.out[nL - 1], live=[],
                    epi=EPI_BWD2, act=ACT_SOFTPLUS, aux1='U%d' % nL, aux2='S%d' % (nL - 1), store='AB%d' % (nL - 1))
        for l in range(nL - 1, 0, -1):
            ab = P.gemm(('WT_u', l), (self.out[l - 1], self.out[l]), [ab], [(self.out[l], 0)], self.out[l - 1], live=[],
                        epi=EPI_BWD2, act=ACT_SOFTPLUS, aux1='U%d' % l, aux2='S%d' % (l - 1), store='AB%d' % (l - 1))
        return P.finalize()

    # packs -----------------------------------------------------------------------------------------
    def _layout(self):
        shapes = [('W%d' % l, (self.out[l], self.inn[l])) for l in range(self.nL + 1)] + \
                 [('b%d' % l, (self.out[l],)) for l in range(self.nL + 1)] + \
                 [('Wc%d' % l, (self.cout[l], self.cin[l])) for l in range(self.nC + 1)] + \
                 [('bc%d' % l, (self.cout[l],)) for l in range(self.nC + 1)]
        return FlatLayout(shapes)

    def _matrix_index(self, key, L):
        """positions (in the flat source vector) of the [rows, cols] matrix a gather key refers to.  The skip layer's 1/sqrt2
        (fields.py:82) is applied to its source W before flattening (see flat_weights)."""
        kind = key[0]
        if kind in ('W', 'b', 'Wc', 'bc'):
            return L[kind + '%d' % key[1]]
        if kind == 'WT_sdfrow':
            return L['W%d' % self.nL][:1].T
        if kind == 'WT_u':                                     # rows = features of u_l (the part of in_l that is u_l)
            l = key[1]
            return L['W%d' % l][:, :self.out[l - 1]].T
        if kind == 'WT_e':
            l = key[1]
            return (L['W%d' % l][:, self.out[l - 1]:] if l == self.skip and l > 0 else L['W%d' % l]).T
        if kind == 'WT_last':
            return L['W%d' % self.nL].T
        if kind == 'WcT':
            return L['Wc%d' % key[1]].T
        if kind == 'WcT0_feat':                                 # rows in OUTF order: [0 (sdf) ; feat]
            M = L['Wc0'][:, self.X:].T
            return np.concatenate([np.full((1, M.shape[1]), L.zero, np.int64), M], 0)
        if kind == 'WcT0_extra':
            return L['Wc0'][:, :self.X].T
        raise KeyError(key)

    def _static(self, device):
        """weight-independent part of the packs: one global gather index + the three descriptors (cached per device)."""
        k = str(device)
        if k not in self._dev:
            L = self._flat_layout
            progs = {n: getattr(self, n) for n in ('prog_fwd', 'prog_cbwd', 'prog_sbwd')}
            gidx, descs = build_static_packs(progs, L, lambda key: self._matrix_index(key, L))
            self._dev[k] = (L, torch.from_numpy(gidx).to(device), {n: (d, torch.from_numpy(d).to(device)) for n, d in descs.items()})
        return self._dev[k]

    def flat_weights(self, W, b, Wc, bc):
        """effective weights -> the flat source vector every pack of a step is ONE gather from (the skip layer's 1/sqrt2 applied)."""
        src = {}
        for l in range(self.nL + 1):
            src['W%d' % l] = W[l] * (1.0 / math.sqrt(2.0)) if l == self.skip else W[l]
            src['b%d' % l] = b[l]
        for l in range(self.nC + 1):
            src['Wc%d' % l], src['bc%d' % l] = Wc[l], bc[l]
        return self._flat_layout.flatten(src)

    def pack(self, W, b, Wc, bc, want_flat=False):
        """flat_weights() + program_pack() in one call (+ the flat source vector): the form tests of earlier commits call"""
        flat = self.flat_weights(W, b, Wc, bc)
        return self.program_pack(flat) + ((flat,) if want_flat else ())

    def program_pack(self, flat):
        """flat_weights() -> the interpreted programs' weight buffer (ONE gather) + their cached descriptors."""
        _, gidx, descs = self._static(flat.device)
        return flat[gidx], descs

    # launches --------------------------------------------------------------------------------------
    def _scratch_names(self):
        """Temporaries of ONE program (the tangent pass's second-order sources, consumed by the reverse sweep of the same prog_sbwd
        program for the same tile): per-workgroup images that stay cache-resident (vqn_tile_program_grid, negative ld)."""
        return {'S%d' % l for l in range(self.nL)}

    def alloc_tensors(self, P, device):
        """every tensor of a step, the interpreter's own (ONES, DOUT, GNCOL, V, GS, the S scratch images) included even when both passes run fused"""
        nt = (P + 31) // 32
        scratch, n_wg = self._scratch_names(), nt
        if scratch:
            n_wg = _C.tile_program_grid(self._static(device)[2]['prog_sbwd'][0], P)
        out = {}
        for name, (kind, w) in self._tensor_specs().items():
            out[name] = torch.empty((P, w), dtype=torch.float32, device=device) if kind == 'vec' \
                else torch.empty((n_wg if name in scratch else nt, w, 32, 32), dtype=torch.float32, device=device)
        out['ONES'].fill_(1.0)
        return out

    def run(self, which, descs, wbuf, tensors, P):
        prog = getattr(self, which)
        d_host, d_dev = descs[which]
        names = list(prog.tn.keys())
        specs, scratch = self._tensor_specs(), self._scratch_names()
        _C.tile_program(which, d_dev, d_host, wbuf, [tensors[n] for n in names], [-specs[n][1] if n in scratch else specs[n][1] for n in names], P)

    # the forward on the render kernel ---------------------------------------------------------------
    def fused_forward(self):
        """Run the forward as ONE launch of the two-image render kernel (csrc/neus_mlp.hip, vqn_neus_train_fwd) instead of the
        interpreted prog_fwd: same saved tensors, the render kernel's summation order.  VQN_TRAIN_FWD=prog selects the interpreter."""
        return self.forward_mode() is not None

    def forward_mode(self):
        """'f32' (vqn_neus_train_fwd) | 'x3' (vqn_neus_train_fwd_x3: the exact-split engine) | None (the interpreted prog_fwd).
        VQN_TRAIN_FWD = fused | x3 | prog; networks of fewer than 5 or more than 8 feature tiles always take the interpreter."""
        want = os.environ.get('VQN_TRAIN_FWD', TRAIN_FWD_DEFAULT)
        if want not in ('fused', 'x3') or os.environ.get('VQN_NEUS_TILE32') is not None:
            return None
        mt = max(self.sdf_net.plan(max_tiles=self.col_net.max_tiles()).max_tiles, self.col_net.max_tiles())
        # 5..8 tiles: the kernels' two-image form (two activation images of 9 tiles are 166 KB of LDS: vqn_neus_train_fwd refuses them)
        if not (5 <= mt <= 8 and self.skip != 0 and self.E <= 64 and self.X <= 64):      # (embedding / extras: at most two feature tiles)
            return None
        return 'x3' if want == 'x3' else 'f32'

    def _x3_handle(self):
        if self._x3_pack is None:
            c, sn = self.col_net, self.sdf_net
            self._x3_pack = _C.NeusPackHandle(list(sn.dims), self.skip, self.mr, self.scale, 0, c.dims[1], c.num_layers - 2, self.mrv,
                                              self.squeeze, 2)
        return self._x3_pack

    def prepare_step(self, s_lins, c_lins):
        """Start of a training render whose forward runs on the exact-split engine: the library-built x3 packs from the current
        weights (one weight-norm launch, one gather + split launch per network), made BEFORE the no-grad up-sampling passes so that
        those read them too (the exact-split SDF kernel, 1.5 x the f32-input one) instead of packing the f32 SDF net chunk by chunk;
        the forward of the same step then skips its own update.  Returns the pack handle, or None when this does not apply."""
        if self.forward_mode() != 'x3' or os.environ.get('VQN_TRAIN_COARSE', TRAIN_COARSE_DEFAULT) != 'x3':
            return None
        from vqnerf_release_amd.geo.models.fields import effective_weights
        with torch.no_grad():
            ws = [w.float().contiguous() for w in effective_weights(list(s_lins) + list(c_lins))]
            n = len(s_lins)
            h = self._x3_handle()
            h.update(ws[:n], [m.bias.detach().float().contiguous() for m in s_lins], ws[n:], [m.bias.detach().float().contiguous() for m in c_lins])
        self._x3_prepared = self._weights_key()
        return h

    def _weights_key(self):
        """what the x3 packs were built from: the process-wide weights epoch (optimiser steps, graph replays) + every parameter's version"""
        import vqnerf_release_amd
        return vqnerf_release_amd.WeightsStamp([p for m in (self.sdf_net, self.col_net) for p in m.parameters()],
                                               (vqnerf_release_amd.weights_epoch(),))

    def run_fused_forward_x3(self, W, b, Wc, bc, T, P):
        """the forward on the exact-split engine: packs by the library's own builder (one gather + split launch per network)"""
        if self._x3_prepared is not None and self._x3_prepared == self._weights_key():      # packed at the start of this render: same weights
            self._x3_prepared = None
        else:
            self._x3_prepared = None
            cont = lambda ts: [t if t.is_contiguous() else t.contiguous() for t in ts]
            self._x3_handle().update(cont(W), cont(b), cont(Wc), cont(bc))
        _C.neus_train_fwd(None, None, None, None, T['X'], T['DIRS'], self._saved_forward(T), self._tiles(self.E), self._tiles(self.F),
                          self._tiles(self.X), T['SDF'], T['N'], T['RGB'], pack=self._x3_pack)

    def _fused_static(self, device):
        """Gather indices of the render kernel's two packs INTO THE FLAT SOURCE VECTOR of flat_weights() (so the forward's packs cost one
        gather each per step) and their descriptors: the plans' own gathers composed with the flat vector's views.  The flat
        vector already holds the skip layer divided by sqrt2, as SdfPackPlan.pack() gathers it."""
        k = str(device)
        if k not in self._fused_dev:
            L = self._flat_layout
            views = lambda name, n: [L[name + '%d' % l] for l in range(n)]
            plan = self.sdf_net.plan(max_tiles=self.col_net.max_tiles())
            c = self.col_net
            col_plan = packing.ColPackPlan(c.d_feature, c.mode, c.dims[1], c.num_layers - 2, c.dims[-1], c.multires_view, c.squeeze_out,
                                           plan.tiles[-1])
            gi_s = plan.gather_index(L, views('W', self.nL + 1), views('b', self.nL + 1))
            gi_c = col_plan.gather_index(L, views('Wc', self.nC + 1), views('bc', self.nC + 1))
            self._fused_dev[k] = (torch.from_numpy(gi_s).to(device), plan.desc.copy(), torch.from_numpy(gi_c).to(device), col_plan.desc.copy())
        return self._fused_dev[k]

    def run_fused_forward(self, flat, T, P):
        """flat: the flat source vector of flat_weights()."""
        gi_s, d_s, gi_c, d_c = self._fused_static(flat.device)
        _C.neus_train_fwd(d_s, flat[gi_s], d_c, flat[gi_c], T['X'], T['DIRS'], self._saved_forward(T), self._tiles(self.E),
                          self._tiles(self.F), self._tiles(self.X), T['SDF'], T['N'], T['RGB'])

    # the backward on the two-image engine ---------------------------------------------------------------
    TB_MAX_L = 12

    def backward_mode(self):
        """'x3' (vqn_neus_train_bwd_x3, layers of at most 256 outputs) | 'f32' (vqn_neus_train_bwd) | None (the interpreted programs).
        VQN_TRAIN_BWD = x3 | fused | prog."""
        want = os.environ.get('VQN_TRAIN_BWD', TRAIN_BWD_DEFAULT)
        if want not in ('fused', 'x3') or not self._fused_backward_shape():
            return None
        return 'x3' if want == 'x3' else 'f32'

    def fused_backward(self):
        return self.backward_mode() is not None

    def run_fused_backward_x3(self, flat, T, P, g_rgb, g_n, g_sdf):
        gidx, n_steps, fidx, desc = self._bwd_static(flat.device, 'x3')
        pieces, wf = _C.pack_x3_gather(flat, gidx, n_steps, fidx)
        _C.neus_train_bwd_x3(desc, pieces, wf, T['X'], g_rgb, T['RGB'] if self.squeeze else None, g_n,
                             g_sdf, self._saved_backward(T), self._outs_backward(T))

    def _fused_backward_shape(self):
        """Run colour backward + SDF backward as ONE launch of csrc/neus_train_bwd.hip (vqn_neus_train_bwd) instead of the
        interpreted prog_cbwd / prog_sbwd (VQN_TRAIN_BWD=prog selects those).  Same tensors out, the kernel's summation order."""
        if os.environ.get('VQN_NEUS_TILE32') is not None:
            return False
        mt = max(self._tiles(w) for w in self.out[:self.nL] + self.cout[:self.nC] + [self.F - 1])
        return 5 <= mt <= 8 and self.skip != 0 and self.nL >= 2 and self.nC >= 1 and max(self.nL, self.nC) < self.TB_MAX_L and self.E <= 64 and self.X <= 64

    def _bwd_static(self, device, mode='f32'):
        """The backward kernel's weight packs as gathers from the flat source vector of flat_weights(), and its int32 descriptor (TrainBwdDesc),
        in the layout of the engine `mode`.  Matrices in A-fragment order, the thin ones as f32 images.
        'f32' (csrc/neus_train_bwd.hip): ONE buffer -> (int64 gather index, descriptor).
        'x3' (csrc/neus_train_bwd_x3.hip): the matrices form a piece pack (vqn_pack_x3_gather splits what it gathers), the thin
        images an f32 buffer of their own -> (int32 index [steps, 64, 8] of the piece pack, its K steps, int32 index of the images,
        descriptor)."""
        cache, k = (self._bwd_x3_dev if mode == 'x3' else self._bwd_dev), str(device)
        if k in cache:
            return cache[k]
        lay, x3 = packing.LAYOUTS[mode], mode == 'x3'
        L, nL, nC, M = self._flat_layout, self.nL, self.nC, self.TB_MAX_L
        tl = self._tiles
        emb_rows = lay.rows_for(self.E)
        mats = GatherPack(L, pieces=x3)
        thin = GatherPack(L) if x3 else mats

        def gemm(view, n_out, n_cols, segs=None):
            return mats.add(view, lay.gemm_index(n_out, n_cols, segs))

        offT, offB, offCB = [0] * M, [0] * M, [0] * M
        for l in range(nL):                                   # W_l over K = [u_{l-1} (, e at the skip layer)] (the 1/sqrt2 is in the flat vector)
            if l == 0:
                segs = [(emb_rows, self.E, 0)]
            elif l == self.skip:
                prev = self.out[l - 1]
                segs = [lay.tile_seg(prev), (emb_rows, self.E, prev)]
            else:
                segs = None
            offT[l] = gemm(L['W%d' % l], self.out[l], self.inn[l], segs)
        for l in range(1, nL):                                # W_l[:, :out_{l-1}]^T
            offB[l] = gemm(L['W%d' % l][:, :self.out[l - 1]].T, self.out[l - 1], self.out[l])
        nf, n_last = self.F - 1, self.inn[nL]
        offBtop = gemm(L['W%d' % nL][1:].T, n_last, nf)
        if x3:                                                # the sdf row of W_L: the x3 kernel reads it in accumulator (bias) order,
            offWrow = thin.add(L['W%d' % nL][0], lay.bias_index(n_last))
        else:                                                 # the f32 kernel as a row-dot image
            offWrow = thin.add(L['W%d' % nL][:1], lay.rowdot_index(1, n_last))
        for l in range(1, nC + 1):                            # Wc_l^T; l = nC: its three columns are ONE K step (1 row for f32, 3 for x3)
            segs = [(lay.rows_per_step, self.cout[l], 0)] if l == nC else None
            offCB[l] = gemm(L['Wc%d' % l].T, self.cin[l], self.cout[l], segs)
        offCBfeat = gemm(L['Wc0'][:, self.X:].T, nf, self.cout[0])
        offCBnrm = thin.add(L['Wc0'][:, self.X - 3:self.X].T, lay.rowdot_index(3, self.cout[0]))
        mt = max(tl(w) for w in self.out[:nL] + self.cout[:nC] + [nf])
        desc = np.zeros(16 + 5 * M, np.int32)
        desc[0:14] = [nL, nC, self.skip, emb_rows, self.E, tl(self.E), mt, tl(nf), tl(self.F), int(self.squeeze), offBtop, offWrow, offCBfeat,
                      offCBnrm]
        desc[14] = np.float32(self.scale).view(np.int32)
        desc[15] = np.float32(1.0 / self.scale).view(np.int32)
        for l in range(nL):
            desc[16 + l] = tl(self.out[l])
        for l in range(nC):
            desc[16 + M + l] = tl(self.cout[l])
        desc[16 + 2 * M:16 + 3 * M] = offT
        desc[16 + 3 * M:16 + 4 * M] = offB
        desc[16 + 4 * M:16 + 5 * M] = offCB
        gidx = mats.index()
        if x3:
            assert gidx.size % 512 == 0 and gidx.max() < 2 ** 31
            cache[k] = (torch.from_numpy(gidx.astype(np.int32)).to(device), gidx.size // 512,
                        torch.from_numpy(thin.index().astype(np.int32)).to(device), desc)
        else:
            cache[k] = (torch.from_numpy(gidx).to(device), desc)
        return cache[k]

    def run_fused_backward(self, flat, T, P, g_rgb, g_n, g_sdf):
        """g_rgb [P,3] (adjoint of the colours AFTER the sigmoid when the colour net has one), g_n [P,3] | None, g_sdf [P] | None."""
        gidx, desc = self._bwd_static(flat.device)
        _C.neus_train_bwd(desc, flat[gidx], T['X'], g_rgb, T['RGB'] if self.squeeze else None, g_n, g_sdf, self._saved_backward(T),
                          self._outs_backward(T))

    def weight_grads(self, T, g_sdf, goutf_row0_is_gs=False):
        """gradients w.r.t. the EFFECTIVE weights / biases (dW, db, dWc, dbc), from the saved tensors: every contraction stated once,
        against the executor the process selects (wgrad.py).  goutf_row0_is_gs: the backward kernel left d loss / d sdf / scale in
        row 0 of GOUTF (the fused kernels do, round 4), so the contraction GOUTF x u_L already holds row 0 of the last layer's gradient
        and of its bias -- in torch that row was an elementwise product over u_L (84 M elements at the bench batch) and a sum over it:
        1 GB of traffic per step."""
        nL, nC, s2 = self.nL, self.nC, 1.0 / math.sqrt(2.0)
        uL, udL = T['U%d' % nL], T['UD%d' % nL]
        nt, dev = uL.shape[0], uL.device
        tsum = lambda t, n: t.sum((0, 3)).reshape(-1)[:n]        # sum over points of a TFMT tensor -> [features]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        dW, db = [new(self.out[l], self.inn[l]) for l in range(nL + 1)], [new(self.out[l]) for l in range(nL + 1)]
        dWc, dbc = [new(self.cout[l], self.cin[l]) for l in range(nC + 1)], [new(self.cout[l]) for l in range(nC + 1)]
        ex = wgrad_executor(self.n_split)
        for l in range(nL):          # dW_l = a_bar_l (x) in_l + g^_l (x) in'_l;  in_l = e, u_l, or [u_l ; e] / sqrt2 at the skip layer
            ab, gh, ld, sc = T['AB%d' % l], T['GH%d' % l], self.inn[l], (s2 if l == self.skip else 1.0)
            if l == 0:
                ex.contract(ab, T['E'], self.out[0], self.E, dW[0], ld, 1, bias_dst=db[0], A2=gh, B2=T['ED'])
            else:
                pu = self.out[l - 1]
                ex.contract(ab, T['U%d' % l], self.out[l], pu, dW[l], ld, 1, bias_dst=db[l], A2=gh, B2=T['UD%d' % l], scale=sc)
                if l == self.skip:
                    ex.contract(ab, T['E'], self.out[l], self.E, dW[l][:, pu:], ld, 1, A2=gh, B2=T['ED'], scale=sc)
        # final layer: rows 1.. from the feature adjoints (row 0 of the contraction: fixed up below)
        ex.contract(T['GOUTF'], uL, self.F, self.out[nL - 1], dW[nL], self.inn[nL], 1, bias_dst=db[nL])
        # colour net: layer 0's input is [extras ; features], the features' columns come from OUTF = [sdf ; features] without its row 0
        ex.contract(T['DC0'], T['EXTR'], self.cout[0], self.X, dWc[0], self.cin[0], 1)
        ex.contract(T['DC0'], T['OUTF'], self.cout[0], self.F, dWc[0][:, self.X - 1:], self.cin[0], 1, bias_dst=dbc[0], col_first=1)
        for l in range(1, nC + 1):
            ex.contract(T['DC%d' % l], T['C%d' % l], self.cout[l], self.cin[l], dWc[l], self.cin[l], 1, bias_dst=dbc[l])
        ex.flush()
        # row 0 of the final layer = (g_sdf/scale) (x) u_L + u'_L ; its bias = sum of g_sdf / scale
        if goutf_row0_is_gs:
            dW[nL][0] += tsum(udL, self.out[nL - 1])
        else:
            gs = torch.zeros(nt * 32, dtype=torch.float32, device=dev)
            gs[:g_sdf.numel()] = g_sdf.reshape(-1) / self.scale
            dW[nL][0] = (uL * gs.view(nt, 1, 1, 32)).sum((0, 3)).reshape(-1)[:self.out[nL - 1]] + tsum(udL, self.out[nL - 1])
            db[nL][0] = gs.sum()
        return dW, db, dWc, dbc


class NeusCoreFunction(torch.autograd.Function):
    """(x, dirs, W_0.., b_0.., Wc_0.., bc_0..) -> (sdf [P,1], n [P,3], rgb [P,3]); backward = the fused kernels or the tile programs."""

    @staticmethod
    def forward(ctx, engine, x, dirs, *params):
        nS, nCc = engine.nL + 1, engine.nC + 1
        params = [p.detach().float() for p in params]
        W, b, Wc, bc = params[:nS], params[nS:2 * nS], params[2 * nS:2 * nS + nCc], params[2 * nS + nCc:]
        P = x.shape[0]
        # an output the loss does not touch reaches backward() as None (the kernels take a NULL adjoint), not as a tensor of zeros
        ctx.set_materialize_grads(False)
        with torch.no_grad():
            mode = engine.forward_mode()
            programs = mode is None or engine.backward_mode() is None          # does any pass of this step run interpreted?
            flat = engine.flat_weights(W, b, Wc, bc)
            wbuf, descs = engine.program_pack(flat) if programs else (None, None)
            T = engine.alloc_tensors(P, x.device)
            T['X'].copy_(x)
            T['DIRS'].copy_(dirs)
            if mode == 'x3':
                engine.run_fused_forward_x3(W, b, Wc, bc, T, P)
            elif mode == 'f32':
                engine.run_fused_forward(flat, T, P)
            else:
                engine.run('prog_fwd', descs, wbuf, T, P)
        ctx.engine, ctx.T, ctx.descs, ctx.wbuf, ctx.P, ctx.flat = engine, T, descs, wbuf, P, flat
        return T['SDF'], T['N'], T['RGB']

    @staticmethod
    def backward(ctx, g_sdf, g_n, g_rgb):
        e, T, P = ctx.engine, ctx.T, ctx.P
        with torch.no_grad():
            rgb = T['RGB']
            g_rgb = torch.zeros_like(rgb) if g_rgb is None else g_rgb
            gs = torch.zeros_like(T['SDF']) if g_sdf is None else g_sdf.reshape(-1, 1).contiguous()
            bmode = e.backward_mode()
            assert bmode is not None or ctx.wbuf is not None, 'VQN_TRAIN_BWD changed to the interpreter after a forward that packed no program'
            if bmode is not None:
                run = e.run_fused_backward_x3 if bmode == 'x3' else e.run_fused_backward
                run(ctx.flat, T, P, g_rgb.contiguous().float(), None if g_n is None else g_n.contiguous().float(),
                    None if g_sdf is None else gs.float())
            else:
                T['DOUT'].copy_(g_rgb * rgb * (1.0 - rgb) if e.squeeze else g_rgb)
                e.run('prog_cbwd', ctx.descs, ctx.wbuf, T, P)
                T['V'].copy_(T['GNCOL'] if g_n is None else g_n + T['GNCOL'])
                T['GS'].copy_(gs)
                e.run('prog_sbwd', ctx.descs, ctx.wbuf, T, P)
            dW, db, dWc, dbc = e.weight_grads(T, gs, goutf_row0_is_gs=bmode is not None)
        ctx.T = ctx.flat = None
        return (None, None, None) + tuple(dW) + tuple(db) + tuple(dWc) + tuple(dbc)
