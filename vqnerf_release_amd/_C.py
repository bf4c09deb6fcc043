"""ctypes binding of libvqnerf_hip.so (include/vqnerf_hip.h and the area headers beside it: ABI_BY_HEADER).

There is NO fallback: if the library is missing or a call fails this raises.  Tensors are passed as
raw device pointers (tensor.data_ptr()) plus sizes; work is enqueued on torch's current HIP stream.
This is the package's only door to the library: every entry point is declared in a table of ABI_BY_HEADER and launched through _call.
"""
import contextlib
import ctypes
import os
import re

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VQN_LIB', os.path.join(_HERE, 'lib', 'libvqnerf_hip.so'))     # VQN_LIB: diagnostic builds only
_lib = None

# Every function of include/vqnerf_hip.h as `R name(A...)`, one code per type: p pointer (device or host, None = NULL), i int /
# int32_t, l int64_t, f float, d double, and for returns s const char* and v void.  lib() installs them as restype / argtypes;
# tests/test_abi_headers.py holds every table to its header.
_ABI = """
i vqn_version()  s vqn_last_error()  i vqn_vq_assign(plipipppppp)  i vqn_vq_assign_variant(iiii)  i vqn_vq_ema_stats(ppliippplp)
l vqn_vq_ema_stats_ws_bytes(lii)  i vqn_vq_ste_loss(pplfpppp)  i vqn_vq_ema_update(pppiidfpppppppp)
i vqn_decomp_loss_fwd(ppppppliiffffffpp)  i vqn_decomp_loss_bwd(ppppppliiffffffpppppp)  i vqn_l2_normalize_rows(plifpp)
i vqn_l2_normalize_rows_bwd(pplifpp)  i vqn_vq_ste_loss_bwd(pppplpp)  i vqn_codebook_prep(ppiifpp)  i vqn_sim_smooth_fwd(piifpp)
i vqn_sim_smooth_bwd(pppiifpp)  i vqn_vq_quantize_rows(plipipffpppppp)  i vqn_vq_train_bwd(pppppflifpp)
i vqn_vq_quantize_rows_train(plipipfffppppppp)  i vqn_mlp_chain_fwd(ppplpipipipip)  i vqn_mlp_chain_fwd_f16s(ppplpipipipip)
i vqn_brdf_shade_fwd(pppppppliippppppppppppipipp)  i vqn_brdf_shade_fwd_rows(ppppppppliippppppppppppipipp)
l vqn_brdf_shade_bwd_partials(l)  i vqn_brdf_shade_bwd(pppppppliipppppppppppppppp)  i vqn_neus_sdf_points(pppppplipp)
l vqn_neus_fine_scratch_bytes(p)  i vqn_neus_fine_points(pppppppppliplpppp)  i vqn_neus_train_fwd(pppppplplpiiiipppp)
l vqn_neus_train_bwd_scratch_bytes(p)  i vqn_neus_train_bwd(ppppppplplpipip)  l vqn_neus_train_bwd_x3_scratch_bytes(p)
i vqn_neus_train_bwd_x3(pppppppplplpipip)  i vqn_pack_x3_gather(pplpp)  i vqn_pack_x3_gather2(pplpplpp)
i vqn_neus_sdf_points_f16s(pppppplipp)  i vqn_neus_fine_points_f16s(pppppppppliplpppp)  i vqn_neus_sdf_points_x3(pppppplipp)
i vqn_neus_fine_points_x3(pppppppppliplpppp)  i vqn_neus_train_fwd_x3(pppppplplpiiiipppp)  i vqn_neus_pack_create(piiifiiiiiip)
i vqn_neus_pack_update(pppppp)  p vqn_neus_pack_sdf_desc(p)  p vqn_neus_pack_col_desc(p)  p vqn_neus_pack_sdf_wbuf(p)
p vqn_neus_pack_col_wbuf(p)  l vqn_neus_pack_sdf_floats(p)  l vqn_neus_pack_col_floats(p)  v vqn_neus_pack_destroy(p)
l vqn_neus_sdf_pack_plan(piiifiiippl)  l vqn_neus_col_pack_plan(iiiiiiiiippl)  i vqn_mlp_chain_vq_fwd(ppppplpppppiffpppppp)
i vqn_vq_codebook_frags(piipp)  i vqn_linear2srgb(plpp)  i vqn_chain_pack_create(iiiipp)  i vqn_chain_pack_update(pppp)
i vqn_chain_pack_n_weights(p)  p vqn_chain_pack_desc(p)  p vqn_chain_pack_wbuf(p)  l vqn_chain_pack_floats(p)
v vqn_chain_pack_destroy(p)  l vqn_chain_pack_plan(iiiipppl)  i vqn_neus_upsample(ppppliffpipp)  i vqn_neus_merge(ppppliippp)
i vqn_neus_section_mids(plifpppp)  i vqn_neus_composite_fwd(pppppppppliffppppppppppp)  i vqn_neus_composite_bwd(pppppppppliffpppppppppp)
i vqn_tile_program(pppppilp)  l vqn_tile_program_grid(pl)  i vqn_weight_norm_fwd(ipppppp)  i vqn_weight_norm_bwd(ipppppppp)
i vqn_tfmt_pack(plilpip)  i vqn_tfmt_pack_delta(plilpipip)  i vqn_tfmt_unpack(piliplp)  i vqn_wgrad_partials(piiipiiilippp)
i vqn_wgrad_partials_x3(piiipiiilippp)  i vqn_wgrad_partials_batched(ipppppppplippip)  i vqn_reduce_partials(piiiplip)
i vqn_wgrad_finalize(ipppppppppppppp)  i vqn_clip_preserve(plffpp)  i vqn_loss_total(plppiiipp)  i vqn_ks_split_fwd(ppilppp)
i vqn_ks_split_bwd(ppilppppp)  i vqn_wgrad_thin_batched(ippppppppplippp)  i vqn_multi_copy(ipppp)  i vqn_refl_train_desc_ints()
i vqn_refl_train_fwd_x3(ppppplpippiip)  i vqn_refl_train_fwd_x3_zx(pppppplpipppiip)  l vqn_refl_train_bwd_x3_scratch_bytes(p)
i vqn_refl_train_bwd_x3(ppplpppipipippiiiplp)  i vqn_adam_step(ippppppppdddddiip)
"""
# One table per public header of include/, in the same notation.  A new header is one more entry here: lib() installs whatever
# ABI_BY_HEADER holds.
_ABI_TEXT = {
    'vqnerf_hip.h': _ABI,
    'vqn_neus_fold.h': 'l vqn_neus_fold_pack(ppplppiippiplpp)',
    'vqn_mesh.h': """
i vqn_mc_classify(piiifppp)  i vqn_mc_emit(piiifppllppppp)  i vqn_mesh_components(pllpp)  i vqn_mesh_remap_tris(plppplplp)
i vqn_mc_brick_points(pppiiiplllpp)  i vqn_mc_brick_classify(pplpiiifppppp)  i vqn_mc_brick_emit(pplpiiifppllppppp)""",
    'vqn_eval.h': """
l vqn_image_metrics_scratch_bytes(lii)  i vqn_image_metrics_u8(ppplfliiipplpp)  i vqn_image_metrics_f32(ppplfliiipplpp)
l vqn_seg_scratch_bytes(lii)  i vqn_seg_contingency_rgb(pppflpipiplpp)  i vqn_seg_contingency_labels(pppliiplpp)
i vqn_meanshift_seek(plplidipppp)  l vqn_meanshift_merge_scratch_bytes(li)  i vqn_meanshift_merge(pplidplppp)
i vqn_meanshift_assign(plpiidppp)""",
    'vqn_material_edit.h': 'i vqn_material_select_edit(pppiplppipipfppppppppppppp)',
    'vqn_material_balls.h': 'i vqn_material_balls(pipippiiifpipppppiiiplp)',
    'vqn_mesh_materials.h': """
l vqn_mesh_label_scratch_bytes(ll)  i vqn_mesh_label_mode(plpliiippplp)  i vqn_mesh_split_count(plplippppp)
i vqn_mesh_split_emit(pllippppllpppp)""",
    'vqn_mesh_raster.h': 'i vqn_raster_count(plplpiifipppp)  i vqn_raster_resolve(plpliiiplpppppp)  i vqn_raster_interpolate(ppiiplplipipp)',
    'vqn_mesh_rays.h': """
i vqn_rays_grid_plan(pplfp)  i vqn_rays_count(plplpppp)  i vqn_rays_bin(plplpplpppp)  i vqn_rays_cast(plpplppppplpppp)
i vqn_rays_occluded(plpplppppplpp)  i vqn_rays_light_visibility(plpplppplpifipp)""",
    'vqn_image_codec.h': """
i vqn_jpeg_plan(llliilppi)  i vqn_jpeg_encode(pllliilplplpip)  i vqn_png_plan(llllilppi)  i vqn_png_encode(pllllilplplpip)""",
    'vqn_geometry_eval.h': """
i vqn_geom_tri_areas(plplpp)  i vqn_geom_sample_surface(plplpplpppp)  i vqn_geom_grid_plan(pplfp)  i vqn_geom_cell_ids(plppp)
i vqn_geom_pack_sorted(plppp)  i vqn_geom_nearest(plppplpfppp)  l vqn_geom_reduce_scratch_bytes(l)
i vqn_geom_reduce(pplpplpiplpp)""",
}
ABI_BY_HEADER = {header: {name: (ret, args) for ret, name, args in re.findall(r'(\w) (\w+)\((\w*)\)', text)}
                 for header, text in _ABI_TEXT.items()}
ABI = ABI_BY_HEADER['vqnerf_hip.h']
_CTYPES = dict(p=ctypes.c_void_p, i=ctypes.c_int, l=ctypes.c_int64, f=ctypes.c_float, d=ctypes.c_double, s=ctypes.c_char_p, v=None)


class VqnError(RuntimeError):
    pass


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    cmd = ['make', '-C', os.path.join(_HERE, 'csrc'), '-j8']
    if not verbose:
        cmd.append('-s')
    subprocess.check_call(cmd)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VqnError(f'{LIB_PATH} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(or `make -C vqnerf_release_amd/csrc`). There is no non-HIP fallback.')
        L = ctypes.CDLL(LIB_PATH)
        for table in ABI_BY_HEADER.values():
            for name, (ret, args) in table.items():
                f = getattr(L, name)
                f.restype, f.argtypes = _CTYPES[ret], [_CTYPES[a] for a in args]
        _lib = L
    return _lib


def require_device(t, what):
    """Inference (no autograd graph) runs only on the HIP kernels: CPU tensors are an error, not a fallback."""
    if not t.is_cuda:
        raise VqnError(f'{what}: got a {t.device} tensor; the no-graph path runs on MI355X HIP kernels only '
                       '(there is no CPU fallback)')
    lib()


def _check(rc, name, count=False):
    """rc of `name`: 0 on success -- or, count=True, a positive count, which is returned."""
    if (rc > 0) if count else (rc == 0):
        return rc
    raise VqnError(f'{name} failed (rc={rc or -3}): {lib().vqn_last_error().decode()}')


def _call(name, *args, clock=True, count=False):
    """lib().<name>(*args, torch's current stream), checked (see _check), inside the KernelClock bracket `clock`: True = the
    entry's own name, a string = that label, False = not clocked."""
    with _clock(name if clock is True else clock) if clock else contextlib.nullcontext():
        rc = getattr(lib(), name)(*args, _stream())
    return _check(rc, name, count)


def _ptr(t):
    """pointer argument of a tensor (None: NULL; an int is an address already)"""
    return t if t is None or isinstance(t, int) else t.data_ptr()


def _ptrs(ts, n=1):
    """host array of the pointers of `ts` (as _ptr), at least n entries (the rest NULL)"""
    return (ctypes.c_void_p * max(n, len(ts)))(*[_ptr(t) for t in ts])


def _host(a, dtype=np.int32):
    """host array of the values `a` for a pointer argument (no copy of a contiguous array of that dtype)"""
    return np.ascontiguousarray(a, dtype=dtype).ctypes


def _i32(desc):
    """-> (desc as a contiguous int32 array, its pointer argument)"""
    d = np.ascontiguousarray(desc, dtype=np.int32)
    return d, d.ctypes.data_as(ctypes.c_void_p)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class KernelClock:
    """Optional per-kernel device timing: HIP events recorded on the stream the kernel is launched on
    (torch's current stream).  Off by default; bench.py switches it on for the timed region.
    Events are POOLED: a process that keeps creating event pairs (two per clocked call, all alive until the summary) runs into a
    one-off stall of tens of ms when the runtime extends its event pool -- scripts/debug/launch_stall.py: 37 ms at the 2,400th live
    event, none for plain launches -- which round 3's bench had to prime its training legs past.  reset() hands the window's events
    back to the free list instead of dropping them."""
    enabled = False
    pairs = {}
    _free = []

    @classmethod
    def _event(cls):
        return cls._free.pop() if cls._free else torch.cuda.Event(enable_timing=True)

    @classmethod
    def reserve(cls, n):
        """create n events now (outside any timed region)"""
        while len(cls._free) < n:
            cls._free.append(torch.cuda.Event(enable_timing=True))

    @classmethod
    def reset(cls, enabled=True):
        for v in cls.pairs.values():
            for a, b in v:
                cls._free.append(a)
                cls._free.append(b)
        cls.enabled = enabled
        cls.pairs = {}

    @classmethod
    def summary(cls):
        """{name: (launches, total_ms)} -- call after torch.cuda.synchronize()."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in cls.pairs.items()}


class _clock:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        # (not while a HIP graph records: an event recorded into a capture has no time stamp; the launch is still counted)
        self.on = KernelClock.enabled and not torch.cuda.is_current_stream_capturing()
        if KernelClock.enabled and not self.on:
            KernelClock.pairs.setdefault(self.name + ' [captured]', [])
        if self.on:
            self.e0 = KernelClock._event()
            self.e0.record()

    def __exit__(self, *exc):
        if self.on:
            e1 = KernelClock._event()
            e1.record()
            KernelClock.pairs.setdefault(self.name, []).append((self.e0, e1))
        return False


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise VqnError(f'{name}: expected a contiguous float32 device tensor, got {t.dtype} '
                       f'contiguous={t.is_contiguous()} device={t.device}')
    return t


# --------------------------------------------------------------------------------------
def vq_assign(x, codebook, sel_mask=None, want_quant=True, want_dist=False):
    """x [N,D], codebook [D,K] -> (idx int64 [N], quant [N,D] | None, dist [N,K] | None)."""
    _f32c(x, 'x'); _f32c(codebook, 'codebook')
    N, D = x.shape
    K = codebook.shape[1]
    assert codebook.shape[0] == D
    idx = torch.empty((N,), dtype=torch.int64, device=x.device)
    quant = torch.empty((N, D), dtype=torch.float32, device=x.device) if want_quant else None
    dist = torch.empty((N, K), dtype=torch.float32, device=x.device) if want_dist else None
    ws = None
    if sel_mask is not None:
        sel_mask = _f32c(sel_mask.reshape(-1).to(torch.float32).contiguous(), 'sel_mask')
        assert sel_mask.numel() == K
        ws = torch.empty((4,), dtype=torch.float32, device=x.device)
    _call('vqn_vq_assign', _ptr(x), N, D, _ptr(codebook), K, _ptr(sel_mask), _ptr(ws), _ptr(idx), _ptr(quant), _ptr(dist))
    return idx, quant, dist


def vq_assign_variant(D, K, has_sel_mask=False, has_dist=False):
    """0: the f32 kernel, 1: the prefiltered kernel (vqn_vq_assign_variant)."""
    return lib().vqn_vq_assign_variant(D, K, bool(has_sel_mask), bool(has_dist))


def vq_ema_stats(x, idx, K):
    """x [N,D], idx [N] int64 -> (counts [K], dw [D,K])."""
    _f32c(x, 'x')
    N, D = x.shape
    assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == N
    counts = torch.empty((K,), dtype=torch.float32, device=x.device)
    dw = torch.empty((D, K), dtype=torch.float32, device=x.device)
    need = lib().vqn_vq_ema_stats_ws_bytes(N, D, K)
    ws = torch.empty((need // 4,), dtype=torch.float32, device=x.device) if need > 0 else None
    _call('vqn_vq_ema_stats', _ptr(x), _ptr(idx), N, D, K, _ptr(counts), _ptr(dw), _ptr(ws), need)
    return counts, dw



def vq_counts(idx, K):
    """idx [N] int64 -> counts [K] float32 (= one_hot(idx, K).sum(0) without the [N,K] pass)."""
    assert idx.dtype == torch.int64 and idx.is_contiguous()
    counts = torch.empty((K,), dtype=torch.float32, device=idx.device)
    _call('vqn_vq_ema_stats', None, _ptr(idx), idx.numel(), 4, K, _ptr(counts), None, None, 0)
    return counts


def vq_ste_loss(x, quant, want_ste=True):
    """x, quant [N,D] -> (x + (quant - x) [N,D] or None, mean((quant - x)^2) scalar tensor), one fused pass."""
    _f32c(x, 'x'); _f32c(quant, 'quant')
    assert x.shape == quant.shape
    n = x.numel()
    ste = torch.empty_like(x) if want_ste else None
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = torch.empty((1024,), dtype=torch.float32, device=x.device)
    _call('vqn_vq_ste_loss', _ptr(x), _ptr(quant), n, 1.0 / n if n else 0.0, _ptr(ste), _ptr(loss), _ptr(ws))
    return ste, loss

def vq_ema_update(counts, dw, codebook, decay, eps, ema_cs, ema_dw):
    """One launch for the EMA codebook move (both averages' state updated in place) -> update [D,K]."""
    _f32c(counts, 'counts'); _f32c(dw, 'dw'); _f32c(codebook, 'codebook')
    D, K = codebook.shape
    for m in (ema_cs, ema_dw):
        _f32c(m.hidden, 'hidden'); _f32c(m.average, 'average')
        assert m.counter.dtype == torch.int64 and m.counter.is_cuda
    update = torch.empty_like(codebook)
    _call('vqn_vq_ema_update', _ptr(counts), _ptr(dw), _ptr(codebook), D, K, decay, eps, _ptr(ema_cs.hidden), _ptr(ema_cs.average),
          _ptr(ema_cs.counter), _ptr(ema_dw.hidden), _ptr(ema_dw.average), _ptr(ema_dw.counter), _ptr(update))
    return update


def _loss_args(rgb_pred, vq_rgb, rgb_gt, z, spec, rough, nerf, w):
    for t, n in ((rgb_pred, 'rgb_pred'), (vq_rgb, 'vq_rgb'), (rgb_gt, 'rgb_gt')):
        _f32c(t, n)
    for t, n in ((z, 'z'), (spec, 'spec'), (rough, 'rough')):
        if t is not None:
            _f32c(t, n)
    N = rgb_pred.shape[0]
    D = 0 if z is None else z.shape[1]
    return (_ptr(rgb_pred), _ptr(vq_rgb), _ptr(rgb_gt), _ptr(z), _ptr(spec), _ptr(rough), N, D, 1 if nerf else 0) + \
        tuple(float(w[k]) for k in ('rgb', 'chr', 'smooth', 'alpha', 'thres', 'lambert'))


def decomp_loss_fwd(rgb_pred, vq_rgb, rgb_gt, z, spec, rough, nerf, w):
    """-> terms [N,5] (rgb, vqrgb, chromaticity, chr_smooth, lambert); w: dict of the six scalars (see include/vqnerf_hip.h)."""
    terms = torch.empty((rgb_pred.shape[0], 5), dtype=torch.float32, device=rgb_pred.device)
    _call('vqn_decomp_loss_fwd', *_loss_args(rgb_pred, vq_rgb, rgb_gt, z, spec, rough, nerf, w), _ptr(terms))
    return terms


def decomp_loss_bwd(rgb_pred, vq_rgb, rgb_gt, z, spec, rough, nerf, w, g_terms):
    _f32c(g_terms, 'g_terms')
    g_pred, g_vq = torch.empty_like(rgb_pred), torch.empty_like(vq_rgb)
    g_z = None if z is None else torch.empty_like(z)
    g_spec = None if spec is None else torch.empty_like(spec)
    _call('vqn_decomp_loss_bwd', *_loss_args(rgb_pred, vq_rgb, rgb_gt, z, spec, rough, nerf, w), _ptr(g_terms), _ptr(g_pred), _ptr(g_vq),
          _ptr(g_z), _ptr(g_spec))
    return g_pred, g_vq, g_z, g_spec


def codebook_prep(raw, g=None, eps=1e-6):
    """clip-with-identity-gradient to [0, 1] + l2-normalise every column of raw [D, K] (g None), or the gradient wrt raw for g [D, K]."""
    _f32c(raw, 'raw')
    if g is not None:
        _f32c(g, 'g')
    out = torch.empty_like(raw)
    _call('vqn_codebook_prep', _ptr(raw), _ptr(g), raw.shape[0], raw.shape[1], eps, _ptr(out))
    return out


def sim_smooth_fwd(cb, weight):
    _f32c(cb, 'codebook')
    out = torch.empty(4, dtype=torch.float32, device=cb.device)
    _call('vqn_sim_smooth_fwd', _ptr(cb), cb.shape[0], cb.shape[1], weight, _ptr(out))
    return out


def sim_smooth_bwd(cb, fwd4, g_loss, weight):
    _f32c(cb, 'codebook'); _f32c(fwd4, 'fwd4'); _f32c(g_loss, 'g_loss')
    g = torch.empty_like(cb)
    _call('vqn_sim_smooth_bwd', _ptr(cb), _ptr(fwd4), _ptr(g_loss), cb.shape[0], cb.shape[1], weight, _ptr(g))
    return g


def l2_normalize_rows_bwd(x, g, eps=1e-6):
    """Gradient of l2_normalize_rows at x [N, D] for the incoming g [N, D]: one pass (vqn_l2_normalize_rows_bwd)."""
    _f32c(x, 'x'); _f32c(g, 'g')
    if x.shape != g.shape or x.dim() != 2:
        raise VqnError('l2_normalize_rows_bwd: x and g must be [N, D]')
    gx = torch.empty_like(x)
    _call('vqn_l2_normalize_rows_bwd', _ptr(x), _ptr(g), x.shape[0], x.shape[1], eps, _ptr(gx))
    return gx


def vq_ste_loss_bwd(x, quant, g_ste, g_loss):
    """g_ste + (x - quant) * (g_loss * 2 / numel) in one pass (g_ste may be None; g_loss a 0-dim device tensor)."""
    _f32c(x, 'x'); _f32c(quant, 'quant'); _f32c(g_loss, 'g_loss')
    if g_ste is not None:
        _f32c(g_ste, 'g_ste')
    gx = torch.empty_like(x)
    _call('vqn_vq_ste_loss_bwd', _ptr(x), _ptr(quant), _ptr(g_ste), _ptr(g_loss), x.numel(), _ptr(gx))
    return gx


def vq_train_bwd(z, xnorm, quant, g_ste, g_loss, eps=1e-6, loss_post=1.0):
    """Backward of the training quantiser in one pass (vqn_vq_train_bwd): straight-through + commitment adjoint, then the l2-normalise
    backward of z."""
    for t in (z, xnorm, quant, g_loss):
        _f32c(t, 'tensor')
    if g_ste is not None:
        _f32c(g_ste, 'g_ste')
    gz = torch.empty_like(z)
    _call('vqn_vq_train_bwd', _ptr(z), _ptr(xnorm), _ptr(quant), _ptr(g_ste), _ptr(g_loss), loss_post, z.shape[0], z.shape[1], eps, _ptr(gz))
    return gz


def l2_normalize_rows(x, eps=1e-6):
    """x [N,D] -> x / sqrt(max(sum_d x^2, eps)) row by row, in the defined summation order of vqn_vq_assign's |x|^2."""
    _f32c(x, 'x')
    y = torch.empty_like(x)
    _call('vqn_l2_normalize_rows', _ptr(x), x.shape[0], x.shape[1], eps, _ptr(y))
    return y


def vq_quantize_rows(z, codebook, sel_mask=None, eps=1e-6, want_ste=True, want_xnorm=False, loss_post=1.0):
    """Fused inference path: z [N,D] un-normalised, codebook [D,K] -> (idx int64 [N], ste [N,D] | None, mean((q - z^)^2) scalar
    tensor, counts [K]) in one pass over the rows (l2-normalise, nearest code, straight-through output, commitment term, usage)."""
    _f32c(z, 'z'); _f32c(codebook, 'codebook')
    N, D = z.shape
    K = codebook.shape[1]
    assert codebook.shape[0] == D
    dev = z.device
    idx = torch.empty((N,), dtype=torch.int64, device=dev)
    ste = torch.empty((N, D), dtype=torch.float32, device=dev) if want_ste else None
    loss = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty((K,), dtype=torch.float32, device=dev)
    ws = torch.empty((4096,), dtype=torch.float32, device=dev)
    if sel_mask is not None:
        sel_mask = _f32c(sel_mask.reshape(-1).to(torch.float32).contiguous(), 'sel_mask')
        assert sel_mask.numel() == K
    n = N * D
    if want_xnorm:                                         # the training form: the normalised rows are kept (EMA statistics, backward)
        xnorm = torch.empty((N, D), dtype=torch.float32, device=dev)
        _call('vqn_vq_quantize_rows_train', _ptr(z), N, D, _ptr(codebook), K, _ptr(sel_mask), eps, 1.0 / n if n else 0.0, loss_post, _ptr(ws),
              _ptr(idx), _ptr(ste), _ptr(loss), _ptr(counts), _ptr(xnorm))
        return idx, ste, loss, counts, xnorm
    _call('vqn_vq_quantize_rows', _ptr(z), N, D, _ptr(codebook), K, _ptr(sel_mask), eps, 1.0 / n if n else 0.0, _ptr(ws), _ptr(idx), _ptr(ste),
          _ptr(loss), _ptr(counts))
    return idx, ste, loss, counts


# --------------------------------------------------------------------------------------
# device scratch of the fused kernels
_scratch_cache = {}      # (device, stream, tag) -> [buffer, held]
_scratch_held = []       # held buffers a larger request replaced: kept for the life of the process


def _scratch(tag, need, device, stream=None, capturing=None):
    """A uint8 buffer of at least `need` bytes for a launch on `stream` (default: torch's current one): one per (device, stream, tag),
    grown, never shrunk; equal tags share it.  A buffer handed out while a graph records (`capturing`, default: asks torch) is held:
    the graph replays with its pointer, so when a larger request replaces it, it stays alive in _scratch_held instead of being freed."""
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    if capturing is None:
        capturing = torch.cuda.is_current_stream_capturing()
    key = (str(device), stream, tag)
    entry = _scratch_cache.get(key)
    if entry is None or entry[0].numel() < need:
        if entry is not None and entry[1]:
            _scratch_held.append(entry[0])
        entry = _scratch_cache[key] = [torch.empty((need,), dtype=torch.uint8, device=device), False]
    entry[1] = entry[1] or capturing
    return entry[0]


def _scratch_bytes(name, desc):
    """the scratch size query `name` of a descriptor; raises on an invalid one"""
    need = getattr(lib(), name)(desc)
    if need <= 0:
        raise VqnError(f'{name}: invalid descriptor')
    return need


# --------------------------------------------------------------------------------------
# fused NeuS networks (csrc/neus_mlp.hip)
def neus_sdf_points(sdf_desc, wbuf_sdf, rays_o=None, rays_d=None, z=None, pts=None, mode='f32', pack=None):
    """SDF value at ray samples (rays_o/rays_d [B,3], z [B,S]) or at explicit pts [P,3] -> [P].  pack: a NeusPackHandle (its
    descriptor and SDF buffer are used, `mode` names the engine it was created for)."""
    if pack is not None:
        dp, wp = pack.sdf_desc, pack.sdf_wbuf
    else:
        _f32c(wbuf_sdf, 'wbuf_sdf')
        dp, wp = _host(sdf_desc), _ptr(wbuf_sdf)
    if pts is not None:
        _f32c(pts, 'pts'); P, S = pts.shape[0], 1
        dev = pts.device
    else:
        _f32c(rays_o, 'rays_o'); _f32c(rays_d, 'rays_d'); _f32c(z, 'z')
        B, S = z.shape
        P = B * S
        dev = z.device
    out = torch.empty((P,), dtype=torch.float32, device=dev)
    entry = {'f32': 'vqn_neus_sdf_points', 'f16s': 'vqn_neus_sdf_points_f16s', 'x3': 'vqn_neus_sdf_points_x3'}[mode]
    _call(entry, dp, wp, _ptr(rays_o), _ptr(rays_d), _ptr(z), _ptr(pts), P, S, _ptr(out))
    return out


def neus_fine_points(sdf_desc, wbuf_sdf, col_desc, wbuf_col, rays_o=None, rays_d=None, z=None, pts=None, dirs=None, mode='f32'):
    """sdf [P], d sdf/d x [P,3], rgb [P,3] at ray samples or explicit (pts, dirs)."""
    _f32c(wbuf_sdf, 'wbuf_sdf'); _f32c(wbuf_col, 'wbuf_col')
    sdp, cdp = _host(sdf_desc), _host(col_desc)
    if pts is not None:
        _f32c(pts, 'pts'); _f32c(dirs, 'dirs'); P, S = pts.shape[0], 1
        dev = pts.device
    else:
        _f32c(rays_o, 'rays_o'); _f32c(rays_d, 'rays_d'); _f32c(z, 'z')
        B, S = z.shape
        P = B * S
        dev = z.device
    buf = _scratch('fine', _scratch_bytes('vqn_neus_fine_scratch_bytes', sdp), dev)
    sdf = torch.empty((P,), dtype=torch.float32, device=dev)
    grad = torch.empty((P, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((P, 3), dtype=torch.float32, device=dev)
    entry = {'f32': 'vqn_neus_fine_points', 'f16s': 'vqn_neus_fine_points_f16s', 'x3': 'vqn_neus_fine_points_x3'}[mode]
    _call(entry, sdp, _ptr(wbuf_sdf), cdp, _ptr(wbuf_col), _ptr(rays_o), _ptr(rays_d), _ptr(z), _ptr(pts), _ptr(dirs), P, S, _ptr(buf),
          buf.numel(), _ptr(sdf), _ptr(grad), _ptr(rgb))
    return sdf, grad, rgb


def neus_fold_pack(sdf_desc, col_desc, wbuf_col, sdf_w_last, sdf_b_last, col_w0, col_b0):
    """Folded colour pack of the f32 fine kernel (csrc/neus_fold.hip): (wbuf, desc) to hand to neus_fine_points in place of
    (wbuf_col, col_desc).  sdf_w_last [1 + F, H] / sdf_b_last and col_w0 [C, extras + F] / col_b0: the effective weights the packs
    were gathered from."""
    for t in (wbuf_col, sdf_w_last, sdf_b_last, col_w0, col_b0):
        _f32c(t, 'weight / bias')
    (F1, H), C = sdf_w_last.shape, col_w0.shape[0]
    sdp, cdp = _host(sdf_desc), _host(col_desc)
    desc = np.zeros(len(col_desc), np.int32)
    args = (sdp, cdp, _ptr(wbuf_col), wbuf_col.numel(), _ptr(sdf_w_last), _ptr(sdf_b_last), H, F1 - 1, _ptr(col_w0), _ptr(col_b0), C)
    n = _call('vqn_neus_fold_pack', *args, None, 0, None, clock=False, count=True)
    out = torch.empty((n,), dtype=torch.float32, device=wbuf_col.device)
    _call('vqn_neus_fold_pack', *args, _ptr(out), n, desc.ctypes.data_as(ctypes.c_void_p), count=True)
    return out, desc


class NeusPackHandle:
    """vqn_neus_pack_create / _update / _destroy: the packs of one (SDFNetwork, RenderingNetwork) shape built by the library from
    tables of device pointers to the effective weights [out, in] and biases (one gather launch per network and update)."""

    def __init__(self, sdf_dims, sdf_skip, multires, scale, col_mode, col_d_hidden, col_n_layers, multires_view, squeeze_out, engine):
        L = lib()
        self.h = ctypes.c_void_p()
        _check(L.vqn_neus_pack_create(_host(sdf_dims), len(sdf_dims) - 1, sdf_skip, multires, scale, col_mode, col_d_hidden, col_n_layers,
                                      multires_view, int(squeeze_out), engine, ctypes.byref(self.h)), 'vqn_neus_pack_create')
        self.sdf_desc, self.col_desc = L.vqn_neus_pack_sdf_desc(self.h), L.vqn_neus_pack_col_desc(self.h)
        self.sdf_wbuf, self.col_wbuf = L.vqn_neus_pack_sdf_wbuf(self.h), L.vqn_neus_pack_col_wbuf(self.h)

    def update(self, W, b, Wc, bc):
        for t in W + b + Wc + bc:
            _f32c(t, 'weight / bias')
        _call('vqn_neus_pack_update', self.h, _ptrs(W), _ptrs(b), _ptrs(Wc), _ptrs(bc))

    def __del__(self):
        try:
            if self.h:
                lib().vqn_neus_pack_destroy(self.h)
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass


def neus_train_fwd(sdf_desc, wbuf_sdf, col_desc, wbuf_col, pts, dirs, saved, e_tiles, outf_tiles, extr_tiles, out_sdf, out_n, out_rgb, pack=None):
    """Training forward of the NeuS core at explicit (pts, dirs): the two-image fine kernel, which also leaves the tensors the backward
    tile programs read (`saved`: [E, OUTF, EXTR, U_1.., GH_0.., C_1..], tile format).  Fills out_sdf [P,1], out_n [P,3], out_rgb [P,3].
    pack: a NeusPackHandle of the exact-split engine -> vqn_neus_train_fwd_x3 on its packs (the descriptor / buffer arguments unused)."""
    _f32c(pts, 'pts'); _f32c(dirs, 'dirs')
    for t in saved + [out_sdf, out_n, out_rgb]:
        _f32c(t, 'saved tensor')
    if pack is not None:
        sdp, cdp, wsp, wcp, entry = pack.sdf_desc, pack.col_desc, pack.sdf_wbuf, pack.col_wbuf, 'vqn_neus_train_fwd_x3'
    else:
        _f32c(wbuf_sdf, 'wbuf_sdf'); _f32c(wbuf_col, 'wbuf_col')
        sdp, cdp, wsp, wcp, entry = _host(sdf_desc), _host(col_desc), _ptr(wbuf_sdf), _ptr(wbuf_col), 'vqn_neus_train_fwd'
    P, dev = pts.shape[0], pts.device
    buf = _scratch('fine', _scratch_bytes('vqn_neus_fine_scratch_bytes', sdp), dev)
    _call(entry, sdp, wsp, cdp, wcp, _ptr(pts), _ptr(dirs), P, _ptr(buf), buf.numel(), _ptrs(saved), len(saved), e_tiles, outf_tiles,
          extr_tiles, _ptr(out_sdf), _ptr(out_n), _ptr(out_rgb))


def pack_x3_gather(flat, gidx, n_steps, fidx=None):
    """bf16 piece triples [n_steps, 3, 64, 8] (as an int16 tensor) of flat[gidx] -- gather + exact split in one launch.  With `fidx`
    (a contiguous int32 index tensor on flat's device): also flat[fidx], in the same launch -> (pieces, f32 images)."""
    _f32c(flat, 'flat')
    if gidx.dtype != torch.int32 or not gidx.is_contiguous() or gidx.numel() != n_steps * 512:
        raise VqnError('pack_x3_gather: gidx must be a contiguous int32 tensor of n_steps * 512 entries')
    out = torch.empty((n_steps, 3, 64, 8), dtype=torch.int16, device=flat.device)
    if fidx is None:
        _call('vqn_pack_x3_gather', _ptr(flat), _ptr(gidx), n_steps, _ptr(out))
        return out
    if fidx.dtype != torch.int32 or not fidx.is_contiguous() or fidx.device != flat.device:
        raise VqnError('pack_x3_gather: fidx must be a contiguous int32 tensor on the device of flat')
    wf = torch.empty(fidx.shape, dtype=torch.float32, device=flat.device)
    _call('vqn_pack_x3_gather2', _ptr(flat), _ptr(gidx), n_steps, _ptr(out), _ptr(fidx), fidx.numel(), _ptr(wf), clock='vqn_pack_x3_gather')
    return out, wf


def neus_train_bwd_x3(desc, wbuf_pieces, wbuf_f32, pts, g_rgb, rgb, g_n, g_sdf, saved, outs):
    """neus_train_bwd on the exact-split engine (csrc/neus_train_bwd_x3.hip)."""
    _f32c(wbuf_f32, 'wbuf_f32'); _f32c(pts, 'pts'); _f32c(g_rgb, 'g_rgb')
    for t in saved + outs + [t for t in (rgb, g_n, g_sdf) if t is not None]:
        _f32c(t, 'tensor')
    dp = _host(desc)
    buf = _scratch('bwd', _scratch_bytes('vqn_neus_train_bwd_x3_scratch_bytes', dp), pts.device)
    _call('vqn_neus_train_bwd_x3', dp, _ptr(wbuf_pieces), _ptr(wbuf_f32), _ptr(pts), _ptr(g_rgb), _ptr(rgb), _ptr(g_n), _ptr(g_sdf),
          pts.shape[0], _ptr(buf), buf.numel(), _ptrs(saved), len(saved), _ptrs(outs), len(outs))


def neus_train_bwd(desc, wbuf, pts, g_rgb, rgb, g_n, g_sdf, saved, outs):
    """Backward of the NeuS core in one launch (csrc/neus_train_bwd.hip): fills `outs` ([DC_0.., GOUTF, ED, UD_1.., AB_0..]) from the
    incoming adjoints and the forward's `saved` tensors ([U_1.., GH_0.., C_1..]); rgb / g_n / g_sdf may be None."""
    _f32c(wbuf, 'wbuf'); _f32c(pts, 'pts'); _f32c(g_rgb, 'g_rgb')
    for t in saved + outs + [t for t in (rgb, g_n, g_sdf) if t is not None]:
        _f32c(t, 'tensor')
    dp = _host(desc)
    buf = _scratch('bwd', _scratch_bytes('vqn_neus_train_bwd_scratch_bytes', dp), pts.device)
    _call('vqn_neus_train_bwd', dp, _ptr(wbuf), _ptr(pts), _ptr(g_rgb), _ptr(rgb), _ptr(g_n), _ptr(g_sdf), pts.shape[0], _ptr(buf),
          buf.numel(), _ptrs(saved), len(saved), _ptrs(outs), len(outs))


def multi_copy(dsts, srcs):
    """dsts[i].copy_(srcs[i]) for contiguous f32 tensors of equal element counts, all in ONE launch (vqn_multi_copy)."""
    k = len(dsts)
    if k == 0:
        return
    for d, s in zip(dsts, srcs):
        _f32c(d, 'dst'); _f32c(s, 'src')
        if d.numel() != s.numel():
            raise VqnError('multi_copy: element counts differ')
    _call('vqn_multi_copy', k, _ptrs(srcs), _ptrs(dsts), _host([t.numel() for t in dsts], np.int64))


# --------------------------------------------------------------------------------------
# per-ray NeuS kernels (csrc/neus_rays.hip)
def neus_upsample(rays_o, rays_d, z, sdf, r_limit, inv_s, u):
    _f32c(rays_o, 'rays_o'); _f32c(rays_d, 'rays_d'); _f32c(z, 'z'); _f32c(sdf, 'sdf'); _f32c(u, 'u')
    B, n = z.shape
    m = u.numel()
    z_new = torch.empty((B, m), dtype=torch.float32, device=z.device)
    _call('vqn_neus_upsample', _ptr(rays_o), _ptr(rays_d), _ptr(z), _ptr(sdf), B, n, r_limit, inv_s, _ptr(u), m, _ptr(z_new))
    return z_new


def neus_merge(z, sdf, z_new, sdf_new):
    _f32c(z, 'z'); _f32c(z_new, 'z_new')
    B, n = z.shape
    m = z_new.shape[1]
    z_out = torch.empty((B, n + m), dtype=torch.float32, device=z.device)
    sdf_out = None
    if sdf is not None and sdf_new is not None:
        _f32c(sdf, 'sdf'); _f32c(sdf_new, 'sdf_new')
        sdf_out = torch.empty((B, n + m), dtype=torch.float32, device=z.device)
    _call('vqn_neus_merge', _ptr(z), _ptr(sdf if sdf_out is not None else None), _ptr(z_new), _ptr(sdf_new if sdf_out is not None else None),
          B, n, m, _ptr(z_out), _ptr(sdf_out))
    return z_out, sdf_out


def neus_section_mids(z, sample_dist, sample_dist_per_ray=None):
    _f32c(z, 'z')
    B, n = z.shape
    mid = torch.empty_like(z)
    dists = torch.empty_like(z)
    if sample_dist_per_ray is not None:
        sample_dist_per_ray = _f32c(sample_dist_per_ray.reshape(-1).contiguous(), 'sample_dist_per_ray')
    _call('vqn_neus_section_mids', _ptr(z), B, n, float(sample_dist), _ptr(sample_dist_per_ray), _ptr(mid), _ptr(dists))
    return mid, dists


def neus_composite_fwd(rays_o, rays_d, mid_z, dists, sdf, grad, rgb, inv_s, background_rgb, radius,
                       cos_anneal_ratio, want_alpha=False):
    for n_, t in (('rays_o', rays_o), ('rays_d', rays_d), ('mid_z', mid_z), ('dists', dists), ('sdf', sdf),
                  ('grad', grad), ('rgb', rgb), ('inv_s', inv_s)):
        _f32c(t, n_)
    B, n = mid_z.shape
    dev = mid_z.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = dict(color=f(B, 3), weights=f(B, n), cdf=f(B, n), inside_sphere=f(B, n), surf=f(B, 3), depth=f(B, 1),
               weight_sum=f(B, 1), weight_max=f(B, 1), gerr=f(B, 2))
    alpha = f(B, n) if want_alpha else None
    if background_rgb is not None:
        background_rgb = _f32c(background_rgb.reshape(-1)[:3].contiguous(), 'background_rgb')
    _call('vqn_neus_composite_fwd', _ptr(rays_o), _ptr(rays_d), _ptr(mid_z), _ptr(dists), _ptr(sdf), _ptr(grad), _ptr(rgb), _ptr(inv_s),
          _ptr(background_rgb), B, n, float(radius), float(cos_anneal_ratio), *[_ptr(t) for t in out.values()], _ptr(alpha))
    if want_alpha:
        out['alpha'] = alpha
    return out


# --------------------------------------------------------------------------------------
# mesh export (csrc/marching_cubes.hip; geo/mesh.py)
def _mc_field(u):
    _f32c(u, 'u')
    if u.dim() != 3:
        raise VqnError(f'marching cubes: expected a field [nx, ny, nz], got shape {tuple(u.shape)}')
    return tuple(int(s) for s in u.shape)


def mc_classify(u, threshold):
    """u [nx,ny,nz] -> (vert_count, tri_count) int32 [nx*ny*nz]: owned crossing edges per grid point, triangles per cell."""
    nx, ny, nz = _mc_field(u)
    vcount = torch.empty((u.numel(),), dtype=torch.int32, device=u.device)
    tcount = torch.empty((u.numel(),), dtype=torch.int32, device=u.device)
    _call('vqn_mc_classify', _ptr(u), nx, ny, nz, float(threshold), _ptr(vcount), _ptr(tcount))
    return vcount, tcount


def mc_emit(u, threshold, vert_offset, tri_offset, n_verts, n_tris, origin=None, step=None):
    """The mesh of u = threshold from the exclusive prefix sums of mc_classify's counts and their totals -> (verts [V,3] f32,
    tris [T,3] int32).  origin / step: three floats each (host), applied as index * step + origin on write."""
    nx, ny, nz = _mc_field(u)
    for t in (vert_offset, tri_offset):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != u.device or t.numel() != u.numel():
            raise VqnError('mc_emit: offsets must be contiguous int32 tensors on the device of u, one entry per grid point')
    verts = torch.empty((n_verts, 3), dtype=torch.float32, device=u.device)
    tris = torch.empty((n_tris, 3), dtype=torch.int32, device=u.device)
    _call('vqn_mc_emit', _ptr(u), nx, ny, nz, float(threshold), _ptr(vert_offset), _ptr(tri_offset), n_verts, n_tris,
          None if origin is None else _host(origin, np.float32), None if step is None else _host(step, np.float32),
          _ptr(verts) if n_verts else None, _ptr(tris) if n_tris else None)
    return verts, tris


def _mesh_tris(triangles, what):
    if triangles.dtype != torch.int32 or not triangles.is_contiguous() or not triangles.is_cuda or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise VqnError(f'{what}: expected contiguous int32 device triangles [T, 3], got {triangles.dtype} {tuple(triangles.shape)} '
                       f'contiguous={triangles.is_contiguous()} device={triangles.device}')
    return triangles.shape[0]


def mesh_components(triangles, n_verts):
    """triangles [T,3] int32 -> labels [n_verts] int32, labels[v] = the smallest vertex index of v's component (csrc/mesh_components.hip)."""
    T = _mesh_tris(triangles, 'mesh_components')
    labels = torch.empty((n_verts,), dtype=torch.int32, device=triangles.device)
    _call('vqn_mesh_components', _ptr(triangles) if T else None, T, n_verts, _ptr(labels) if n_verts else None)
    return labels


def mesh_remap_tris(triangles, keep_tri, tri_offset, new_index, n_out):
    """The triangles with keep_tri (bool / uint8 [T]) set, in order, at rows tri_offset (int32 [T], the exclusive prefix sum of
    keep_tri; n_out its total), vertex ids rewritten through new_index (int32 [V]) -> [n_out, 3] int32."""
    T = _mesh_tris(triangles, 'mesh_remap_tris')
    keep_tri = keep_tri.view(torch.uint8) if keep_tri.dtype == torch.bool else keep_tri
    for t, dt, n in ((keep_tri, torch.uint8, T), (tri_offset, torch.int32, T), (new_index, torch.int32, new_index.numel())):
        if t.dtype != dt or not t.is_contiguous() or t.device != triangles.device or t.dim() != 1 or t.numel() != n:
            raise VqnError('mesh_remap_tris: keep_tri (uint8) and tri_offset (int32) need one entry per triangle, new_index (int32) one '
                           'per vertex, contiguous and on the device of the triangles')
    if not 0 <= n_out <= T:
        raise VqnError(f'mesh_remap_tris: n_out = {n_out} is not the size of a subset of {T} triangles')
    out = torch.empty((n_out, 3), dtype=torch.int32, device=triangles.device)
    if T and n_out:
        _call('vqn_mesh_remap_tris', _ptr(triangles), T, _ptr(keep_tri), _ptr(tri_offset), _ptr(new_index) if new_index.numel() else None,
              new_index.numel(), _ptr(out), n_out)
    return out


# mesh export on a sparse set of bricks (csrc/marching_cubes_bricks.hip; geo/mesh.py)
# (this and every block of constants below: the #defines of the area's header, include/vqn_mesh.h here; tests/test_abi_headers.py
# holds them equal)
BRICK_CELLS = 8               # cells per brick and axis (VQN_MC_BRICK_CELLS)
BRICK_POINTS = 729            # stored points of a brick: 9^3 (VQN_MC_BRICK_POINTS)


def _mc_bricks(ub, brick_ijk, slot, dims):
    """checks of the brick arguments -> (n_bricks, nx, ny, nz)"""
    nx, ny, nz = (int(d) for d in dims)
    n = brick_ijk.shape[0]
    if brick_ijk.dtype != torch.int32 or not brick_ijk.is_contiguous() or not brick_ijk.is_cuda or tuple(brick_ijk.shape) != (n, 3):
        raise VqnError(f'marching cubes on bricks: brick_ijk must be a contiguous int32 device tensor [n, 3], got {brick_ijk.dtype} '
                       f'{tuple(brick_ijk.shape)} on {brick_ijk.device}')
    if ub is not None:
        _f32c(ub, 'ub')
        if ub.numel() != n * BRICK_POINTS or ub.device != brick_ijk.device:
            raise VqnError(f'marching cubes on bricks: ub must hold [n, 9, 9, 9] values for n = {n} bricks on the device of brick_ijk, '
                           f'got shape {tuple(ub.shape)}')
    if slot is not None:
        n_slots = 1
        for d in (nx, ny, nz):
            n_slots *= max(1, -(-(d - 1) // BRICK_CELLS))                         # (a dimension < 2 is the library's to refuse)
        if slot.dtype != torch.int32 or not slot.is_contiguous() or slot.device != brick_ijk.device or slot.numel() != n_slots:
            raise VqnError(f'marching cubes on bricks: slot must be a contiguous int32 tensor with one entry per brick of the grid '
                           f'({n_slots}) on the device of brick_ijk')
    return n, nx, ny, nz


def mc_brick_points(axes, dims, brick_ijk, first, count):
    """The stored points [first, first + count) of the bricks brick_ijk [n,3] (729 per brick, padding repeats the brick's last
    point) as rows [count, 3] of the three device axis arrays `axes`."""
    n, nx, ny, nz = _mc_bricks(None, brick_ijk, None, dims)
    for a, d in zip(axes, (nx, ny, nz)):
        _f32c(a, 'axis')
        if a.numel() != d or a.device != brick_ijk.device:
            raise VqnError('mc_brick_points: one contiguous f32 axis array of the grid\'s length per dimension, on the device of brick_ijk')
    pts = torch.empty((count, 3), dtype=torch.float32, device=brick_ijk.device)
    _call('vqn_mc_brick_points', _ptr(axes[0]), _ptr(axes[1]), _ptr(axes[2]), nx, ny, nz, _ptr(brick_ijk) if n else None, n, first, count,
          _ptr(pts) if count else None)
    return pts


def mc_brick_classify(ub, brick_ijk, slot, dims, threshold):
    """-> (vert_count, tri_count int32 [n * 729], keys int64 [n * 729]: the dense linear index of every owned point, INT64_MAX
    elsewhere, leaks int32 [1]: (brick, face) pairs where the surface runs into a brick that is not in the list)."""
    n, nx, ny, nz = _mc_bricks(ub, brick_ijk, slot, dims)
    dev = brick_ijk.device
    vcount = torch.empty((n * BRICK_POINTS,), dtype=torch.int32, device=dev)
    tcount = torch.empty((n * BRICK_POINTS,), dtype=torch.int32, device=dev)
    keys = torch.empty((n * BRICK_POINTS,), dtype=torch.int64, device=dev)
    leaks = torch.empty((1,), dtype=torch.int32, device=dev)
    _call('vqn_mc_brick_classify', _ptr(ub) if n else None, _ptr(brick_ijk) if n else None, n, _ptr(slot), nx, ny, nz, float(threshold),
          _ptr(vcount) if n else None, _ptr(tcount) if n else None, _ptr(keys) if n else None, _ptr(leaks))
    return vcount, tcount, keys, leaks


def mc_brick_emit(ub, brick_ijk, slot, dims, threshold, vert_offset, tri_offset, n_verts, n_tris, origin=None, step=None, out=None):
    """The mesh from the offsets (int32 [n * 729]: exclusive prefix sums of mc_brick_classify's counts taken in the order of its keys)
    and their totals -> (verts [V,3] f32, tris [T,3] int32).  out = (verts, tris): write into these (at least that large) instead."""
    n, nx, ny, nz = _mc_bricks(ub, brick_ijk, slot, dims)
    for t in (vert_offset, tri_offset):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != ub.device or t.numel() != n * BRICK_POINTS:
            raise VqnError('mc_brick_emit: offsets must be contiguous int32 tensors on the device of ub, 729 entries per brick')
    if out is None:
        verts = torch.empty((n_verts, 3), dtype=torch.float32, device=ub.device)
        tris = torch.empty((n_tris, 3), dtype=torch.int32, device=ub.device)
    else:
        verts, tris = out
        if (verts.dtype != torch.float32 or tris.dtype != torch.int32 or not verts.is_contiguous() or not tris.is_contiguous()
                or verts.device != ub.device or tris.device != ub.device or verts.numel() < 3 * n_verts or tris.numel() < 3 * n_tris):
            raise VqnError('mc_brick_emit: out = (f32 verts, int32 tris), contiguous, on the device of ub, at least [n_verts, 3] / [n_tris, 3]')
    _call('vqn_mc_brick_emit', _ptr(ub) if n else None, _ptr(brick_ijk) if n else None, n, _ptr(slot), nx, ny, nz, float(threshold),
          _ptr(vert_offset) if n else None, _ptr(tri_offset) if n else None, n_verts, n_tris,
          None if origin is None else _host(origin, np.float32), None if step is None else _host(step, np.float32),
          _ptr(verts) if n_verts else None, _ptr(tris) if n_tris else None)
    return verts, tris


# --------------------------------------------------------------------------------------
# material codes on a mesh (csrc/mesh_materials.hip, include/vqn_mesh_materials.h; geo/mesh.py, decomp/material_mesh.py)
MESHMAT_MAX_CODES = 128            # codes at most (VQN_MESHMAT_MAX_CODES)
MESHMAT_FACES_PER_BLOCK = 512      # faces per row entry of block_count (VQN_MESHMAT_FACES_PER_BLOCK)
MESHMAT_WORD_BITS = 32             # vertices per word of the usage bitmap (VQN_MESHMAT_WORD_BITS)


def _mesh_codes(triangles, codes, what):
    """checks of (triangles [T,3], codes [V]) -> (T, V)"""
    T = _mesh_tris(triangles, what)
    if codes.dtype != torch.int32 or not codes.is_contiguous() or codes.device != triangles.device or codes.dim() != 1:
        raise VqnError(f'{what}: expected contiguous int32 codes [V] on the device of the triangles, got {codes.dtype} {tuple(codes.shape)} '
                       f'on {codes.device}')
    return T, codes.shape[0]


def mesh_label_mode(triangles, codes, n_codes, iters, self_weight):
    """`iters` >= 1 rounds of majority vote over the mesh (vqn_mesh_label_mode) -> (codes int32 [V], changed int32 [iters]), new tensors."""
    T, V = _mesh_codes(triangles, codes, 'mesh_label_mode')
    out = torch.empty_like(codes)
    changed = torch.empty((max(int(iters), 0),), dtype=torch.int32, device=codes.device)
    need = lib().vqn_mesh_label_scratch_bytes(T, V)
    buf = _scratch('mesh_label_mode', max(need, 64), codes.device)        # (need < 0: sizes the call itself refuses, with the reason)
    _call('vqn_mesh_label_mode', _ptr(triangles) if T else None, T, _ptr(codes) if V else None, V, int(n_codes), int(self_weight), int(iters),
          _ptr(out) if V else None, _ptr(changed) if changed.numel() else None, _ptr(buf), buf.numel())
    return out, changed


def mesh_split_shape(T, V):
    """-> (B, W): the face blocks and the bitmap words per code of a mesh of T triangles and V vertices"""
    return max(1, -(-T // MESHMAT_FACES_PER_BLOCK)), -(-V // MESHMAT_WORD_BITS)


def mesh_split_count(triangles, codes, n_codes):
    """-> (face_code int32 [T], block_count int32 [K, B], bitmap int32 [K, W] (the bits of a uint32), word_count int32 [K, W])."""
    T, V = _mesh_codes(triangles, codes, 'mesh_split_count')
    K = int(n_codes)
    B, W = mesh_split_shape(T, V)
    dev = triangles.device
    rows = min(max(K, 0), MESHMAT_MAX_CODES)                             # (a refused K: nothing is written, nothing large is allocated)
    face_code = torch.empty((T,), dtype=torch.int32, device=dev)
    block_count = torch.empty((rows, B), dtype=torch.int32, device=dev)
    bitmap = torch.empty((rows, W), dtype=torch.int32, device=dev)
    word_count = torch.empty((rows, W), dtype=torch.int32, device=dev)
    _call('vqn_mesh_split_count', _ptr(triangles) if T else None, T, _ptr(codes) if V else None, V, K, _ptr(face_code) if T else None,
          _ptr(block_count) if rows else None, _ptr(bitmap) if rows * W else None, _ptr(word_count) if rows * W else None)
    return face_code, block_count, bitmap, word_count


def mesh_split_emit(triangles, n_verts, n_codes, face_code, block_offset, bitmap, word_offset, n_faces, n_slots, out=None):
    """The split from the flat exclusive prefix sums of mesh_split_count's counts and their totals -> (face_src int32 [F],
    tris_local int32 [F, 3], vert_src int32 [S]).  out: these three, to be written in place."""
    T = _mesh_tris(triangles, 'mesh_split_emit')
    K, V = int(n_codes), int(n_verts)
    B, W = mesh_split_shape(T, V)
    for t, n in ((face_code, T), (block_offset, K * B), (bitmap, K * W), (word_offset, K * W)):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != triangles.device or t.numel() != n:
            raise VqnError('mesh_split_emit: face_code [T], block_offset [K, B], bitmap and word_offset [K, W]: contiguous int32 tensors on '
                           'the device of the triangles')
    if out is None:
        out = (torch.empty((n_faces,), dtype=torch.int32, device=triangles.device),
               torch.empty((n_faces, 3), dtype=torch.int32, device=triangles.device),
               torch.empty((n_slots,), dtype=torch.int32, device=triangles.device))
    face_src, tris_local, vert_src = out
    nul = lambda t: _ptr(t) if t.numel() else None
    _call('vqn_mesh_split_emit', nul(triangles), T, V, K, nul(face_code), nul(block_offset), nul(bitmap), nul(word_offset), int(n_faces),
          int(n_slots), nul(face_src), nul(tris_local), nul(vert_src))
    return face_src, tris_local, vert_src


# --------------------------------------------------------------------------------------
# mesh rasteriser (csrc/mesh_raster.hip, include/vqn_mesh_raster.h; geo/mesh_render.py)
RASTER_TILE = 16                   # pixels per side of a tile (VQN_RASTER_TILE)
RASTER_SUBPIXEL_BITS = 8           # screen coordinates snap to 1 / 256 pixel (VQN_RASTER_SUBPIXEL_BITS)
RASTER_MAX_SIDE = 8192             # H and W at most (VQN_RASTER_MAX_SIDE)
RASTER_COORD_LIMIT = 1 << 23       # |snapped coordinate| below this, in sub-pixel units (VQN_RASTER_COORD_LIMIT)
RASTER_CHUNK = 256                 # triangles staged in LDS at a time (VQN_RASTER_CHUNK)
RASTER_STATS = 4                   # counters of dropped triangles (VQN_RASTER_STATS)
RASTER_MAX_CHANNELS = 16           # attribute channels at most (VQN_RASTER_MAX_CHANNELS)
RASTER_STAT_NAMES = ('bad_index', 'unusable_vertex', 'zero_area', 'culled')


def raster_tiles(H, W):
    """-> (TY, TX): the tile grid of an H x W image"""
    return -(-int(H) // RASTER_TILE), -(-int(W) // RASTER_TILE)


def _raster_mesh(vertices, triangles, what):
    T = _mesh_tris(triangles, what)
    if vertices.dtype != torch.float32 or not vertices.is_contiguous() or vertices.device != triangles.device or vertices.dim() != 2 \
            or vertices.shape[1] != 3:
        raise VqnError(f'{what}: expected contiguous float32 vertices [V, 3] on the device of the triangles, got {vertices.dtype} '
                       f'{tuple(vertices.shape)} on {vertices.device}')
    return T, vertices.shape[0]


def _raster_side(H, W):
    """the sides an allocation is sized by: a refused H or W allocates for 1 (the call itself refuses, with the reason)"""
    ok = 1 <= int(H) <= RASTER_MAX_SIDE and 1 <= int(W) <= RASTER_MAX_SIDE
    return (int(H), int(W)) if ok else (1, 1)


def raster_count(vertices, triangles, P, H, W, near, cull, out=None):
    """vqn_raster_count -> (pverts int32 [V, 3], tile_count int32 [TY * TX], stats int32 [RASTER_STATS]).  P: host floats [3, 4].
    out: these three, to be written in place."""
    T, V = _raster_mesh(vertices, triangles, 'raster_count')
    P = np.ascontiguousarray(P, dtype=np.float32)
    if P.shape != (3, 4):
        raise VqnError(f'raster_count: P is a host array [3, 4], got {P.shape}')
    if out is None:
        ty, tx = raster_tiles(*_raster_side(H, W))
        dev = triangles.device
        out = (torch.empty((V, 3), dtype=torch.int32, device=dev), torch.empty((ty * tx,), dtype=torch.int32, device=dev),
               torch.empty((RASTER_STATS,), dtype=torch.int32, device=dev))
    pverts, tile_count, stats = out
    _call('vqn_raster_count', _ptr(vertices) if V else None, V, _ptr(triangles) if T else None, T, P.ctypes.data, int(H), int(W), float(near),
          int(cull), _ptr(pverts) if V else None, _ptr(tile_count), _ptr(stats))
    return pverts, tile_count, stats


def raster_resolve(triangles, pverts, H, W, cull, tile_offset, n_pairs, out=None):
    """vqn_raster_resolve from the exclusive prefix sum of raster_count's tile_count and its total -> (face int32 [H, W], depth f32
    [H, W], bary f32 [H, W, 3]).  out = (cursor int32 [TY * TX], bin int32 [n_pairs], face, depth, bary): write into these."""
    T = _mesh_tris(triangles, 'raster_resolve')
    V = pverts.shape[0]
    dev = triangles.device
    if out is None:
        h, w = _raster_side(H, W)
        ty, tx = raster_tiles(h, w)
        out = (torch.empty((ty * tx,), dtype=torch.int32, device=dev), torch.empty((max(int(n_pairs), 0),), dtype=torch.int32, device=dev),
               torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev),
               torch.empty((h, w, 3), dtype=torch.float32, device=dev))
    cursor, bin_, face, depth, bary = out
    for t, dt in ((pverts, torch.int32), (tile_offset, torch.int32), (cursor, torch.int32), (bin_, torch.int32), (face, torch.int32),
                  (depth, torch.float32), (bary, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise VqnError('raster_resolve: pverts, tile_offset, cursor, bin and face are contiguous int32 tensors, depth and bary float32, on '
                           'the device of the triangles')
    _call('vqn_raster_resolve', _ptr(triangles) if T else None, T, _ptr(pverts) if V else None, V, int(H), int(W), int(cull), _ptr(tile_offset),
          int(n_pairs), _ptr(cursor), _ptr(bin_) if bin_.numel() else None, _ptr(face), _ptr(depth), _ptr(bary))
    return face, depth, bary


def raster_interpolate(face, bary, triangles, attr, background, nearest=False, out=None):
    """vqn_raster_interpolate: attr f32 [V, C] over (face [H, W], bary [H, W, 3]) -> f32 [H, W, C]; background f32 [C] (device)."""
    T = _mesh_tris(triangles, 'raster_interpolate')
    dev = triangles.device
    H, W = face.shape
    if attr.dim() != 2 or background.dim() != 1 or background.shape[0] != attr.shape[1]:
        raise VqnError(f'raster_interpolate: attr [V, C] and background [C], got {tuple(attr.shape)} and {tuple(background.shape)}')
    V, C = attr.shape
    if out is None:
        out = torch.empty((H, W, C if 1 <= C <= RASTER_MAX_CHANNELS else 1), dtype=torch.float32, device=dev)
    for t, dt in ((face, torch.int32), (bary, torch.float32), (attr, torch.float32), (background, torch.float32), (out, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise VqnError('raster_interpolate: face is a contiguous int32 tensor, bary, attr, background and out float32, on the device of the '
                           'triangles')
    if bary.numel() != 3 * H * W:
        raise VqnError(f'raster_interpolate: bary is [H, W, 3] of face [H, W], got {tuple(bary.shape)} and {tuple(face.shape)}')
    _call('vqn_raster_interpolate', _ptr(face), _ptr(bary), H, W, _ptr(triangles) if T else None, T, _ptr(attr) if V else None, V, C,
          _ptr(background) if C else None, int(bool(nearest)), _ptr(out))
    return out


# --------------------------------------------------------------------------------------
# mesh ray caster (csrc/mesh_rays.hip, include/vqn_mesh_rays.h; geo/mesh_rays.py)
RAYS_MAX_AXIS = 1024               # cells per axis at most (VQN_RAYS_MAX_AXIS)
RAYS_MAX_CELLS = 1 << 24           # cells at most (VQN_RAYS_MAX_CELLS)
RAYS_STATS = 3                     # counters of dropped triangles (VQN_RAYS_STATS)
RAYS_MARGIN_INV = 16               # a triangle's box is widened by 1 / 16 cell before it is binned (VQN_RAYS_MARGIN_INV)
RAYS_PACKED_FLOATS = 12            # floats of a packed triangle (VQN_RAYS_PACKED_FLOATS)
RAYS_MAX_LIGHTS = 65536            # lights of rays_light_visibility at most (VQN_RAYS_MAX_LIGHTS)
RAYS_TILE = 64                     # points x lights of the staged tile (VQN_RAYS_TILE)
RAYS_MIN_DIR_LOG2 = -60            # a ray is cast only if max |d component| >= 2^-60 (VQN_RAYS_MIN_DIR_LOG2)
RAYS_LANES_POINTS = 0              # a wave holds 64 neighbouring points of one light (VQN_RAYS_LANES_POINTS)
RAYS_LANES_LIGHTS = 1              # a wave holds 64 lights of one point (VQN_RAYS_LANES_LIGHTS)
RAYS_STAT_NAMES = ('bad_index', 'nonfinite_vertex', 'zero_area')


def rays_grid_plan(lo, hi, n_tris, cell=None):
    """The grid over a mesh of n_tris triangles whose finite vertices have the bounding box lo .. hi (three floats each; host only)
    -> GeomGrid.  cell: its size, None for the default.  A plan the library refuses raises ValueError with its reason."""
    grid = GeomGrid()
    lo, hi = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(hi, dtype=np.float32)
    if lo.shape != (3,) or hi.shape != (3,):
        raise VqnError(f'rays_grid_plan: lo and hi are three floats each, got {lo.shape} and {hi.shape}')
    rc = lib().vqn_rays_grid_plan(lo.ctypes.data, hi.ctypes.data, int(n_tris), 0.0 if cell is None else float(cell), ctypes.addressof(grid))
    if rc != 0:
        raise ValueError(lib().vqn_last_error().decode())
    return grid


def _rays_cells(grid):
    """the cells an allocation is sized by: a grid the call itself refuses allocates for 1"""
    d = [int(x) for x in grid.dims]
    ok = all(1 <= x <= RAYS_MAX_AXIS for x in d) and d[0] * d[1] * d[2] == int(grid.cells) <= RAYS_MAX_CELLS
    return int(grid.cells) if ok else 1


def _rays_tensors(what, dev, i32=(), f32=(), u8=()):
    for ts, dt in ((i32, torch.int32), (f32, torch.float32), (u8, torch.uint8)):
        for t in ts:
            if t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise VqnError(f'{what}: expected a contiguous {dt} tensor on {dev}, got {t.dtype} contiguous={t.is_contiguous()} on {t.device}')


def rays_count(vertices, triangles, grid, out=None):
    """vqn_rays_count -> (cell_count int32 [cells], stats int32 [RAYS_STATS]).  out: these two, to be written in place."""
    T, V = _raster_mesh(vertices, triangles, 'rays_count')
    dev = triangles.device
    if out is None:
        out = (torch.empty((_rays_cells(grid),), dtype=torch.int32, device=dev), torch.empty((RAYS_STATS,), dtype=torch.int32, device=dev))
    cell_count, stats = out
    _rays_tensors('rays_count', dev, i32=(cell_count, stats))
    _call('vqn_rays_count', _ptr(vertices) if V else None, V, _ptr(triangles) if T else None, T, ctypes.addressof(grid), _ptr(cell_count),
          _ptr(stats))
    return cell_count, stats


def rays_bin(vertices, triangles, grid, cell_offset, n_pairs, out=None):
    """vqn_rays_bin from the exclusive prefix sum of rays_count's cell_count and its total -> (bin int32 [n_pairs], packed f32
    [T, RAYS_PACKED_FLOATS]).  out = (cursor int32 [cells], bin, packed): write into these."""
    T, V = _raster_mesh(vertices, triangles, 'rays_bin')
    dev = triangles.device
    if out is None:
        out = (torch.empty((_rays_cells(grid),), dtype=torch.int32, device=dev), torch.empty((max(int(n_pairs), 0),), dtype=torch.int32, device=dev),
               torch.empty((T, RAYS_PACKED_FLOATS), dtype=torch.float32, device=dev))
    cursor, bin_, packed = out
    _rays_tensors('rays_bin', dev, i32=(cell_offset, cursor, bin_), f32=(packed,))
    _call('vqn_rays_bin', _ptr(vertices) if V else None, V, _ptr(triangles) if T else None, T, ctypes.addressof(grid), _ptr(cell_offset),
          int(n_pairs), _ptr(cursor), _ptr(bin_) if bin_.numel() else None, _ptr(packed) if T else None)
    return bin_, packed


def _rays_scene(what, packed, grid, cell_offset, n_pairs, bin_):
    """checks of a built grid -> its leading arguments"""
    if packed.dim() != 2 or packed.shape[1] != RAYS_PACKED_FLOATS or not packed.is_cuda:
        raise VqnError(f'{what}: packed is a device tensor [T, {RAYS_PACKED_FLOATS}], got {tuple(packed.shape)} on {packed.device}')
    _rays_tensors(what, packed.device, i32=(cell_offset, bin_), f32=(packed,))
    T = packed.shape[0]
    return (_ptr(packed) if T else None, T, ctypes.addressof(grid), _ptr(cell_offset), int(n_pairs), _ptr(bin_) if bin_.numel() else None)


def _rays_rays(what, dev, o, d, tmin, tmax):
    _rays_tensors(what, dev, f32=(o, d, tmin, tmax))
    n = tmin.numel()
    if o.dim() != 2 or o.shape != (n, 3) or d.shape != (n, 3) or tmax.numel() != n:
        raise VqnError(f'{what}: o, d [n, 3] and tmin, tmax [n], got {tuple(o.shape)}, {tuple(d.shape)}, {tuple(tmin.shape)}, {tuple(tmax.shape)}')
    return n


def rays_cast(packed, grid, cell_offset, n_pairs, bin_, o, d, tmin, tmax, out=None):
    """vqn_rays_cast -> (face int32 [n], t f32 [n], uv f32 [n, 2]).  out: these three, to be written in place."""
    scene = _rays_scene('rays_cast', packed, grid, cell_offset, n_pairs, bin_)
    dev = packed.device
    n = _rays_rays('rays_cast', dev, o, d, tmin, tmax)
    if out is None:
        out = (torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev),
               torch.empty((n, 2), dtype=torch.float32, device=dev))
    face, t, uv = out
    _rays_tensors('rays_cast', dev, i32=(face,), f32=(t, uv))
    nul = lambda x: _ptr(x) if n else None
    _call('vqn_rays_cast', *scene, nul(o), nul(d), nul(tmin), nul(tmax), n, nul(face), nul(t), nul(uv))
    return face, t, uv


def rays_occluded(packed, grid, cell_offset, n_pairs, bin_, o, d, tmin, tmax, out=None):
    """vqn_rays_occluded -> uint8 [n]"""
    scene = _rays_scene('rays_occluded', packed, grid, cell_offset, n_pairs, bin_)
    dev = packed.device
    n = _rays_rays('rays_occluded', dev, o, d, tmin, tmax)
    if out is None:
        out = torch.empty((n,), dtype=torch.uint8, device=dev)
    _rays_tensors('rays_occluded', dev, u8=(out,))
    nul = lambda x: _ptr(x) if n else None
    _call('vqn_rays_occluded', *scene, nul(o), nul(d), nul(tmin), nul(tmax), n, nul(out))
    return out


def rays_light_visibility(packed, grid, cell_offset, n_pairs, bin_, points, normals, lights, bias, lanes=RAYS_LANES_POINTS, out=None):
    """vqn_rays_light_visibility: points, normals f32 [n, 3], lights f32 [L, 3] -> f32 [n, L]"""
    scene = _rays_scene('rays_light_visibility', packed, grid, cell_offset, n_pairs, bin_)
    dev = packed.device
    _rays_tensors('rays_light_visibility', dev, f32=(points, normals, lights))
    if points.dim() != 2 or points.shape[1] != 3 or normals.shape != points.shape or lights.dim() != 2 or lights.shape[1] != 3:
        raise VqnError(f'rays_light_visibility: points, normals [n, 3] and lights [L, 3], got {tuple(points.shape)}, {tuple(normals.shape)}, '
                       f'{tuple(lights.shape)}')
    n, L = points.shape[0], lights.shape[0]
    if out is None:
        out = torch.empty((n, L if 1 <= L <= RAYS_MAX_LIGHTS else 1), dtype=torch.float32, device=dev)
    _rays_tensors('rays_light_visibility', dev, f32=(out,))
    nul = lambda x: _ptr(x) if n else None
    _call('vqn_rays_light_visibility', *scene, nul(points), nul(normals), n, _ptr(lights) if L else None, L, float(bias), int(lanes), nul(out))
    return out


# --------------------------------------------------------------------------------------
# image metrics (csrc/image_metrics.hip, include/vqn_eval.h; decomp/nerfactor/util/metric.py)
IMAGE_METRICS_WINDOW = 11      # weights of the SSIM window (VQN_IMAGE_METRICS_WINDOW)
IMAGE_METRICS_OUT_WORDS = 16   # 8-byte words of the output per image pair (VQN_IMAGE_METRICS_OUT_WORDS)


def image_metrics(a, b, window, alpha=None, alpha_thres=0.0):
    """a, b [B,H,W,C] contiguous device tensors, both uint8 or both float32 (rows in [0, 1], quantised by the kernel), C in {1, 3};
    window: the 11 normalised weights (host doubles); alpha: float32 [H,W] (one plane for all pairs) or [B,H,W], pixels that are
    not alpha > alpha_thres turn white -> int64 [B, 16], the words of vqn_image_metrics_u8's `out` (view the first ten as float64).
    Two launches, no host read."""
    if a.dtype != b.dtype or a.dtype not in (torch.uint8, torch.float32) or a.shape != b.shape or a.dim() != 4 or a.device != b.device \
            or not (a.is_cuda and a.is_contiguous() and b.is_contiguous()):
        raise VqnError(f'image_metrics: expected two contiguous device tensors [B, H, W, C] of one shape, uint8 or float32, got '
                       f'{a.dtype} {tuple(a.shape)} on {a.device} and {b.dtype} {tuple(b.shape)} on {b.device}')
    B, H, W, C = (int(s) for s in a.shape)
    stride = 0
    if alpha is not None:
        _f32c(alpha, 'alpha')
        if alpha.device != a.device or tuple(alpha.shape) not in ((H, W), (B, H, W)):
            raise VqnError(f'image_metrics: alpha must be [H, W] or [B, H, W] on the device of the images, got {tuple(alpha.shape)}')
        stride = H * W if alpha.dim() == 3 else 0
    out = torch.empty((B, IMAGE_METRICS_OUT_WORDS), dtype=torch.int64, device=a.device)
    entry = 'vqn_image_metrics_u8' if a.dtype == torch.uint8 else 'vqn_image_metrics_f32'
    need = lib().vqn_image_metrics_scratch_bytes(B, H, W)
    buf = _scratch('image_metrics', max(need, 64), a.device)           # (need = 0: a shape the call itself refuses, with the reason)
    _call(entry, _ptr(a), _ptr(b), _ptr(alpha), stride, float(alpha_thres), B, H, W, C, _host(window, np.float64), _ptr(buf), buf.numel(),
          _ptr(out))
    return out


# --------------------------------------------------------------------------------------
# segmentation scores (csrc/segmentation_metrics.hip, include/vqn_eval.h; decomp/nerfactor/util/segmentation.py)
SEG_PIXELS_PER_PASS = 4096     # pixels a workgroup takes per pass (VQN_SEG_PIXELS_PER_PASS)
SEG_GRID_CAP = 512             # workgroups at most (VQN_SEG_GRID_CAP)
SEG_MAX_SIDE = 65              # table sides R = n_gt + 1, C = n_pd + 1 at most (VQN_SEG_MAX_SIDE)
SEG_HEAD_WORDS = 42            # 8-byte words of the output row ahead of the table (VQN_SEG_HEAD_WORDS)


def segmentation_counts(gt, pd, sel=None, alpha_thres=0.0, gt_palette=None, pd_palette=None, n_gt=None, n_pd=None):
    """Contingency table and clustering scores of n pixels, two launches, no host read.
    Colour form: gt, pd uint8 [n, 3] contiguous device tensors, gt_palette [n_gt, 3] and pd_palette [n_pd, 3] host uint8 arrays,
    sel = alpha float32 [n] or None (counted: alpha > alpha_thres, strict).  Label form: gt, pd int32 [n], n_gt and n_pd the largest
    labels, sel = mask uint8 [n] or None (counted: mask != 0).
    -> int64 [42 + R * C], the words of vqn_seg_contingency_rgb's `out` (include/vqn_eval.h)."""
    colour = gt.dtype == torch.uint8
    want = 2 if colour else 1
    if gt.dtype != pd.dtype or gt.dtype not in (torch.uint8, torch.int32) or gt.shape != pd.shape or gt.dim() != want \
            or (colour and gt.shape[-1] != 3) or gt.device != pd.device or not (gt.is_cuda and gt.is_contiguous() and pd.is_contiguous()):
        raise VqnError(f'segmentation_counts: expected two contiguous device tensors of one shape, uint8 [n, 3] or int32 [n], got '
                       f'{gt.dtype} {tuple(gt.shape)} on {gt.device} and {pd.dtype} {tuple(pd.shape)} on {pd.device}')
    n = int(gt.shape[0])
    if sel is not None:
        sel_dtype = torch.float32 if colour else torch.uint8
        if sel.dtype != sel_dtype or tuple(sel.shape) != (n,) or sel.device != gt.device or not sel.is_contiguous():
            raise VqnError(f'segmentation_counts: expected {"alpha float32" if colour else "mask uint8"} [{n}] contiguous on the device of '
                           f'the labels, got {sel.dtype} {tuple(sel.shape)} on {sel.device}')
    if colour:
        pals = [np.ascontiguousarray(p, dtype=np.uint8) for p in (gt_palette, pd_palette)]
        if any(p.ndim != 2 or p.shape[1] != 3 for p in pals):
            raise VqnError(f'segmentation_counts: palettes must be uint8 [rows, 3], got {pals[0].shape} and {pals[1].shape}')
        n_gt, n_pd = int(pals[0].shape[0]), int(pals[1].shape[0])
    elif n_gt is None or n_pd is None:
        raise VqnError('segmentation_counts: the label form needs n_gt and n_pd, the largest labels')
    n_gt, n_pd = int(n_gt), int(n_pd)
    R, C = n_gt + 1, n_pd + 1
    cells = R * C if 1 <= R <= SEG_MAX_SIDE and 1 <= C <= SEG_MAX_SIDE else 0
    out = torch.empty((SEG_HEAD_WORDS + cells,), dtype=torch.int64, device=gt.device)
    need = lib().vqn_seg_scratch_bytes(n, R, C)
    buf = _scratch('segmentation_metrics', max(need, 64), gt.device)    # (need = 0: a shape the call itself refuses, with the reason)
    if colour:
        _call('vqn_seg_contingency_rgb', _ptr(gt), _ptr(pd), _ptr(sel), float(alpha_thres), n, pals[0].ctypes.data, n_gt, pals[1].ctypes.data,
              n_pd, _ptr(buf), buf.numel(), _ptr(out))
    else:
        _call('vqn_seg_contingency_labels', _ptr(gt), _ptr(pd), _ptr(sel), n, n_gt, n_pd, _ptr(buf), buf.numel(), _ptr(out))
    return out


# --------------------------------------------------------------------------------------
# material selection and editing (csrc/material_edit.hip, include/vqn_material_edit.h; decomp/nerfactor/util/material_edit.py)
MATEDIT_ROWS_PER_PASS = 1024   # rows a workgroup takes per pass (VQN_MATEDIT_ROWS_PER_PASS)
MATEDIT_GRID_CAP = 1024        # workgroups at most (VQN_MATEDIT_GRID_CAP)
MATEDIT_MAX_PLANES = 8         # property planes at most, of 1 .. 3 channels each (VQN_MATEDIT_MAX_PLANES)
MATEDIT_MAX_TERMS = 32         # terms of a program at most (VQN_MATEDIT_MAX_TERMS)
MATEDIT_MAX_CONDS = 8          # conditions of a program at most (VQN_MATEDIT_MAX_CONDS)
MATEDIT_HEAD_WORDS = 3         # words of the counts row ahead of the 65 per-code counts: selected, rows, invalid (VQN_MATEDIT_HEAD_WORDS)
MATEDIT_CODES = 65             # code labels 0 .. 64 (VQN_MATEDIT_CODES)


def _overlap(a, b):
    """do the bytes of two tensors overlap (views of one storage that do not touch are fine)"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a.numel() > 0 and b.numel() > 0 and a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def material_select_edit(n, planes=(), embed=None, mask_in=None, terms=(), ops=(), n_conds=0, codes=None, eps=5e-6, edit=None, dst=None,
                         opt_scale=None, out=None, want_mask=True, device=None):
    """Selection, material edit, opt_scale scaling and counts of n rows in ONE launch (include/vqn_material_edit.h), no host read.
    planes: up to 8 float32 [n, ch] (ch <= 3) contiguous device tensors or None; embed: int32 [n] or float32 [n] or None; mask_in:
    uint8 [n] or None.  terms: rows (plane, channel, denominator channel or -1, lo, hi, condition id); ops: 0 'and' / 1 'or', one
    fewer than n_conds; codes: the labels of the set (each in 0 .. 64) or None.  edit = (albedo [n, 3], spec [n, 3], rough [n, 1])
    with dst = 7 floats diff[3], spec[3], rough[1] and opt_scale = 3 floats or None; `out`: the output tensors to write (default:
    new ones), in the order of the result.
    -> (mask uint8 [n] or None, counts int64 [68] = selected, n, invalid, per code [65], edited: None or (albedo', spec', rough') or
    (albedo', spec', rough', albedo' * opt_scale, spec' * opt_scale)).
    Inputs need not be 16-byte aligned (the kernel then goes row by row) but must be contiguous; outputs may not overlap inputs."""
    n = int(n)
    planes = list(planes) + [None] * (MATEDIT_MAX_PLANES - len(planes))
    if len(planes) > MATEDIT_MAX_PLANES:
        raise VqnError(f'material_select_edit: at most {MATEDIT_MAX_PLANES} planes, got {len(planes)}')
    given = [t for t in planes if t is not None] + [t for t in (embed, mask_in) if t is not None] + list(edit or ())
    dev = given[0].device if given else torch.device(device or 'cuda')
    plane_ch = np.zeros(MATEDIT_MAX_PLANES, np.int32)
    for p, t in enumerate(planes):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != n or not t.is_cuda or not t.is_contiguous() or t.device != dev:
            raise VqnError(f'material_select_edit: plane {p}: expected a contiguous float32 [{n}, ch] tensor on {dev}, got {t.dtype} '
                           f'{tuple(t.shape)} contiguous={t.is_contiguous()} on {t.device}')
        plane_ch[p] = t.shape[1]
    if embed is not None and (embed.dtype not in (torch.int32, torch.float32) or tuple(embed.shape) != (n,) or embed.device != dev
                              or not embed.is_contiguous()):
        raise VqnError(f'material_select_edit: embed: expected a contiguous int32 or float32 [{n}] tensor on {dev}, got {embed.dtype} '
                       f'{tuple(embed.shape)} on {embed.device}')
    if mask_in is not None and (mask_in.dtype != torch.uint8 or tuple(mask_in.shape) != (n,) or mask_in.device != dev or not mask_in.is_contiguous()):
        raise VqnError(f'material_select_edit: mask_in: expected a contiguous uint8 [{n}] tensor on {dev}, got {mask_in.dtype} '
                       f'{tuple(mask_in.shape)} on {mask_in.device}')
    shapes = [(n, 3), (n, 3), (n, 1)]
    if edit is not None:
        if dst is None or len(edit) != 3:
            raise VqnError('material_select_edit: an edit needs (albedo, spec, rough) and dst')
        for t, shp in zip(edit, shapes):
            if t.dtype != torch.float32 or tuple(t.shape) != shp or t.device != dev or not t.is_contiguous():
                raise VqnError(f'material_select_edit: edit inputs are contiguous float32 [n, 3], [n, 3], [n, 1] on {dev}, got {t.dtype} '
                               f'{tuple(t.shape)} on {t.device}')
        if opt_scale is not None:
            shapes = shapes + [(n, 3), (n, 3)]
    outs = []
    if edit is not None:
        outs = list(out) if out is not None else [torch.empty(shp, dtype=torch.float32, device=dev) for shp in shapes]
        if len(outs) != len(shapes) or any(o.dtype != torch.float32 or tuple(o.shape) != shp or o.device != dev or not o.is_contiguous()
                                           for o, shp in zip(outs, shapes)):
            raise VqnError(f'material_select_edit: outputs are contiguous float32 tensors of shapes {shapes} on {dev}')
    mask_out = torch.empty((n,), dtype=torch.uint8, device=dev) if want_mask else None
    written = outs + ([mask_out] if mask_out is not None else [])
    for i, o in enumerate(written):
        if any(_overlap(o, t) for t in given) or any(_overlap(o, w) for w in written[:i]):
            raise VqnError('material_select_edit: an output aliases an input (or another output); the selection reads the pre-edit values')
    terms = list(terms)
    ti = np.ascontiguousarray([[t[0], t[1], t[2], t[5]] for t in terms], dtype=np.int32).reshape(-1, 4)
    tf = np.ascontiguousarray([[t[3], t[4]] for t in terms], dtype=np.float32).reshape(-1, 2)
    ops_h = np.ascontiguousarray(list(ops), dtype=np.int32)
    if len(ops_h) != max(int(n_conds) - 1, 0):
        raise VqnError(f'material_select_edit: {n_conds} conditions take {max(int(n_conds) - 1, 0)} ops, got {len(ops_h)}')
    codes_h = None
    if codes is not None:
        codes_h = np.zeros(MATEDIT_CODES, np.uint8)
        for c in codes:
            if not 0 <= int(c) < MATEDIT_CODES:
                raise VqnError(f'material_select_edit: code labels are 0 .. {MATEDIT_CODES - 1}, got {c}')
            codes_h[int(c)] = 1
    dst_h = None if dst is None else np.ascontiguousarray(dst, dtype=np.float32).reshape(-1)
    if dst_h is not None and dst_h.size != 7:
        raise VqnError(f'material_select_edit: dst is 7 floats diff[3], spec[3], rough[1], got {dst_h.size}')
    scale_h = None if opt_scale is None else np.ascontiguousarray(
        opt_scale.detach().cpu().numpy() if torch.is_tensor(opt_scale) else opt_scale, dtype=np.float32).reshape(-1)
    if scale_h is not None and scale_h.size != 3:
        raise VqnError(f'material_select_edit: opt_scale is 3 floats, got {scale_h.size}')
    nul = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    e = list(edit) if edit is not None else [None] * 3
    o = outs + [None] * (5 - len(outs))
    if n == 0 and len(terms) <= MATEDIT_MAX_TERMS and int(n_conds) <= MATEDIT_MAX_CONDS:
        # nothing to launch: the counts of no rows (the refusals below still come from the library when a limit is exceeded)
        return mask_out, torch.zeros((MATEDIT_HEAD_WORDS + MATEDIT_CODES,), dtype=torch.int64, device=dev), (tuple(outs) if edit is not None else None)
    counts = torch.empty((MATEDIT_HEAD_WORDS + MATEDIT_CODES,), dtype=torch.int64, device=dev)
    _call('vqn_material_select_edit', _ptrs(planes, MATEDIT_MAX_PLANES), plane_ch.ctypes.data, _ptr(embed),
          int(embed is not None and embed.dtype == torch.float32), _ptr(mask_in), n, nul(ti), nul(tf), len(terms), nul(ops_h), int(n_conds),
          nul(codes_h), float(eps), _ptr(e[0]), _ptr(e[1]), _ptr(e[2]), nul(dst_h), nul(scale_h), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]),
          _ptr(o[4]), _ptr(mask_out), _ptr(counts))
    return mask_out, counts, (tuple(outs) if edit is not None else None)


# --------------------------------------------------------------------------------------
# material balls (csrc/material_balls.hip, include/vqn_material_balls.h; decomp/nerfactor/util/material_balls.py)
MATBALLS_MAX_MATERIALS = 65        # materials at most (VQN_MATBALLS_MAX_MATERIALS)
MATBALLS_MAX_PROBES = 24           # probes at most (VQN_MATBALLS_MAX_PROBES)
MATBALLS_SCRATCH_PER_LIGHT = 288   # bytes of scratch per light that always suffice (VQN_MATBALLS_SCRATCH_PER_LIGHT)
MATBALLS_MAX_OUT_BYTES = 2 ** 31 - 1   # bytes of an output buffer at most (VQN_MATBALLS_MAX_OUT_BYTES)


def material_balls(materials, lights, lxyz, areas, ims, spp, sphere_radius=0.4, cam_rot=None, white_bg=True, gamma=None,
                   want_f32=True, want_u8=False, sheet=None, out=None):
    """materials float32 [M, 7] = albedo[3], f0[3], rough[1]; lights [P, L, 3]; lxyz [L, 3]; areas [L]: contiguous device tensors.
    cam_rot: 9 host floats or None (the default camera); gamma: 2 host floats or None.  sheet: None or (order, rows, cols), order a
    host list of distinct material indices or None (0 .. M - 1).  out: None or (f32, u8, sheet) tensors to write into (None entries are
    not written), which replaces want_f32 / want_u8 / sheet's allocation -- the refusal tests hand in canary-filled buffers.
    -> dict(f32 [M, P, ims, ims, 3] | None, u8 uint8 [M, P, ims, ims, 3] | None, sheet uint8 [P, rows ims, cols ims, 3] | None)."""
    for n_, t in (('materials', materials), ('lights', lights), ('lxyz', lxyz), ('areas', areas)):
        _f32c(t, n_)
    M, dev = materials.shape[0], materials.device
    P, L = (lights.shape[0], lights.shape[1]) if lights.dim() == 3 else (0, 0)
    if materials.dim() != 2 or materials.shape[1] != 7 or lights.dim() != 3 or lights.shape[2] != 3 or lxyz.numel() != 3 * L or areas.numel() != L:
        raise VqnError(f'material_balls: expected materials [M, 7], lights [P, L, 3], lxyz [L, 3], areas [L], got {tuple(materials.shape)}, '
                       f'{tuple(lights.shape)}, {tuple(lxyz.shape)}, {tuple(areas.shape)}')
    ims, spp = int(ims), int(spp)
    order, rows, cols = sheet if sheet is not None else (None, 0, 0)
    order_h = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    rot_h = None if cam_rot is None else np.ascontiguousarray(cam_rot, dtype=np.float32).reshape(-1)
    gam_h = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float32).reshape(-1)
    if (rot_h is not None and rot_h.size != 9) or (gam_h is not None and gam_h.size != 2):
        raise VqnError('material_balls: cam_rot is 9 floats and gamma 2')
    if out is not None:
        f32, u8, sh = out
    else:
        shapes = [(M, P, ims, ims, 3) if want_f32 else None, (M, P, ims, ims, 3) if want_u8 else None,
                  (P, int(rows) * ims, int(cols) * ims, 3) if sheet is not None else None]
        if any(s is not None and (min(s) < 0 or int(np.prod(s, dtype=np.float64)) * (4 if i == 0 else 1) > MATBALLS_MAX_OUT_BYTES)
               for i, s in enumerate(shapes)):
            raise VqnError(f'material_balls: an output of {M} x {P} images of {ims} x {ims} pixels (sheet {rows} x {cols}) exceeds '
                           f'{MATBALLS_MAX_OUT_BYTES} bytes')
        f32, u8, sh = [None if s is None else torch.empty(s, dtype=torch.float32 if i == 0 else torch.uint8, device=dev)
                       for i, s in enumerate(shapes)]
    need = MATBALLS_SCRATCH_PER_LIGHT * max(L, 1)
    scratch = _scratch('material_balls', need, dev)
    nul = lambda a: None if a is None else a.ctypes.data
    _call('vqn_material_balls', _ptr(materials), M, _ptr(lights), P, _ptr(lxyz), _ptr(areas), L, ims, spp, float(sphere_radius), nul(rot_h),
          int(bool(white_bg)), nul(gam_h), _ptr(f32), _ptr(u8), _ptr(sh), nul(order_h), 0 if order_h is None else int(order_h.size),
          int(rows), int(cols), _ptr(scratch), need)
    return dict(f32=f32, u8=u8, sheet=sh)


# --------------------------------------------------------------------------------------
# mean-shift clustering (csrc/meanshift.hip, include/vqn_eval.h; decomp/nerfactor/util/meanshift.py)
MEANSHIFT_MAX_DIM = 8              # features per point at most (VQN_MEANSHIFT_MAX_DIM)
MEANSHIFT_POINTS_PER_TILE = 256    # points the seek kernel stages in LDS per pass (VQN_MEANSHIFT_POINTS_PER_TILE)
MEANSHIFT_SEEDS_PER_GROUP = 64     # seeds a seek workgroup owns (VQN_MEANSHIFT_SEEDS_PER_GROUP)
MEANSHIFT_ASSIGN_SPAN = 256        # points an assign workgroup labels per pass (VQN_MEANSHIFT_ASSIGN_SPAN)
MEANSHIFT_ASSIGN_CENTRES = 512     # centres the assign kernel holds in LDS at a time (VQN_MEANSHIFT_ASSIGN_CENTRES)


# --------------------------------------------------------------------------------------
# baseline JPEG of device frames (csrc/jpeg_encode.hip, csrc/jpeg_plan.h, include/vqn_image_codec.h; decomp/nerfactor/util/mjpeg.py)
JPEG_HEADER_CAP = 1024             # bytes a header never reaches (VQN_JPEG_HEADER_CAP)
# the fields of struct VqnJpegGeom, in order
JPEG_GEOM = ('n', 'h', 'w', 'quality', 'sub', 'ri', 'mcu', 'mcus_x', 'mcus_y', 'blocks_per_mcu', 'intervals', 'slot_bytes', 'by_y', 'bx_y',
             'by_c', 'bx_c', 'off_cb', 'off_cr', 'off_slots', 'off_lens', 'off_dst', 'scratch_bytes', 'out_bytes', 'header_bytes')


def _codec_plan(entry, fields, head_cap, *args):
    """jpeg_plan / png_plan: the planner `entry` over *args -> ({name: int} over `fields`, its head_cap bytes of a file's front)"""
    geom = np.zeros(len(fields), np.int64)
    head = np.zeros(head_cap, np.uint8)
    rc = getattr(lib(), entry)(*(int(a) for a in args), geom.ctypes.data, head.ctypes.data, head.size)
    if rc != 0:
        raise ValueError(lib().vqn_last_error().decode())
    return {k: int(v) for k, v in zip(fields, geom)}, head


def _codec_encode(name, fields, x, last, g, scratch, out, meta):
    """jpeg_encode / png_encode: vqn_<name> on x with the planner's arguments (the first six of `fields`) out of the plan g"""
    want = (g['n'], g['h'], g['w'], last)
    if x.dtype != torch.uint8 or tuple(x.shape) != want or not x.is_contiguous():
        raise VqnError(f'{name}: expected a contiguous uint8 {list(want)} tensor, got {x.dtype} '
                       f'{tuple(x.shape)} contiguous={x.is_contiguous()}')
    require_device(x, name)
    only = out is None
    _call('vqn_' + name, _ptr(x), *[g[k] for k in fields[:6]], _ptr(scratch), scratch.numel(), _ptr(out), 0 if only else out.numel(),
          _ptr(meta), int(only))


def jpeg_plan(n, h, w, quality, subsampling, restart_interval):
    """The planner's view of a batch (host only): ({name: int} over JPEG_GEOM, the header bytes SOI .. SOS).  subsampling 420 or 444.
    A batch it refuses raises ValueError with its reason."""
    g, header = _codec_plan('vqn_jpeg_plan', JPEG_GEOM, JPEG_HEADER_CAP, n, h, w, quality, subsampling, restart_interval)
    return g, header[:g['header_bytes']].tobytes()


def jpeg_encode(frames, g, scratch, out=None, meta=None):
    """frames uint8 [n, h, w, 3] contiguous device tensor, g the plan of its batch, scratch a uint8 device buffer of g['scratch_bytes']
    (g['off_slots'] when out is None: the coefficients only).  Fills scratch (the coefficient planes first), out and meta int64 [n, 2];
    no host read."""
    _codec_encode('jpeg_encode', JPEG_GEOM, frames, 3, g, scratch, out, meta)


# PNG files of device images (csrc/png_encode.hip, csrc/png_plan.h, include/vqn_image_codec.h; decomp/nerfactor/util/png.py)
# the fields of struct VqnPngGeom, in order
PNG_GEOM = ('n', 'h', 'w', 'c', 'filter_mode', 'rows_per_segment', 'stride', 'segments', 'segment_bytes', 'slot_bytes', 'off_slots',
            'off_lens', 'off_adler', 'off_dst', 'off_sums', 'scratch_bytes', 'out_bytes')
PNG_FILTERS = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': 5}    # 'adaptive': VQN_PNG_FILTER_ADAPTIVE
PNG_SEGMENT_TARGET = 8192          # bytes a default segment holds at most, in whole rows (VQN_PNG_SEGMENT_TARGET)
PNG_HEAD_BYTES = 33                # bytes of a file in front of IDAT (VQN_PNG_HEAD_BYTES)


def png_plan(n, h, w, c, filter_mode, rows_per_segment):
    """The planner's view of a batch (host only): ({name: int} over PNG_GEOM, the 33 bytes of a file in front of IDAT).  filter_mode:
    a value of PNG_FILTERS.  A batch it refuses raises ValueError with its reason."""
    g, head = _codec_plan('vqn_png_plan', PNG_GEOM, PNG_HEAD_BYTES, n, h, w, c, filter_mode, rows_per_segment)
    return g, head.tobytes()


def png_encode(images, g, scratch, out=None, meta=None):
    """images uint8 [n, h, w, c] contiguous device tensor, g the plan of its batch, scratch a uint8 device buffer of g['scratch_bytes']
    (n h stride when out is None: the filtered stream only).  Fills scratch (the filtered stream first), out and meta int64 [n, 2];
    no host read."""
    _codec_encode('png_encode', PNG_GEOM, images, g['c'], g, scratch, out, meta)


def _f64_rows(t, name, D=None):
    if t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda or (D is not None and t.shape[1] != D):
        raise VqnError(f'{name}: expected a contiguous float64 device tensor [rows, {"D" if D is None else D}], got {t.dtype} '
                       f'{tuple(t.shape)} contiguous={t.is_contiguous()} device={t.device}')
    return t


def meanshift_seek(points, seeds, bandwidth, max_iter):
    """points [n, D], seeds [S, D] float64 -> (means float64 [S, D], counts int32 [S] (0: dropped), iters int32 [S]): every seed to
    convergence in one launch, no host read (vqn_meanshift_seek)."""
    _f64_rows(points, 'points')
    n, D = (int(s) for s in points.shape)
    _f64_rows(seeds, 'seeds', D)
    S = int(seeds.shape[0])
    means = torch.empty((S, D), dtype=torch.float64, device=points.device)
    counts = torch.empty((S,), dtype=torch.int32, device=points.device)
    iters = torch.empty((S,), dtype=torch.int32, device=points.device)
    _call('vqn_meanshift_seek', _ptr(points), n, _ptr(seeds), S, D, float(bandwidth), int(max_iter), _ptr(means), _ptr(counts), _ptr(iters))
    return means, counts, iters


def meanshift_merge(candidates, counts, bandwidth):
    """candidates float64 [M, D] with their int32 counts [M], sorted descending by (count, coordinates) -> (kept uint8 [M],
    n_kept int32 [1]), one launch, no host read (vqn_meanshift_merge)."""
    _f64_rows(candidates, 'candidates')
    M, D = (int(s) for s in candidates.shape)
    if counts.dtype != torch.int32 or tuple(counts.shape) != (M,) or not counts.is_contiguous() or counts.device != candidates.device:
        raise VqnError(f'meanshift_merge: counts must be a contiguous int32 [{M}] on the device of the candidates')
    kept = torch.empty((M,), dtype=torch.uint8, device=candidates.device)
    n_kept = torch.empty((1,), dtype=torch.int32, device=candidates.device)
    need = lib().vqn_meanshift_merge_scratch_bytes(M, D)
    buf = _scratch('meanshift_merge', max(need, 64), candidates.device)      # (need = 0: a shape the call itself refuses, with the reason)
    _call('vqn_meanshift_merge', _ptr(candidates), _ptr(counts), M, D, float(bandwidth), _ptr(buf), buf.numel(), _ptr(kept), _ptr(n_kept))
    return kept, n_kept


def meanshift_assign(points, centres, bandwidth=0.0, want_dist=False):
    """points [n, D], centres [K, D] float64 -> (labels int32 [n], dist float64 [n] | None): the nearest centre, ties to the lowest
    index; bandwidth > 0: -1 where the distance is larger (vqn_meanshift_assign)."""
    _f64_rows(points, 'points')
    n, D = (int(s) for s in points.shape)
    _f64_rows(centres, 'centres', D)
    labels = torch.empty((n,), dtype=torch.int32, device=points.device)
    dist = torch.empty((n,), dtype=torch.float64, device=points.device) if want_dist else None
    _call('vqn_meanshift_assign', _ptr(points), n, _ptr(centres), int(centres.shape[0]), D, float(bandwidth), _ptr(labels), _ptr(dist))
    return labels, dist


# --------------------------------------------------------------------------------------
# geometry scores (csrc/geometry_eval.hip, include/vqn_geometry_eval.h; geo/geometry_eval.py)
GEOM_MAX_CELLS = 1 << 24           # cells of a grid at most (VQN_GEOM_MAX_CELLS)
GEOM_MAX_AXIS = 1024               # cells per axis at most (VQN_GEOM_MAX_AXIS)
GEOM_MAX_THRESHOLDS = 8            # distance thresholds of one reduction at most (VQN_GEOM_MAX_THRESHOLDS)
GEOM_OUT_WORDS = 16                # 8-byte words of the reduction's output (VQN_GEOM_OUT_WORDS)
GEOM_THREADS = 256                 # threads of every workgroup (VQN_GEOM_THREADS)
GEOM_REDUCE_GRID_CAP = 1024        # workgroups of the reduction's first launch at most (VQN_GEOM_REDUCE_GRID_CAP)


class GeomGrid(ctypes.Structure):
    """struct VqnGeomGrid: its fields, in order"""
    _fields_ = [('origin', ctypes.c_float * 3), ('h', ctypes.c_float), ('dims', ctypes.c_int32 * 3), ('cells', ctypes.c_int32)]


def _rows3(t, name, dtype=torch.float32, rows=None):
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous() or not t.is_cuda or (rows is not None and t.shape[0] != rows):
        raise VqnError(f'{name}: expected a contiguous {dtype} device tensor [{"n" if rows is None else rows}, 3], got {t.dtype} '
                       f'{tuple(t.shape)} contiguous={t.is_contiguous()} device={t.device}')
    return t


def geom_grid_plan(lo, hi, n, cell=None):
    """The grid over n reference points of bounding box lo .. hi (three floats each; host only) -> GeomGrid.  cell: its size, None for
    the default.  A plan the library refuses raises ValueError with its reason."""
    grid = GeomGrid()
    lo, hi = np.ascontiguousarray(lo, dtype=np.float32).reshape(3), np.ascontiguousarray(hi, dtype=np.float32).reshape(3)
    rc = lib().vqn_geom_grid_plan(lo.ctypes.data, hi.ctypes.data, int(n), 0.0 if cell is None else float(cell), ctypes.addressof(grid))
    if rc != 0:
        raise ValueError(lib().vqn_last_error().decode())
    return grid


def geom_tri_areas(vertices, triangles):
    """vertices f32 [V,3], triangles int32 [T,3] -> float64 [T] (vqn_geom_tri_areas)."""
    _rows3(vertices, 'vertices')
    _rows3(triangles, 'triangles', torch.int32)
    areas = torch.empty((triangles.shape[0],), dtype=torch.float64, device=vertices.device)
    _call('vqn_geom_tri_areas', _ptr(vertices), int(vertices.shape[0]), _ptr(triangles), int(triangles.shape[0]), _ptr(areas))
    return areas


def geom_sample_surface(vertices, triangles, cum, u):
    """cum float64 [T] = the inclusive prefix sum of the areas, u f32 [n,3] in [0,1) -> (points f32 [n,3], normals f32 [n,3], face
    int32 [n]) (vqn_geom_sample_surface)."""
    _rows3(vertices, 'vertices')
    _rows3(triangles, 'triangles', torch.int32)
    _rows3(u, 'u')
    T, n = int(triangles.shape[0]), int(u.shape[0])
    if cum.dtype != torch.float64 or tuple(cum.shape) != (T,) or not cum.is_contiguous() or cum.device != vertices.device:
        raise VqnError(f'geom_sample_surface: cum must be a contiguous float64 [{T}] on the device of the vertices')
    points = torch.empty((n, 3), dtype=torch.float32, device=vertices.device)
    normals = torch.empty((n, 3), dtype=torch.float32, device=vertices.device)
    face = torch.empty((n,), dtype=torch.int32, device=vertices.device)
    _call('vqn_geom_sample_surface', _ptr(vertices), int(vertices.shape[0]), _ptr(triangles), T, _ptr(cum), _ptr(u), n, _ptr(points),
          _ptr(normals), _ptr(face))
    return points, normals, face


def geom_cell_ids(points, grid):
    """points f32 [n,3] -> int32 [n], the id of each point's cell of `grid` (vqn_geom_cell_ids)."""
    _rows3(points, 'points')
    ids = torch.empty((points.shape[0],), dtype=torch.int32, device=points.device)
    _call('vqn_geom_cell_ids', _ptr(points), int(points.shape[0]), ctypes.addressof(grid), _ptr(ids))
    return ids


def geom_pack_sorted(points, order):
    """points f32 [n,3], order int64 [n] (a permutation) -> f32 [n,4]: record j = (x, y, z, the bits of order[j]) of point order[j]
    (vqn_geom_pack_sorted)."""
    _rows3(points, 'points')
    n = int(points.shape[0])
    if order.dtype != torch.int64 or tuple(order.shape) != (n,) or not order.is_contiguous() or order.device != points.device:
        raise VqnError(f'geom_pack_sorted: order must be a contiguous int64 [{n}] on the device of the points')
    packed = torch.empty((n, 4), dtype=torch.float32, device=points.device)
    _call('vqn_geom_pack_sorted', _ptr(points), n, _ptr(order), _ptr(packed))
    return packed


def geom_nearest(query, packed, cell_start, grid, max_d2=float('inf'), q_order=None):
    """query f32 [n_q,3]; packed f32 [n_ref,4], cell_start int32 [cells + 1] and grid: the sorted reference -> (d2 f32 [n_q], idx int32
    [n_q], the original index; -1 / +inf where the nearest d2 > max_d2).  q_order int32 [n_q]: the order in which threads take the
    queries.  One launch (vqn_geom_nearest)."""
    _rows3(query, 'query')
    n_q, n_ref = int(query.shape[0]), int(packed.shape[0])
    if packed.dtype != torch.float32 or packed.dim() != 2 or packed.shape[1] != 4 or not packed.is_contiguous() or packed.device != query.device:
        raise VqnError('geom_nearest: packed must be the contiguous float32 [n_ref, 4] of geom_pack_sorted on the device of the queries')
    if cell_start.dtype != torch.int32 or tuple(cell_start.shape) != (grid.cells + 1,) or not cell_start.is_contiguous() \
            or cell_start.device != query.device:
        raise VqnError(f'geom_nearest: cell_start must be a contiguous int32 [{grid.cells + 1}] on the device of the queries')
    if q_order is not None and (q_order.dtype != torch.int32 or tuple(q_order.shape) != (n_q,) or not q_order.is_contiguous()
                                or q_order.device != query.device):
        raise VqnError(f'geom_nearest: q_order must be a contiguous int32 [{n_q}] on the device of the queries')
    d2 = torch.empty((n_q,), dtype=torch.float32, device=query.device)
    idx = torch.empty((n_q,), dtype=torch.int32, device=query.device)
    _call('vqn_geom_nearest', _ptr(query), n_q, _ptr(q_order), _ptr(packed), _ptr(cell_start), n_ref, ctypes.addressof(grid), float(max_d2),
          _ptr(d2), _ptr(idx))
    return d2, idx


def geom_reduce(d2, idx, n_ref, thresholds=(), q_normals=None, ref_normals=None):
    """The directed sums of one nearest-neighbour result -> int64 [16], the words of vqn_geom_reduce's `out` (view 10..13 as float64).
    Two launches, no host read."""
    n = int(d2.shape[0])
    if d2.dtype != torch.float32 or idx.dtype != torch.int32 or d2.dim() != 1 or tuple(idx.shape) != (n,) or not (d2.is_cuda and idx.is_cuda) \
            or not (d2.is_contiguous() and idx.is_contiguous()):
        raise VqnError('geom_reduce: expected contiguous device tensors d2 float32 [n] and idx int32 [n]')
    if q_normals is not None:
        _rows3(q_normals, 'q_normals', rows=n)
    if ref_normals is not None:
        _rows3(ref_normals, 'ref_normals', rows=int(n_ref))
    out = torch.empty((GEOM_OUT_WORDS,), dtype=torch.int64, device=d2.device)
    need = lib().vqn_geom_reduce_scratch_bytes(n)
    buf = _scratch('geom_reduce', max(need, 64), d2.device)             # (need = 0: a shape the call itself refuses, with the reason)
    _call('vqn_geom_reduce', _ptr(d2), _ptr(idx), n, _ptr(q_normals), _ptr(ref_normals), int(n_ref), _host(thresholds, np.float64),
          len(thresholds), _ptr(buf), buf.numel(), _ptr(out))
    return out


# --------------------------------------------------------------------------------------
# reflectance path (csrc/mlp_chain.hip, csrc/brdf_shade.hip)
def mlp_chain_fwd(desc, wbuf, x, out_widths, mode='f32', outs=None, lds=None):
    """Run a layer program (decomp/packing.py) over x [N, in_stride]; returns one [N, w] tensor per output slot.
    mode 'f16s': the split-precision kernel (program and pack must come from ChainBuilder(mode='f16s')).
    outs / lds: the caller's own output buffers, one per slot ([N, ld] float32 device tensors), and their leading dimensions
    (lds[i] >= out_widths[i]; default: the widths); they are returned as given."""
    assert mode in ('f32', 'f16s')
    entry = 'vqn_mlp_chain_fwd' if mode == 'f32' else 'vqn_mlp_chain_fwd_f16s'
    _f32c(wbuf, 'wbuf'); _f32c(x, 'x')
    d, dp = _i32(desc)
    N = x.shape[0]
    assert x.shape[1] == int(d[8]), (x.shape, int(d[8]))
    lds = list(out_widths) if lds is None else list(lds)
    assert len(lds) == len(out_widths) <= 4 and all(ld >= w for ld, w in zip(lds, out_widths)), (lds, out_widths)
    if outs is None:
        outs = [torch.empty((N, ld), dtype=torch.float32, device=x.device) for ld in lds]
        if lds != list(out_widths):
            outs = [o[:, :w] for o, w in zip(outs, out_widths)]
        ptrs = [o.data_ptr() for o in outs]
    else:
        assert len(outs) == len(out_widths)
        for i, (o, ld) in enumerate(zip(outs, lds)):
            _f32c(o, f'outs[{i}]')
            assert o.numel() >= N * ld, (i, tuple(o.shape), N, ld)
        ptrs = [o.data_ptr() for o in outs]
    args = []
    for i in range(4):
        args += [ptrs[i], lds[i]] if i < len(outs) else [None, 0]
    _call(entry, dp, _ptr(wbuf), _ptr(x), N, *args)
    return outs


def linear2srgb(x):
    """clip to [0, 1] + the sRGB transfer curve in one pass (vqn_linear2srgb)."""
    x = x.contiguous()
    _f32c(x, 'x')
    y = torch.empty_like(x)
    _call('vqn_linear2srgb', _ptr(x), x.numel(), _ptr(y))
    return y


def vq_codebook_frags(codebook):
    """codebook [256, K <= 64] -> the B-fragment + |c|^2 image the fused reflectance kernel reads (vqn_vq_codebook_frags)."""
    _f32c(codebook, 'codebook')
    D, K = codebook.shape
    frags = torch.empty(((1 if K <= 16 else (2 if K <= 32 else 4)) * (16 * 64 * 4 + 16),), dtype=torch.float32, device=codebook.device)
    _call('vqn_vq_codebook_frags', _ptr(codebook), D, K, _ptr(frags))
    return frags


def mlp_chain_vq_fwd(desc_a, wbuf_a, widths_a, desc_b, wbuf_b, widths_b, x, frags, K, eps=1e-6, want_z=False, want_ste=False):
    """Program A (encoder + heads, z through slot 0) -> VQ step on z in LDS -> program B (heads on the straight-through rows) in one
    launch (vqn_mlp_chain_vq_fwd).  Returns (outs_a, outs_b, idx, ste, loss, counts); outs_a[0] (z) is None unless want_z, ste
    (the straight-through rows [N, 256]) None unless want_ste."""
    _f32c(wbuf_a, 'wbuf_a'); _f32c(wbuf_b, 'wbuf_b'); _f32c(x, 'x'); _f32c(frags, 'frags')
    N = x.shape[0]
    dev = x.device
    da, dpa = _i32(desc_a)
    assert x.shape[1] == int(da[8]), (x.shape, int(da[8]))
    outs_a = [torch.empty((N, w), dtype=torch.float32, device=dev) if (i > 0 or want_z) else None for i, w in enumerate(widths_a)]
    outs_b = [torch.empty((N, w), dtype=torch.float32, device=dev) for w in widths_b]
    idx = torch.empty((N,), dtype=torch.int64, device=dev)
    ste = torch.empty((N, 256), dtype=torch.float32, device=dev) if want_ste else None
    loss = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty((K,), dtype=torch.float32, device=dev)
    ws = torch.empty((4096,), dtype=torch.float32, device=dev)
    n = N * 256
    _call('vqn_mlp_chain_vq_fwd', dpa, _ptr(wbuf_a), _host(desc_b), _ptr(wbuf_b), _ptr(x), N, _ptrs(outs_a, 4), (ctypes.c_int32 * 4)(*widths_a),
          _ptrs(outs_b, 4), (ctypes.c_int32 * 4)(*widths_b), _ptr(frags), K, eps, 1.0 / n if n else 0.0, _ptr(idx), _ptr(ste), _ptr(loss),
          _ptr(counts), _ptr(ws))
    return outs_a, outs_b, idx, ste, loss, counts


def brdf_shade_fwd(xyz, normal, rayo, lvis, lxyz, lareas, light, materials, gamma=None, want_normal=True,
                   want_split=False, raw=False, probes=None, lvis_rows=None):
    """materials: [(albedo [N,3], spec [N,3], rough [N,1])] (1 or 2 sets).
    lvis_rows [N] int64 (optional): `lvis` is the FULL-view buffer [n_view, L] and point n reads its row lvis_rows[n].
    -> dict(rgb=[...per set], normal=..., rgb_diff=..., rgb_spec=...)."""
    for n_, t in (('xyz', xyz), ('normal', normal), ('rayo', rayo), ('lxyz', lxyz), ('lareas', lareas), ('light', light)):
        _f32c(t, n_)
    L = lareas.numel()
    assert lxyz.numel() == 3 * L and light.numel() == 3 * L
    N = xyz.shape[0]
    assert normal.shape[0] == N and rayo.shape[0] == N
    rows = None
    if lvis is not None:
        _f32c(lvis, 'lvis')
        if lvis_rows is not None:
            rows = lvis_rows
            assert rows.dtype == torch.int64 and rows.is_contiguous() and rows.is_cuda and rows.numel() == N and lvis.shape[1] == L
        else:
            assert tuple(lvis.shape) == (N, L)
    mats = []
    for (a, s, r) in materials:
        _f32c(a, 'albedo'); _f32c(s, 'spec'); _f32c(r, 'rough')
        assert tuple(a.shape) == (N, 3) and tuple(s.shape) == (N, 3) and r.numel() == N
        mats += [a, s, r]
    while len(mats) < 6:
        mats.append(None)
    dev = xyz.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    rgb = [f(N, 3) for _ in materials]
    nout = f(N, 3) if want_normal else None
    rd, rs = (f(N, 3), f(N, 3)) if want_split else (None, None)
    if gamma is not None:
        gamma = _f32c(gamma.reshape(-1).contiguous(), 'gamma')
    n_probes, rgb_probes = 0, None
    if probes is not None:
        probes = _f32c(probes.reshape(-1, L, 3).contiguous(), 'probes')
        n_probes = probes.shape[0]
        rgb_probes = f(N, n_probes, 3)
    _call('vqn_brdf_shade_fwd_rows', _ptr(rows), _ptr(xyz), _ptr(normal), _ptr(rayo), _ptr(lvis), _ptr(lxyz), _ptr(lareas), _ptr(light), N, L,
          len(materials), *[_ptr(m) for m in mats], _ptr(gamma), _ptr(nout), _ptr(rgb[0]), _ptr(rgb[1] if len(rgb) > 1 else None), _ptr(rd),
          _ptr(rs), int(raw), _ptr(probes), n_probes, _ptr(rgb_probes), clock='vqn_brdf_shade_fwd')
    return dict(rgb=rgb, normal=nout, rgb_diff=rd, rgb_spec=rs, rgb_probes=rgb_probes)


def neus_composite_bwd(rays_o, rays_d, mid_z, dists, sdf, grad, rgb, inv_s, background_rgb, radius, cos_anneal_ratio,
                       g_color, g_weight_sum=None, g_weights=None, g_gradient_error=None, gerr_den=None):
    """Reverse of neus_composite_fwd -> (g_sdf [B,n], g_grad [B,n,3], g_rgb [B,n,3], g_inv_s [B])."""
    for n_, t in (('rays_o', rays_o), ('rays_d', rays_d), ('mid_z', mid_z), ('dists', dists), ('sdf', sdf), ('grad', grad),
                  ('rgb', rgb), ('inv_s', inv_s), ('g_color', g_color)):
        _f32c(t, n_)
    B, n = mid_z.shape
    dev = mid_z.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    g_sdf, g_grad, g_rgb, g_inv_s = f(B, n), f(B, n, 3), f(B, n, 3), f(B)
    opt = lambda t, nm: None if t is None else _f32c(t.contiguous(), nm)
    g_weight_sum, g_weights = opt(g_weight_sum, 'g_weight_sum'), opt(g_weights, 'g_weights')
    g_gradient_error, gerr_den = opt(g_gradient_error, 'g_gradient_error'), opt(gerr_den, 'gerr_den')
    if background_rgb is not None:
        background_rgb = _f32c(background_rgb.reshape(-1)[:3].contiguous(), 'background_rgb')
    _call('vqn_neus_composite_bwd', _ptr(rays_o), _ptr(rays_d), _ptr(mid_z), _ptr(dists), _ptr(sdf), _ptr(grad), _ptr(rgb), _ptr(inv_s),
          _ptr(background_rgb), B, n, float(radius), float(cos_anneal_ratio), _ptr(g_color), _ptr(g_weight_sum), _ptr(g_weights),
          _ptr(g_gradient_error), _ptr(gerr_den), _ptr(g_sdf), _ptr(g_grad), _ptr(g_rgb), _ptr(g_inv_s))
    return g_sdf, g_grad, g_rgb, g_inv_s


def brdf_shade_bwd(xyz, normal, rayo, lvis, lxyz, lareas, light, materials, g_sums):
    """Reverse of brdf_shade_fwd(raw=True).  materials / g_sums: per set (albedo, spec, rough) and d loss / d sum [N,3].
    -> ([(g_albedo, g_spec, g_rough [N,1])...], g_light [L,3])."""
    N, L = xyz.shape[0], lareas.numel()
    dev = xyz.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    args_m, outs = [], []
    for (a, s, r), g in zip(materials, g_sums):
        for t in (a, s, r, g):
            _f32c(t, 'material')
        args_m += [a, s, r, g]
        outs.append((f(N, 3), f(N, 3), f(N, 1)))
    while len(args_m) < 8:
        args_m.append(None)
    flat_out = [t for o in outs for t in o]
    while len(flat_out) < 6:
        flat_out.append(None)
    part = f(lib().vqn_brdf_shade_bwd_partials(N), L, 3)
    _call('vqn_brdf_shade_bwd', _ptr(xyz), _ptr(normal), _ptr(rayo), _ptr(lvis), _ptr(lxyz), _ptr(lareas), _ptr(light), N, L, len(materials),
          *[_ptr(t) for t in args_m], *[_ptr(t) for t in flat_out], _ptr(part))
    return outs, part.sum(0)


# -------------------------------------------------------------------------------------- reflectance training passes (round 4)
def refl_train_fwd_x3(desc, wbuf_pieces, wbuf_f32, pts, z_rows, P, saved, z_rows_out, head_out, split_heads=False, save=True, zx_rows=None,
                      zx_tiles_out=None):
    """Forward of a reflectance stack (optional encoder + up to three heads) on the exact-split engine, keeping what the backward
    needs (csrc/refl_train_x3.hip: vqn_refl_train_fwd_x3).  split_heads: one workgroup row per head (small batches).
    zx_rows [P, z]: the heads' second input (descriptors with zx_tiles > 0: vqn_refl_train_fwd_x3_zx); zx_tiles_out: its tile-format copy."""
    _f32c(wbuf_f32, 'wbuf_f32')
    for t in [t for t in saved if t is not None] + list(head_out) + [t for t in (pts, z_rows, z_rows_out, zx_rows, zx_tiles_out) if t is not None]:
        _f32c(t, 'tensor')
    dp, sp, hp = _host(desc), _ptrs(saved), _ptrs(head_out)
    if zx_rows is None:
        _call('vqn_refl_train_fwd_x3', dp, _ptr(wbuf_pieces), _ptr(wbuf_f32), _ptr(pts), _ptr(z_rows), P, sp, len(saved), _ptr(z_rows_out), hp,
              int(split_heads), int(save))
        return
    if zx_rows.shape[0] != P:
        raise VqnError('refl_train_fwd_x3: zx_rows must have one row per point')
    _call('vqn_refl_train_fwd_x3_zx', dp, _ptr(wbuf_pieces), _ptr(wbuf_f32), _ptr(pts), _ptr(z_rows), _ptr(zx_rows), P, sp, len(saved),
          _ptr(z_rows_out), _ptr(zx_tiles_out), hp, int(split_heads), int(save), clock='vqn_refl_train_fwd_x3')


def refl_train_bwd_x3(desc, wbuf_pieces, wbuf_f32, P, g_out, head_out, g_z_rows, saved, outs, gz_rows_out, run_heads=True, run_enc=True,
                      split_heads=False, d2_row0=None):
    """Backward of the same stack (vqn_refl_train_bwd_x3): fills `outs` with every layer's per-point adjoint in the tile format.
    g_z_rows: list of up to four [P, z] adjoints flowing into z from outside this launch's heads; run_heads / run_enc select the part
    of the stack walked; split_heads (heads only): gz_rows_out holds one [P, z] slice per head."""
    _f32c(wbuf_f32, 'wbuf_f32')
    g_z_rows = [t for t in (g_z_rows or []) if t is not None]
    for t in list(saved) + list(outs) + list(g_out) + list(head_out) + g_z_rows + [t for t in (gz_rows_out,) if t is not None]:
        _f32c(t, 'tensor')
    dp = _host(desc)
    buf = _scratch('refl_bwd', _scratch_bytes('vqn_refl_train_bwd_x3_scratch_bytes', dp), wbuf_f32.device)
    _call('vqn_refl_train_bwd_x3', dp, _ptr(wbuf_pieces), _ptr(wbuf_f32), P, _ptrs(g_out), _ptrs(head_out), _ptrs(g_z_rows), len(g_z_rows),
          _ptrs(saved), len(saved), _ptrs(outs), len(outs), _ptr(gz_rows_out), None if d2_row0 is None else _host(d2_row0),
          int(run_heads), int(run_enc), int(split_heads), _ptr(buf), buf.numel())


# -------------------------------------------------------------------------------------- element-wise pieces (round 4)
def clip_preserve(x, lo, hi):
    """x + (clip(x) - x) in one launch (vqn_clip_preserve)."""
    _f32c(x, 'x')
    y = torch.empty_like(x)
    _call('vqn_clip_preserve', _ptr(x), x.numel(), lo, hi, _ptr(y))
    return y


def ks_split_fwd(basecolor, ks):
    _f32c(basecolor, 'basecolor'); _f32c(ks, 'ks')
    albedo, spec = torch.empty_like(basecolor), torch.empty_like(basecolor)
    _call('vqn_ks_split_fwd', _ptr(basecolor), _ptr(ks), ks.shape[1], basecolor.shape[0], _ptr(albedo), _ptr(spec))
    return albedo, spec


def ks_split_bwd(basecolor, ks, g_albedo, g_spec):
    for t in (g_albedo, g_spec):
        if t is not None:
            _f32c(t, 'gradient')
    g_bc, g_ks = torch.empty_like(basecolor), torch.empty_like(ks)
    _call('vqn_ks_split_bwd', _ptr(basecolor), _ptr(ks), ks.shape[1], basecolor.shape[0], _ptr(g_albedo), _ptr(g_spec), _ptr(g_bc), _ptr(g_ks))
    return g_bc, g_ks


def loss_total(terms, vqloss, sim, use_chr, use_smooth, use_lambert):
    _f32c(terms, 'terms'); _f32c(vqloss, 'vqloss')
    if sim is not None:
        _f32c(sim, 'sim')
    out = torch.empty((terms.shape[0],), dtype=torch.float32, device=terms.device)
    _call('vqn_loss_total', _ptr(terms), terms.shape[0], _ptr(vqloss), _ptr(sim), int(use_chr), int(use_smooth), int(use_lambert), _ptr(out))
    return out


# -------------------------------------------------------------------------------------- training engines (csrc/tile_vm.hip, wgrad*.hip)
def tfmt_pack(x, N, F, ldx, out, tiles_f):
    """rows x [N, F] (row stride ldx) -> the tile format `out` with tiles_f feature tiles, zero padded (vqn_tfmt_pack; not clocked)"""
    _call('vqn_tfmt_pack', _ptr(x), N, F, ldx, _ptr(out), tiles_f, clock=False)


def tfmt_pack_delta(g, N, F, ldg, y_tfmt, act, out, tiles_f):
    """out (tile format) = g act'(y_tfmt), g [N, F] rows of stride ldg or None (vqn_tfmt_pack_delta)"""
    _call('vqn_tfmt_pack_delta', _ptr(g), N, F, ldg, _ptr(y_tfmt), act, _ptr(out), tiles_f)


def tfmt_unpack(t, tiles_f, N, F, out, ldx):
    """the tile format t -> rows out [N, F] of stride ldx (vqn_tfmt_unpack; not clocked)"""
    _call('vqn_tfmt_unpack', _ptr(t), tiles_f, N, F, _ptr(out), ldx, clock=False)


def tile_program(which, desc_dev, desc_host, wbuf, tensors, tensor_ld, N):
    """Run a tile program over N points (vqn_tile_program, clocked as 'vqn_tile_program:' + which); tensors: one tensor (or None) per
    tensor slot of the program, tensor_ld their leading dimensions."""
    _call('vqn_tile_program', _ptr(desc_dev), _host(desc_host), _ptr(wbuf), _ptrs(tensors), _host(tensor_ld), len(tensors), N,
          clock='vqn_tile_program:' + which)


def tile_program_grid(desc_host, N):
    """workgroups vqn_tile_program launches for this program over N points"""
    return lib().vqn_tile_program_grid(_host(desc_host), N)


def wgrad_partials(A, a_tiles, a_t0, a_nt, B, b_tiles, b_t0, b_nt, n_point_tiles, n_split, ws, rowsum_ws=None, x3=False):
    """Split-over-points partial blocks of sum_p A[o][p] B[i][p] (vqn_wgrad_partials, x3: vqn_wgrad_partials_x3) -> their number."""
    return _call('vqn_wgrad_partials_x3' if x3 else 'vqn_wgrad_partials', _ptr(A), a_tiles, a_t0, a_nt, _ptr(B), b_tiles, b_t0, b_nt,
                 n_point_tiles, n_split, _ptr(ws), _ptr(rowsum_ws), count=True)


def reduce_partials(ws, n, rows, cols, out, out_ld, accumulate=0, rowsum=None):
    """out[r][c] (+)= the ordered sum of the n partial blocks [rows, cols] at ws (vqn_reduce_partials; out: a tensor whose first
    element is (0, 0), row stride out_ld).  rowsum = (ws, out, out_ld): also the [1, rows] row-sum partials, in the same clock bracket."""
    with _clock('vqn_reduce_partials'):
        _call('vqn_reduce_partials', _ptr(ws), n, rows, cols, _ptr(out), out_ld, accumulate, clock=False)
        if rowsum is not None:
            _call('vqn_reduce_partials', _ptr(rowsum[0]), n, 1, rows, _ptr(rowsum[1]), rowsum[2], 0, clock=False)


def wgrad_partials_batched(A, a_tiles, a_t0, a_nt, B, b_tiles, b_t0, b_nt, n_point_tiles, n_split, ws, rowsum_ws, x3):
    """vqn_wgrad_partials_batched over the problem lists (clocked as the per-problem entry) -> partial blocks per problem"""
    return _call('vqn_wgrad_partials_batched', len(A), _ptrs(A), _host(a_tiles), _host(a_t0), _host(a_nt), _ptrs(B), _host(b_tiles),
                 _host(b_t0), _host(b_nt), n_point_tiles, n_split, _ptrs(ws), _ptrs(rowsum_ws), int(x3), count=True,
                 clock='vqn_wgrad_partials_x3' if x3 else 'vqn_wgrad_partials')


def wgrad_thin_batched(A, a_tiles, a_t0, a_row0, a_rows, B, b_tiles, b_t0, b_nt, n_point_tiles, n_split, ws, rowsum_ws):
    """vqn_wgrad_thin_batched over the problem lists -> partial blocks per problem"""
    return _call('vqn_wgrad_thin_batched', len(A), _ptrs(A), _host(a_tiles), _host(a_t0), _host(a_row0), _host(a_rows), _ptrs(B),
                 _host(b_tiles), _host(b_t0), _host(b_nt), n_point_tiles, n_split, _ptrs(ws), _ptrs(rowsum_ws), count=True)


def wgrad_finalize(ws, n, ws2, n2, src_rows, src_cols, rows_valid, col_first, cols_valid, dst, dst_row_stride, dst_col_stride, scale):
    """vqn_wgrad_finalize over the entry lists (one entry per result window)"""
    _call('vqn_wgrad_finalize', len(ws), _ptrs(ws), _host(n), _ptrs(ws2), _host(n2), _host(src_rows), _host(src_cols), _host(rows_valid),
          _host(col_first), _host(cols_valid), _ptrs(dst), _host(dst_row_stride, np.int64), _host(dst_col_stride, np.int64),
          _host(scale, np.float32))


def weight_norm_fwd(v, g, w):
    """w_l = g_l v_l / ||v_l||_row for every layer l in one launch (vqn_weight_norm_fwd; not clocked)"""
    _call('vqn_weight_norm_fwd', len(v), _ptrs(v), _ptrs(g), _ptrs(w), _host([t.shape[0] for t in v]), _host([t.shape[1] for t in v]),
          clock=False)


def weight_norm_bwd(v, g, dw, dv, dg):
    """its backward: dv_l, dg_l from dw_l (vqn_weight_norm_bwd; not clocked)"""
    _call('vqn_weight_norm_bwd', len(v), _ptrs(v), _ptrs(g), _ptrs(dw), _ptrs(dv), _ptrs(dg), _host([t.shape[0] for t in v]),
          _host([t.shape[1] for t in v]), clock=False)


def adam_step(params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, steps, lr, beta1, beta2, eps, weight_decay, maximize, eps_mode):
    """vqn_adam_step over the tensor lists (max_exp_avg_sq None without AMSGrad); lr a float or a device scalar tensor"""
    lr_dev = lr if torch.is_tensor(lr) else None
    _call('vqn_adam_step', len(params), _ptrs(params), _ptrs(grads), _ptrs(exp_avg), _ptrs(exp_avg_sq),
          None if max_exp_avg_sq is None else _ptrs(max_exp_avg_sq), _ptrs(steps), _host([p.numel() for p in params], np.int64), _ptr(lr_dev),
          0.0 if lr_dev is not None else float(lr), beta1, beta2, eps, weight_decay, int(maximize), eps_mode)
