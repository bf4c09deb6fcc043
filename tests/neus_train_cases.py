"""Shapes, points, the float32 / float64 statement and the bounds of the per-kernel tests of the NeuS training step
(tests/test_gpu_neus_train_kernels.py): vqn_neus_train_fwd / _x3, vqn_neus_train_bwd / _x3 and the interpreted prog_fwd / prog_cbwd /
prog_sbwd beside them, one network shape at a time.  Everything here runs on the CPU, so the conditions the GPU test rests on (the
statement is the oracle's, every kept point is away from the ReLU kinks in both precisions, the engines the table names are the
ones the host code selects, the comparison can fail) are checked without a GPU too (tests/test_neus_train_cases.py).

The statement is a torch function of the EFFECTIVE weights and biases -- the leaves NeusCoreFunction differentiates:
    sdf = (last SDF layer)[0] / scale, features = the rest;  n = d sdf / dx (create_graph=True);
    rgb = colour net on [x, posenc(dirs), n, features];      L = <rgb, g_rgb> + <n, g_n> + <sdf, g_sdf>
evaluated in float64 (the truth) and in float32 (the yardstick's reference) on the SAME float32 numbers."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import geo as og

Shape = namedtuple('Shape', 'd_hidden n_layers skip_in multires d_out c_hidden c_layers multires_view squeeze_out scale')

SHAPES = {
    'shipped': Shape(256, 8, (4,), 6, 257, 256, 4, 4, True, 1.0),     # baseline
    'w160': Shape(160, 2, (), 6, 161, 96, 2, 4, True, 1.0),           # no skip, 5 tiles, narrower colour net, minimum depth
    'w200': Shape(200, 3, (1,), 10, 201, 136, 1, 1, False, 1.0),      # partial tiles (200; 137 before the skip; 136), 63-feature
                                                                      # embedding, 15 extras, one colour layer, no sigmoid
    'w224': Shape(224, 5, (4,), 6, 225, 256, 3, 4, True, 1.5),        # skip at the last admissible layer (185 wide), colour wider
                                                                      # than SDF, scale != 1
    'w129': Shape(129, 4, (2,), 4, 97, 160, 2, 2, True, 1.0),         # one feature in the last tile, 96 features, 27-feature embedding
    'w288': Shape(288, 3, (2,), 6, 289, 256, 2, 4, True, 1.0),        # 9 tiles: one more than two LDS images hold -- the interpreter, whatever
                                                                      # the environment (the default one used to pick a forward kernel that refuses it)
    'w64': Shape(64, 2, (), 6, 65, 64, 2, 4, True, 1.0),              # interpreter only (the BASELINE small config)
    'w48': Shape(48, 5, (3,), 6, 49, 48, 2, 4, True, 1.0),            # interpreter only, 9-wide layer before the skip
}

# engine id -> environment (both variables are read at call time; 'default' = neither set)
ENGINES = {
    'x3': {'VQN_TRAIN_FWD': 'x3', 'VQN_TRAIN_BWD': 'x3'},
    'fused': {'VQN_TRAIN_FWD': 'fused', 'VQN_TRAIN_BWD': 'fused'},
    'prog': {'VQN_TRAIN_FWD': 'prog', 'VQN_TRAIN_BWD': 'prog'},
    'fwd_x3+bwd_fused': {'VQN_TRAIN_FWD': 'x3', 'VQN_TRAIN_BWD': 'fused'},
    'fwd_fused+bwd_x3': {'VQN_TRAIN_FWD': 'fused', 'VQN_TRAIN_BWD': 'x3'},
    'default': {},
}
# engine id -> (forward_mode(), backward_mode()) the engine must report ('default' is used at 9 tiles only)
MODES = {'x3': ('x3', 'x3'), 'fused': ('f32', 'f32'), 'prog': (None, None), 'fwd_x3+bwd_fused': ('x3', 'f32'),
         'fwd_fused+bwd_x3': ('f32', 'x3'), 'default': (None, None)}
SHAPE_ENGINES = {
    'shipped': ('x3', 'fused', 'prog'), 'w160': ('x3', 'fused', 'prog'),
    'w200': ('x3', 'fused', 'prog', 'fwd_x3+bwd_fused', 'fwd_fused+bwd_x3'),
    'w224': ('x3', 'fused', 'prog'), 'w129': ('x3', 'fused', 'prog'), 'w288': ('default', 'prog'), 'w64': ('prog',), 'w48': ('prog',),
}
# (w288 runs the same three programs under 'default' and 'prog': the GPU test runs 'default', the mode check on the CPU covers both)
GPU_CASES = [(s, e) for s, es in SHAPE_ENGINES.items() for e in es if (s, e) != ('w288', 'prog')]

# the entry points as launches().counts names them (exact keys: vqn_neus_train_fwd is a prefix of its x3 twin)
FWD_ENTRY = {'x3': ('vqn_neus_train_fwd_x3',), 'f32': ('vqn_neus_train_fwd',), None: ('vqn_tile_program:prog_fwd',)}
BWD_ENTRY = {'x3': ('vqn_neus_train_bwd_x3',), 'f32': ('vqn_neus_train_bwd',),
             None: ('vqn_tile_program:prog_cbwd', 'vqn_tile_program:prog_sbwd')}
ALL_ENTRIES = tuple(n for t in list(FWD_ENTRY.values()) + list(BWD_ENTRY.values()) for n in t)

POINTS = (1, 33, 65, 161)        # one tile + phantom second image; ragged second tile; odd tile count; six tiles, one point in the last
POISON_POINTS = (33, 161)
MARGIN = 1e-5                    # smallest |colour pre-activation| (float64) of a kept point
REJECT_CAP = 0.15                # of the 2 P candidates of a case
EPS8 = 8.0 * 2.0 ** -24          # the floor of kernel_cases.yardstick, relative to the largest entry


def select(monkeypatch, engine):
    """the environment of an engine id, and nothing else that moves the choice"""
    for k in ('VQN_TRAIN_FWD', 'VQN_TRAIN_BWD', 'VQN_NEUS_TILE32'):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv(k, v)


def expected_entries(engine):
    """-> (entry points that must have run, entry points that must not)"""
    f, b = MODES[engine]
    ran = FWD_ENTRY[f] + BWD_ENTRY[b]
    return ran, tuple(n for n in ALL_ENTRIES if n not in ran)


# ---------------------------------------------------------------------------------------------------------------- networks
def cfg_of(shape):
    s = SHAPES[shape]
    return dict(sdf=dict(d_in=3, d_out=s.d_out, d_hidden=s.d_hidden, n_layers=s.n_layers, skip_in=tuple(s.skip_in), multires=s.multires,
                         bias=0.5, scale=s.scale),
                color=dict(d_feature=s.d_out - 1, mode='idr', d_in=9, d_out=3, d_hidden=s.c_hidden, n_layers=s.c_layers,
                           multires_view=s.multires_view, squeeze_out=s.squeeze_out))


@functools.lru_cache(maxsize=None)
def params_of(shape):
    cfg = cfg_of(shape)
    return og.make_sdf_params(cfg, 0), og.make_color_params(cfg, 1)


def build_modules(shape, device='cpu'):
    """SDFNetwork / RenderingNetwork of the shape holding the oracle's parameters (as tests/test_gpu_neus_render._build)."""
    from vqnerf_release_amd.geo.models.fields import SDFNetwork, RenderingNetwork
    cfg = cfg_of(shape)
    c, cc = cfg['sdf'], cfg['color']
    p_sdf, p_col = params_of(shape)
    sdf = SDFNetwork(d_in=3, d_out=c['d_out'], d_hidden=c['d_hidden'], n_layers=c['n_layers'], skip_in=tuple(c['skip_in']),
                     multires=c['multires'], bias=c['bias'], scale=c['scale'], geometric_init=True, weight_norm=True)
    sdf.load_state_dict({k: torch.tensor(v) for k, v in p_sdf.items()})
    col = RenderingNetwork(d_feature=cc['d_feature'], mode=cc['mode'], d_in=cc['d_in'], d_out=cc['d_out'], d_hidden=cc['d_hidden'],
                           n_layers=cc['n_layers'], weight_norm=True, multires_view=cc['multires_view'], squeeze_out=cc['squeeze_out'])
    col.load_state_dict({k: torch.tensor(v) for k, v in p_col.items()})
    return sdf.to(device), col.to(device)


def build_engine(shape, device='cpu'):
    from vqnerf_release_amd.geo.train_programs import NeusTrainEngine
    return NeusTrainEngine(*build_modules(shape, device))


@functools.lru_cache(maxsize=None)
def effective_params(shape):
    """The float32 effective weights and biases every evaluation starts from: (W, b, Wc, bc) as lists of float32 CPU tensors."""
    p_sdf, p_col = (og.to_torch(p) for p in params_of(shape))
    cfg = cfg_of(shape)
    nS, nCc = len(og.sdf_dims(cfg)) - 1, len(og.color_dims(cfg)) - 1
    return ([og.wn_weight(p_sdf, l) for l in range(nS)], [p_sdf[f'lin{l}.bias'] for l in range(nS)],
            [og.wn_weight(p_col, l) for l in range(nCc)], [p_col[f'lin{l}.bias'] for l in range(nCc)])


def grad_names(shape):
    W, b, Wc, bc = effective_params(shape)
    return [f'dW{l}' for l in range(len(W))] + [f'db{l}' for l in range(len(b))] + [f'dWc{l}' for l in range(len(Wc))] + \
        [f'dbc{l}' for l in range(len(bc))]


# ---------------------------------------------------------------------------------------------------------------- the statement
def loss_of(sdf, n, rgb, adj):
    """L of one adjoint variant; adj = (g_rgb, g_n | None, g_sdf | None): a None term is absent from the loss"""
    g_rgb, g_n, g_sdf = adj
    L = (rgb * g_rgb).sum()
    if g_n is not None:
        L = L + (n * g_n).sum()
    if g_sdf is not None:
        L = L + (sdf * g_sdf).sum()
    return L


def statement(shape, W, b, Wc, bc, x, dirs, adjoints=None, skip_div=True, sdf_div=True):
    """The training step's network in the dtype of its arguments.  adjoints: {variant: (g_rgb, g_n | None, g_sdf | None)} -> the
    gradients of L for every leaf of W + b + Wc + bc per variant.  skip_div / sdf_div = False leave out the 1/sqrt2 of the skip
    layer / the 1/scale of the sdf output: the two wrong statements of the mutation check, never a reference.
    -> dict(sdf [P,1], feat, n [P,3], rgb [P,3], pre = [colour ReLU pre-activations], grads = {variant: {name: array}})"""
    s = SHAPES[shape]
    nS, nCc = len(W), len(Wc)
    x = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        emb = og.posenc(x * s.scale, s.multires)
        h = emb
        for l in range(nS):
            if l in s.skip_in:
                h = torch.cat([h, emb], 1)
                if skip_div:
                    h = h / math.sqrt(2)
            h = F.linear(h, W[l], b[l])
            if l < nS - 1:
                h = og.softplus100(h)
        sdf = h[:, :1] / s.scale if sdf_div else h[:, :1]
        feat = h[:, 1:]
        n = torch.autograd.grad(sdf.sum(), x, create_graph=True)[0]
        h = torch.cat([x, og.posenc(dirs, s.multires_view), n, feat], -1)
        pre = []
        for l in range(nCc):
            h = F.linear(h, Wc[l], bc[l])
            if l < nCc - 1:
                pre.append(h)
                h = F.relu(h)
        rgb = torch.sigmoid(h) if s.squeeze_out else h
        out = dict(sdf=sdf.detach().numpy(), feat=feat.detach().numpy(), n=n.detach().numpy(), rgb=rgb.detach().numpy(),
                   pre=[p.detach().numpy() for p in pre], grads={})
        leaves = list(W) + list(b) + list(Wc) + list(bc)
        for name, adj in (adjoints or {}).items():
            g = torch.autograd.grad(loss_of(sdf, n, rgb, adj), leaves, retain_graph=True, allow_unused=True)
            out['grads'][name] = {k: (torch.zeros_like(t) if gi is None else gi).numpy() for k, gi, t in zip(grad_names(shape), g, leaves)}
    return out


def _leaves(shape, dtype, grad):
    return tuple([t.to(dtype).clone().requires_grad_(grad) for t in ts] for ts in effective_params(shape))


def seed_of(shape, P):
    return 1000 * list(SHAPES).index(shape) + P


@functools.lru_cache(maxsize=None)
def reference(shape, P):
    """One case: P screened points, the three adjoints, and the statement in float32 and float64 with the gradients of the variants
    'all' (three adjoints) and 'rgb' (g_rgb alone).  Computed once per (shape, P) and shared; nobody writes into it.
    -> dict(x, dirs, g_rgb, g_n, g_sdf: float32 tensors; n_candidates, n_rejected; f32, f64: results of statement())"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)             # one summation order for the float32 reference, however many cores the machine has
    try:
        return _reference(shape, P)
    finally:
        torch.set_num_threads(threads)


def _reference(shape, P):
    rng = np.random.default_rng(seed_of(shape, P))
    xc = rng.uniform(-1.0, 1.0, (2 * P, 3)).astype(np.float32)
    dc = rng.normal(size=(2 * P, 3))
    dc = (dc / np.linalg.norm(dc, axis=1, keepdims=True)).astype(np.float32)
    g_rgb, g_n, g_sdf = (torch.tensor(rng.normal(size=(P, k)).astype(np.float32)) for k in (3, 3, 1))
    # ReLU is the only kink: keep the first P candidates whose colour pre-activations all stay MARGIN away from it in float64
    scr = statement(shape, *_leaves(shape, torch.float64, False), torch.tensor(xc).double(), torch.tensor(dc).double())
    ok = np.concatenate([np.abs(p) for p in scr['pre']], 1).min(1) >= MARGIN
    keep = np.flatnonzero(ok)[:P]
    assert keep.size == P, f'{shape} P={P}: only {keep.size} of {2 * P} candidates pass the screening'
    x, dirs = torch.tensor(xc[keep]), torch.tensor(dc[keep])
    ref = dict(x=x, dirs=dirs, g_rgb=g_rgb, g_n=g_n, g_sdf=g_sdf, n_candidates=2 * P, n_rejected=int((~ok).sum()))
    for key, dt in (('f32', torch.float32), ('f64', torch.float64)):
        adj = {'all': (g_rgb.to(dt), g_n.to(dt), g_sdf.to(dt)), 'rgb': (g_rgb.to(dt), None, None)}
        ref[key] = statement(shape, *_leaves(shape, dt, True), x.to(dt), dirs.to(dt), adj)
    return ref


# ---------------------------------------------------------------------------------------------------------------- the gradient bound
def pooled_gradient_check(got, ref32, ref64, f_max=3.0, f_rms=2.0):
    """Parameter gradients of ONE case (dicts name -> array).  Every tensor's error is normalised by the largest entry of its float64
    reference; every tensor is held to f_max x the LARGEST normalised error of the float32 statement over the case's tensors (rms:
    f_rms x the largest normalised rms), floor 8 float32 epsilons.  Pooled, because the float32 statement's own error varies between
    2e-8 and 3e-6 of the largest entry among the tensors of one case: a per-tensor bound would fail a correct kernel on the tensors
    where torch happened to be exact (the idea behind kernel_cases.yardstick's floor).  A tensor whose reference is identically
    zero must be exactly zero.
    -> dict(bound, rms_bound, tensors = {name: dict(e_hip, e_ref, rms_hip, rms_ref)}, bad = [names], ok)"""
    rms = lambda e: float(np.sqrt((e ** 2).mean()))
    per, bad = {}, []
    for k, r64 in ref64.items():
        h, r32, r64 = (np.asarray(a, np.float64) for a in (got[k], ref32[k], r64))
        assert h.shape == r32.shape == r64.shape, (k, h.shape, r32.shape, r64.shape)
        assert np.isfinite(r64).all() and np.isfinite(r32).all(), f'{k}: reference is not finite'
        top = float(np.abs(r64).max())
        if top == 0.0:
            if np.any(h != 0.0):
                bad.append(k)
            continue
        eh = np.where(np.isfinite(h), np.abs(h - r64), np.inf) / top
        er = np.abs(r32 - r64) / top
        per[k] = dict(e_hip=float(eh.max()), e_ref=float(er.max()), rms_hip=rms(eh), rms_ref=rms(er))
    bound = max(f_max * max(t['e_ref'] for t in per.values()), EPS8)
    rms_bound = max(f_rms * max(t['rms_ref'] for t in per.values()), EPS8)
    bad += [k for k, t in per.items() if not (t['e_hip'] <= bound and t['rms_hip'] <= rms_bound)]
    return dict(bound=bound, rms_bound=rms_bound, tensors=per, bad=bad, ok=not bad)
