"""Inputs and references of the per-kernel tests of the reflectance step's loss side (tests/test_gpu_loss_kernels.py): the entry
points of csrc/decomp_loss.hip and csrc/elementwise.hip.  Like tests/kernel_cases.py everything here runs on the CPU from the oracle
statements alone, so the conditions the GPU tests rest on are checked without a GPU (tests/test_loss_kernel_cases.py).  Three kinds
of reference: oracle.decomp's torch statements evaluated in float64 (the truth) and in float32 (the yardstick's measure of what
float32 can deliver), closed forms where torch's autograd gives NaN and the statement's framework gives 0, and plain numpy float32
restatements -- one rounding per operation -- for the kernels that promise the statement's own bits."""
import numpy as np
import torch

from oracle import decomp as od
from tests import kernel_cases as kc

yardstick, Report = kc.yardstick, kc.Report
f32 = np.float32
MARGIN = 1e-5                # what the tests require of every kink
BUILD_MARGIN = 4e-4          # what the inputs are built with
MI355X_CUS = 256             # for sizing the grid-cap cases without a device (the GPU tests take the device's own count)


def F(v):
    """the float32 the C ABI receives for the Python number v, as a Python float: both references use the kernel's own constants"""
    return float(f32(v))


def bits(a):
    """float32 array -> its bit patterns, every NaN folded into one (for the comparisons that have no tolerance)"""
    a = np.ascontiguousarray(np.asarray(a, f32))
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


# ------------------------------------------------------------------------------------------- vqn_decomp_loss_fwd / _bwd
W = {k: F(v) for k, v in dict(rgb=0.2, chr=1.0, smooth=0.05, alpha=60.0, thres=0.1, lambert=1e-3).items()}
LOSS_N = (1, 2, 3, 9, 258)
LOSS_D = (4, 60, 64, 252, 256, 260)
TERMS = ('rgb', 'vqrgb', 'chromaticity', 'chr_smooth', 'lambert')
SRGB_KNEE = 0.04045


def _chroma64(v):
    v = np.asarray(v, np.float64)
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return np.divide(v, n, out=np.zeros_like(v), where=n != 0)


def pair_distance(rgb_gt):
    """e of every whole pair (rows 2j, 2j + 1), in float64 on the float32 inputs -> [N // 2]"""
    P = rgb_gt.shape[0] // 2
    c = _chroma64(rgb_gt[:2 * P])
    return np.sqrt(((c[0::2] - c[1::2]) ** 2).sum(-1))


def spec_gap(spec):
    """largest minus second largest entry of every row (0.0 exactly on a tie)"""
    s = np.sort(np.asarray(spec, np.float64), -1)
    return s[:, 2] - s[:, 1]


def loss_inputs(N, D, seed=0):
    """float32 inputs of the per-point loss terms after the recipe of tests/test_gpu_decomp.py: about half of the pairs under
    chr_thres, targets on both sides of the sRGB knee, rough on both sides of 0.5, rows with vq_rgb == 0 (the chromaticity gradient
    is 0 there), a three-way and a two-way tie in max(spec), and an independent upstream gradient per term.  Every kink is kept
    BUILD_MARGIN away by construction: no row is ever filtered."""
    rng = np.random.default_rng(100003 * seed + 1009 * N + D)
    P = N // 2
    gt = np.where(rng.uniform(size=(N, 3)) < 0.1, rng.uniform(0.005, 0.04, (N, 3)), rng.uniform(0.06, 1.0, (N, 3)))
    gt[0, 1] = 0.02                                                       # under the knee in every case
    if P:
        close = rng.uniform(size=(P, 1)) < 0.5
        close[0] = True
        if P > 1:
            close[1] = False
        gt[1:2 * P:2] = np.where(close, gt[0:2 * P:2] + rng.normal(0, 0.01, (P, 3)), gt[1:2 * P:2]).clip(0.005, 1.0)
    gt = gt.astype(f32)
    gt[np.abs(gt.astype(np.float64) - SRGB_KNEE) < BUILD_MARGIN] = 0.05
    if P:
        bad = np.flatnonzero(np.abs(pair_distance(gt) - W['thres']) < BUILD_MARGIN)
        gt[2 * bad + 1] = gt[2 * bad]                                     # e == 0.0 in every precision
    rough = rng.uniform(0, 1, (N, 1)).astype(f32)
    rough[np.abs(rough - 0.5) < BUILD_MARGIN] = 0.75
    spec = rng.uniform(0, 0.3, (N, 3)).astype(f32)
    tie3 = 5 if N > 5 else N - 1
    tie2 = [r for r in ((6, 7) if N > 7 else (N - 2,)) if 0 <= r != tie3]
    spec[tie3] = 0.2
    for n_, r in enumerate(tie2):                                         # (a, m, m): first maximum 1; (m, a, m): first maximum 0
        spec[r] = (0.1, 0.25, 0.25) if n_ == 0 else (0.25, 0.1, 0.25)
    free = np.ones(N, bool)
    free[[tie3] + tie2] = False
    top = np.argmax(spec, -1)
    fix = free & (spec_gap(spec) < BUILD_MARGIN)
    spec[fix, top[fix]] += f32(0.01)
    vq = rng.uniform(0, 1, (N, 3)).astype(f32)
    zero_rows = np.zeros(N, bool)
    zero_rows[[r for r in (3, 10) if r < N]] = True
    if N < 4 and D % 8 == 4:
        zero_rows[N - 1] = True
    vq[zero_rows] = 0.0
    return dict(rgb_pred=rng.uniform(0, 1, (N, 3)).astype(f32), vq_rgb=vq, rgb_gt=gt, z=(rng.normal(size=(N, D)) / np.sqrt(D)).astype(f32),
                spec=spec, rough=rough, g_terms=rng.normal(size=(N, 5)).astype(f32), zero_rows=zero_rows, tie3=tie3, tie2=tuple(tie2))


def loss_reference(inp, nerf, dtype, w=W, use_z=True, use_spec=True):
    """oracle.decomp.compute_loss's train branch in `dtype` on the float32 inputs, its per-point terms as [N, 5] (TERMS), and the
    autograd adjoints of sum(g_terms * terms).  The pair term is taken on the whole pairs; a lone last point of an odd N has none.
    Rows with |vq_rgb| = 0: torch differentiates sqrt at 0 and returns NaN; TensorFlow's divide_no_nan and SqrtGrad give 0 for the
    chromaticity part there, which leaves the mse part g_1 (2 / 3) (vq_rgb - linear_gt) -- the closed form put in place here.
    -> dict(terms, g_pred, g_vq, g_z | None, g_spec | None) of numpy arrays."""
    T = lambda k: torch.tensor(inp[k], dtype=dtype)
    N = inp['rgb_gt'].shape[0]
    leaves = {k: T(k).requires_grad_(True) for k in ('rgb_pred', 'vq_rgb', 'z', 'spec')}
    gt, rough, g_terms = T('rgb_gt'), T('rough'), T('g_terms')
    P2 = 2 * (N // 2)
    parts = []
    for a, b in ((0, P2), (P2, N)):
        if a == b:
            continue
        out = dict(rgb=leaves['rgb_pred'][a:b], vq_rgb=leaves['vq_rgb'][a:b], vq=dict(loss=torch.zeros((), dtype=dtype)),
                   z_vq=leaves['z'][a:b], spec=leaves['spec'][a:b], rough=rough[a:b])
        _, ld = od.compute_loss(out, gt[a:b], None, mode='train', data_type='nerf' if nerf else 'hw', chr_alpha=w['alpha'],
                                chr_thres=w['thres'], chromaticity_weight=w['chr'], combine_weight=w['rgb'], sim_loss_weight=0.0,
                                mat_sloss_weight=w['smooth'] if (use_z and (a, b) == (0, P2)) else 0.0,
                                lambert_weight=w['lambert'] if use_spec else 0.0)
        parts.append(torch.stack([ld[k] if k in ld else torch.zeros(b - a, dtype=dtype) for k in TERMS], -1))
    terms = torch.cat(parts, 0)
    g = torch.autograd.grad((g_terms * terms).sum(), list(leaves.values()), allow_unused=True)
    g_pred, g_vq, g_z, g_spec = (torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, leaves.values()))
    zr = torch.tensor(inp['zero_rows'])
    lin = od.srgb2linear(gt) if nerf else gt
    g_vq = torch.where(zr[:, None], g_terms[:, 1:2] * (2.0 / 3.0) * (leaves['vq_rgb'].detach() - lin), g_vq)
    n = lambda t: t.detach().numpy()
    return dict(terms=n(terms), g_pred=n(g_pred), g_vq=n(g_vq), g_z=n(g_z) if use_z else None, g_spec=n(g_spec) if use_spec else None)


def loss_pair_distance(inp, dtype):
    """e of every whole pair as the statement computes it in `dtype` (before the threshold)"""
    P = inp['rgb_gt'].shape[0] // 2
    c = od.rgb2chromaticity(torch.tensor(inp['rgb_gt'][:2 * P], dtype=dtype))
    return torch.sqrt(((c[::2] - c[1::2]) ** 2).sum(-1)).numpy()


# --------------------------------------------------------------------------- vqn_sim_smooth_fwd / _bwd, vqn_codebook_prep
SIM_CASES = ((252, 15), (256, 33), (256, 48), (256, 49), (33, 5), (7, 2), (1028, 256))
SIM_UNALIGNED = (256, 15)     # the case that is also run on a view 4 bytes into its buffer
SIM_W = F(0.3)


def sim_chain_factor(D):
    """Yardstick factor for a sim-smooth tensor that passes the default 3 x / 2 x: 3 sqrt(D), for max and rms alike.  The kernel
    accumulates the pair's squared distance as ONE in-order chain of D fmaf (its documented, bit-reproducible order): D roundings,
    each up to u = 2^-24 of the running sum, which add up like a random walk to ~sqrt(D) u of the sum (worst case D u).  The float32
    statement is torch's pairwise sum -- log2(D) roundings deep, ~u of the sum in all, and for the one-element tensors `dist` and
    `term` simply wherever in its last half ulp the result happens to fall (0.09 ulp at D = 1028).  So a correct chain may err
    ~sqrt(D) times the statement's own error: 3 sqrt(D) keeps the yardstick's factor of 3 on top of that ratio (96 at D = 1028,
    48 at D = 256; the worst-case ratio D / log2(D) would allow 308 and 96).  `dist`, `term` = -w log(dist) and g_cb = -w g (c_i -
    c_j) / dist^2 all inherit the chain's error through the one number dist, fully correlated over the elements of g_cb, which is
    why rms gets the same factor as max."""
    return dict(f_max=3.0 * float(np.sqrt(D)), f_rms=3.0 * float(np.sqrt(D)))
SIM_G = F(2.0)


def sim_inputs(D, K, seed=0):
    """A prepared codebook [D, K] (clipped, l2-normalised columns) whose closest pair is separated from the runner-up by
    construction: column K - 1 is moved half-way towards column K // 3 (for K > 2), which puts the pair's flat index i K + j past
    the first 256 wherever K allows."""
    rng = np.random.default_rng(977 * seed + 31 * D + K)
    cb = od.get_codebook(torch.tensor(rng.uniform(-0.2, 1.2, (D, K)).astype(f32))).numpy().copy()
    if K > 2:
        i, j = K // 3, K - 1
        cb[:, j] = cb[:, i] + f32(0.5) * (cb[:, j] - cb[:, i])
    return cb


def sim_distances(cb, dtype):
    """|c_i - c_j| for i < j, +inf elsewhere, [K, K] in `dtype` (rows in blocks: [K, K, D] at K = 256, D = 1028 is half a GB)"""
    c = torch.tensor(np.asarray(cb), dtype=dtype).t()
    K = c.shape[0]
    d = torch.full((K, K), float('inf'), dtype=dtype)
    for i0 in range(0, K, 16):
        blk = torch.sqrt(((c[i0:i0 + 16, None, :] - c[None, :, :]) ** 2).sum(-1))
        keep = torch.arange(K)[None, :] > torch.arange(i0, min(K, i0 + 16))[:, None]
        d[i0:i0 + 16] = torch.where(keep, blk, d[i0:i0 + 16])
    return d


def sim_reference(cb, dtype, w=SIM_W, g_loss=SIM_G):
    """The code-separation term of compute_loss (oracle/decomp.py, `sim_loss_weight`: -w log of the smallest distance between two
    different codes) on an already prepared codebook, in `dtype`, and g_loss times its gradient wrt the codebook.  The minimum over
    the masked matrix is the minimum over the pairs i < j; autograd through it reaches only the minimal pair's two columns, which is
    how the gradient is taken here.  -> dict(term, dist, pair (first minimum in the order of i K + j), gap (runner-up / min - 1), g_cb).
    The same torch statement serves both precisions (torch's float32 sum is pairwise: see SIM_CHAIN_FACTOR)."""
    d = sim_distances(cb, dtype)
    K = d.shape[0]
    flat = d.reshape(-1)
    p = int(torch.argmin(flat))
    assert int((flat == flat[p]).nonzero()[0]) == p
    i, j = p // K, p % K
    rest = flat.clone()
    rest[p] = float('inf')
    gap = float(rest.min() / flat[p] - 1.0) if K > 2 else float('inf')
    c = torch.tensor(np.asarray(cb), dtype=dtype).requires_grad_(True)
    dist = torch.sqrt(((c[:, i] - c[:, j]) ** 2).sum())
    term = w * (-torch.log(dist))
    g_cb, = torch.autograd.grad(g_loss * term, c)
    return dict(term=term.detach().numpy().reshape(1), dist=dist.detach().numpy().reshape(1), pair=(i, j), gap=gap, g_cb=g_cb.numpy())


def sim_tie_case(same_thread):
    """Entries k / 64, D = 8, K = 40: every squared distance is a multiple of 1 / 4096 below 8, exact in float32.  Two pairs differ
    in one entry by 1 / 64 (the smallest distance there can be, bit-equal for both); every other pair is farther apart.  Pair p is
    visited by thread p % 256 of the one workgroup: (0, 5) and (6, 21) are 256 apart -- one thread meets both -- while (2, 30) and
    (20, 25) belong to threads 110 and 57, so the pair with the smaller index sits in the LATER thread.
    -> (codebook [8, 40] float32, integer numerators [8, 40], the two pairs, the pair to report)."""
    K, D = 40, 8
    rng = np.random.default_rng(40 + int(same_thread))
    q = rng.integers(8, 56, (D, K))
    pairs = ((0, 5), (6, 21)) if same_thread else ((2, 30), (20, 25))
    for i, j in pairs:
        q[:, j] = q[:, i]
        q[3, j] += 1
    return (q / 64.0).astype(f32), q, pairs, min(pairs, key=lambda p: p[0] * K + p[1])


PREP_D = (1, 32, 252, 256, 515)
PREP_K = (1, 15, 70)
PREP_EPS = F(1e-6)


def prep_inputs(D, K, seed=0):
    """raw codebook variable [D, K] with entries outside [0, 1] and (column 0, wherever there is a second column or D is even) a
    column whose squared norm is under the eps clamp; gy [D, K] the upstream gradient of the `g` form."""
    rng = np.random.default_rng(811 * seed + 17 * D + K)
    raw = rng.uniform(-0.2, 1.2, (D, K)).astype(f32)
    if K > 1 or D % 2 == 0:
        raw[:, 0] *= f32(1e-5)
    return raw, rng.normal(size=(D, K)).astype(f32)


def prep_reference(raw, gy, dtype):
    """get_codebook with the model's gradient convention (clip with identity gradient, oracle.decomp._clip01_pg; the values are
    get_codebook's) and the adjoint of sum(gy * codebook) wrt raw.  -> (codebook, g_raw, squared column norms before the clamp)"""
    x = torch.tensor(raw, dtype=dtype).requires_grad_(True)
    c = od._clip01_pg(x)
    cb = od.safe_l2_normalize(c, 0, eps=PREP_EPS)
    g, = torch.autograd.grad((cb * torch.tensor(gy, dtype=dtype)).sum(), x)
    return cb.detach().numpy(), g.numpy(), (c * c).sum(0).detach().numpy()


# ------------------------------------------------------------------------------------------------------ vqn_vq_ema_update
EMA_K = (1, 2, 15, 256, 257, 1024)
EMA_D = (1, 4, 252)
EMA_DECAY = 0.999
EMA_EPS = F(1e-5)
EMA_CALLS = 4


def ema_inputs(K, D, seed=0):
    """Four training calls' worth of rows for oracle.decomp.vq_ema_call: x [n, D] with entries m / 64 and at most 6 rows per code, so
    that counts and dw = x^T one_hot(idx) are exact in float32 and float64 alike (the kernel's inputs are then the statement's own
    intermediate values, to the bit); in the third call the upper half of the codes (the only code at K = 1) gets no row.
    -> dict(cb [D, K], calls = [dict(x, idx, counts [K], dw [D, K])])."""
    rng = np.random.default_rng(613 * seed + 7 * K + D)
    cb = rng.uniform(0, 1, (D, K))
    cb = (cb / np.linalg.norm(cb, axis=0, keepdims=True)).astype(f32)
    calls = []
    for c in range(EMA_CALLS):
        per = rng.integers(1, 7, K)
        if c == 2:
            per[K // 2:] = 0
        idx = rng.permutation(np.repeat(np.arange(K), per))
        if len(idx) == 0:                                        # (K = 1, third call: the statement still needs a row; it goes nowhere)
            x, counts, dw = np.zeros((0, D), f32), np.zeros(K, f32), np.zeros((D, K), f32)
        else:
            x = (rng.integers(0, 65, (len(idx), D)) / 64.0).astype(f32)
            counts = np.bincount(idx, minlength=K).astype(f32)
            dw = np.zeros((D, K))
            np.add.at(dw.T, idx, x.astype(np.float64))
            assert np.array_equal(dw.astype(f32).astype(np.float64), dw)
            dw = dw.astype(f32)
        calls.append(dict(x=x, idx=idx.astype(np.int64), counts=counts, dw=dw))
    return dict(cb=cb, calls=calls)


def ema_reference(inp, dtype):
    """oracle.decomp.vq_ema_call in training (both EMA objects, the Laplace-smoothed cluster sizes, the codebook move) over the calls,
    state carried in `dtype`.  -> per call dict(counter, hidden_cs, average_cs, hidden_dw, average_dw, update)."""
    D, K = inp['cb'].shape
    C = torch.tensor(inp['cb'], dtype=dtype)
    ema_cs, ema_dw = od.EMA(EMA_DECAY, (K,), dtype), od.EMA(EMA_DECAY, (D, K), dtype)
    out = []
    for c in inp['calls']:
        r = od.vq_ema_call(torch.tensor(c['x'], dtype=dtype), C, ema_cs, ema_dw, True, eps=EMA_EPS, idx=torch.tensor(c['idx']))
        out.append(dict(counter=ema_cs.counter, hidden_cs=ema_cs.hidden.numpy().copy(), average_cs=ema_cs.average.numpy().copy(),
                        hidden_dw=ema_dw.hidden.numpy().copy(), average_dw=ema_dw.average.numpy().copy(), update=r['update'].numpy().copy()))
    return out


def ema_hidden_f32(inp):
    """hidden of both averages after every call, numpy float32, one rounding per operation: h - (h - v) * float32(1 - decay)"""
    om = f32(1.0 - EMA_DECAY)
    h_cs, h_dw = np.zeros_like(inp['calls'][0]['counts']), np.zeros_like(inp['calls'][0]['dw'])
    out = []
    for c in inp['calls']:
        h_cs = h_cs - (h_cs - c['counts']) * om
        h_dw = h_dw - (h_dw - c['dw']) * om
        assert h_cs.dtype == f32 and h_dw.dtype == f32
        out.append((h_cs, h_dw))
    return out


# ------------------------------------------------------------------------------ vqn_l2_normalize_rows_bwd, vqn_vq_train_bwd
ROW_D = (4, 252, 256, 260, 1020, 1024)
ROW_N = (1, 3, 5, 1001)
ROW_EPS = F(1e-6)
ROW_GL = F(0.37)


def row_inputs(N, D, seed=0):
    """signed rows x [N, D] (for N >= 3: row 1 at 1e-5 scale, under the eps clamp, and row 2 zero), an upstream g, and the training
    quantiser's tensors: xn = the normalised rows in float32, q unit rows, gs the straight-through adjoint."""
    rng = np.random.default_rng(409 * seed + 13 * N + D)
    x = rng.normal(size=(N, D)).astype(f32)
    if N >= 3:
        x[1] *= f32(1e-5)
        x[2] = 0.0
    q = rng.normal(size=(N, D))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    xn = od.safe_l2_normalize(torch.tensor(x), 1, eps=ROW_EPS).numpy()
    return dict(x=x, g=rng.normal(size=(N, D)).astype(f32), xn=xn, q=q, gs=rng.normal(size=(N, D)).astype(f32))


def l2_bwd_reference(x, g, dtype):
    xr = torch.tensor(x, dtype=dtype).requires_grad_(True)
    gx, = torch.autograd.grad(od.safe_l2_normalize(xr, 1, eps=ROW_EPS), xr, torch.tensor(g, dtype=dtype))
    return gx.numpy()


def train_bwd_reference(inp, c, with_ste, dtype):
    """backward of the training quantiser: the adjoint of xn is gs + (xn - q) (g_loss c 2 / numel) -- straight-through plus the
    commitment term c mean((q - xn)^2) -- and goes through the l2-normalise backward at x"""
    T = lambda k: torch.tensor(inp[k], dtype=dtype)
    g = (T('xn') - T('q')) * (ROW_GL * F(c) * 2.0 / inp['x'].size)
    if with_ste:
        g = T('gs') + g
    return l2_bwd_reference(inp['x'], g.numpy(), dtype)


def row_sums(x):
    return (np.asarray(x, np.float64) ** 2).sum(1)


# ----------------------------------------------------------------------------------- numpy float32 statements (bit-exact kernels)
def ste_loss_bwd_f32(x, q, gs, gl):
    """gs + (x - q) * (gl * float32(2 / numel)), every step rounded"""
    t = f32(gl) * f32(2.0 / x.size)
    o = (x - q) * t
    o = o if gs is None else gs + o
    assert o.dtype == f32
    return o


def clip_preserve_f32(x, lo, hi):
    """x + (clip(x) - x): NaN stays NaN, +-inf becomes inf - inf = NaN, as in the statement"""
    with np.errstate(invalid='ignore'):
        return x + (np.clip(x, f32(lo), f32(hi)) - x)


def ks_split_fwd_f32(bc, ks):
    """-> (albedo, spec); ks [n, 1] broadcasts over the channels"""
    return (f32(1.0) - ks) * bc, ks * bc


def ks_split_bwd_f32(bc, ks, g_alb, g_spec):
    """-> (g_basecolor, g_ks); an absent gradient counts as zeros; a one-channel ks sums its three channels left to right"""
    ga = np.zeros_like(bc) if g_alb is None else g_alb
    gs = np.zeros_like(bc) if g_spec is None else g_spec
    g_bc = ga * (f32(1.0) - ks) + gs * ks
    gk = gs * bc - ga * bc
    if ks.shape[1] == 1:
        gk = ((gk[:, 0] + gk[:, 1]) + gk[:, 2])[:, None]
    assert g_bc.dtype == f32 and gk.dtype == f32
    return g_bc, gk


def loss_total_f32(terms, vqloss, sim, use_chr, use_smooth, use_lambert):
    """((((rgb + vqrgb) + vqloss) [+ chr]) [+ smooth]) [+ sim]) [+ lambert], left to right"""
    l = (terms[:, 0] + terms[:, 1]) + f32(vqloss)
    if use_chr:
        l = l + terms[:, 2]
    if use_smooth:
        l = l + terms[:, 3]
    if sim is not None:
        l = l + f32(sim)
    if use_lambert:
        l = l + terms[:, 4]
    assert l.dtype == f32
    return l
