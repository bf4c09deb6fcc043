"""Inputs, float32 / float64 references and the error yardstick of the per-kernel tests (tests/test_gpu_composite_kernels.py,
tests/test_gpu_shade_kernels.py, tests/test_gpu_ray_kernels.py).  Everything here runs on the CPU from the oracles alone, so the
conditions those tests rest on (no reference NaN, both precisions on the same side of every kink) are checked without a GPU too
(tests/test_kernel_cases.py)."""
import math

import numpy as np
import torch

from oracle import decomp as od
from oracle import geo as og

RADIUS = 1.0
MARGIN = 1e-3
PROFILES = ('crossing', 'miss', 'saturated', 'near_saturated', 'plus5', 'two_crossings', 'zero_grads')
NEAR_SAT_ALPHAS = (0.9, 0.99, 0.998)


# ---------------------------------------------------------------------------------------------------------------- yardstick
def yardstick(hip, ref32, ref64, f_max=3.0, f_rms=2.0):
    """The project's accuracy scheme (tests/test_gpu_decomp.py): a kernel output must be as close to the float64 statement as the
    float32 evaluation of the same statement is, max error within f_max x, rms within f_rms x, with a floor of 8 float32 epsilons of
    the tensor's largest entry for the cases where the float32 reference happens to be exact.
    -> dict(e_hip, e_ref, bound, rms_hip, rms_ref, rms_bound, ok)."""
    hip, ref32, ref64 = (np.asarray(a, np.float64) for a in (hip, ref32, ref64))
    assert hip.shape == ref64.shape == ref32.shape, (hip.shape, ref32.shape, ref64.shape)
    assert np.isfinite(ref64).all() and np.isfinite(ref32).all(), 'reference is not finite'
    if hip.size == 0:
        return dict(e_hip=0.0, e_ref=0.0, bound=0.0, rms_hip=0.0, rms_ref=0.0, rms_bound=0.0, ok=True)
    floor = 8.0 * 2.0 ** -24 * float(np.abs(ref64).max())
    rms = lambda e: float(np.sqrt((e ** 2).mean()))
    eh, er = np.abs(hip - ref64), np.abs(ref32 - ref64)
    eh = np.where(np.isfinite(hip), eh, np.inf)
    r = dict(e_hip=float(eh.max()), e_ref=float(er.max()), rms_hip=rms(eh), rms_ref=rms(er))
    r['bound'] = max(f_max * r['e_ref'], floor)
    r['rms_bound'] = max(f_rms * r['rms_ref'], floor)
    r['ok'] = r['e_hip'] <= r['bound'] and r['rms_hip'] <= r['rms_bound']
    return r


class Report:
    """Collects every (case, tensor) comparison of one test, so that a failing run shows all its figures, not the first."""

    def __init__(self, test):
        self.test, self.bad = test, []

    def check(self, key, hip, ref32, ref64, **kw):
        from tests.gpu_util import record_observed
        r = yardstick(hip, ref32, ref64, **kw)
        record_observed(self.test, key, r['e_hip'], r['bound'])
        record_observed(self.test, key + '#ref32', r['e_ref'], r['bound'])
        if not r['ok']:
            self.bad.append((key, r))
        return r

    def exact(self, key, hip, want):
        hip, want = np.asarray(hip), np.asarray(want)
        if hip.shape != want.shape or not np.array_equal(hip, want):
            n_bad = int((hip != want).sum()) if hip.shape == want.shape else -1
            self.bad.append((key, f'{n_bad} of {want.size} elements differ (exact comparison)'))

    def finish(self):
        assert not self.bad, '\n'.join(f'{k}: {v}' for k, v in self.bad)


# ---------------------------------------------------------------------------------------------------------------- compositing
def composite_inputs(B, n, inv_s, shift=0, seed=0):
    """float32 inputs of the compositing kernels: ray r follows PROFILES[(r + shift) % 7].  mid_z / dists come from sorted uniform
    depths in [2, 6]; the gradient vector of every sample is built from a drawn `true_cos` kept MARGIN away from the kinks of
    iter_cos (0 and 1), and mid-points closer than MARGIN to the radius tests are moved along the ray.  -> dict of numpy arrays."""
    rng = np.random.default_rng(1000 * seed + 7 * n + B)
    prof = (np.arange(B) + shift) % len(PROFILES)
    o = np.array([[0.0, 0.0, 4.0]]) + rng.uniform(-0.05, 0.05, (B, 3))
    tgt = np.concatenate([rng.uniform(-0.6, 0.6, (B, 2)), np.zeros((B, 1))], 1)
    d = tgt - o
    ph = rng.uniform(0, 2 * np.pi, B)
    miss = prof == PROFILES.index('miss')
    d[miss] = np.stack([np.sin(0.6) * np.cos(ph), np.sin(0.6) * np.sin(ph), -np.cos(0.6) * np.ones(B)], -1)[miss]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = o.astype(np.float32)
    z = np.sort(rng.uniform(2.0, 6.0, (B, n)).astype(np.float32), 1)
    dists = np.concatenate([z[:, 1:] - z[:, :-1], np.full((B, 1), 4.0 / max(n, 1), np.float32)], 1).astype(np.float32)
    mid_z = (z + dists * np.float32(0.5)).astype(np.float32)
    # keep every mid-point MARGIN away from both radius tests (judged in float64 on the float32 inputs)
    for _ in range(50):
        r = np.linalg.norm(o.astype(np.float64)[:, None] + d.astype(np.float64)[:, None] * mid_z.astype(np.float64)[..., None], axis=-1)
        bad = (np.abs(r - RADIUS) < 2 * MARGIN) | (np.abs(r - 1.1 * RADIUS) < 2 * MARGIN)
        if not bad.any():
            break
        mid_z = np.where(bad, mid_z + np.float32(0.013), mid_z).astype(np.float32)
    assert not bad.any()
    t = (mid_z - 2.0) / 4.0
    sdf = np.zeros((B, n), np.float32)
    tc = rng.uniform(-1.3, 1.3, (B, n))
    tc = np.where(np.abs(tc) < 0.01, 0.01, tc)
    tc = np.where(np.abs(tc - 1.0) < 0.01, 1.01, tc)
    zero_g = np.zeros((B, n), bool)
    k0 = max(0, min(n - 3, (n // 2) // 4 * 4 + 2))           # the nearly saturated samples straddle a lane boundary (4 items per lane)
    for r_ in range(B):
        p = PROFILES[prof[r_]]
        if p == 'crossing':
            sdf[r_] = 0.4 - 0.8 * t[r_] + rng.normal(0, 0.01, n)
            tc[r_] = -np.abs(tc[r_])
        elif p == 'miss':
            sdf[r_] = rng.normal(0.0, 0.3, n)
        elif p == 'saturated':
            sdf[r_] = -5.0
        elif p == 'near_saturated':
            sdf[r_] = np.where(np.arange(n) < k0, 0.3, -0.3)
            for j, a in enumerate(NEAR_SAT_ALPHAS):
                if k0 + j < n:
                    # sdf = 0, true_cos = -1 to rounding, far from both kinks (iter_cos = -1 at every anneal ratio): alpha = 1 - exp(-inv_s dist) up to the 1e-5 terms
                    sdf[r_, k0 + j] = 0.0
                    tc[r_, k0 + j] = -1.0
                    dists[r_, k0 + j] = -math.log(1.0 - a) / min(max(inv_s, 1e-6), 1e6)
        elif p == 'plus5':
            sdf[r_] = 5.0
        elif p == 'two_crossings':
            sdf[r_] = 0.25 * np.cos(4 * np.pi * t[r_])
        else:
            sdf[r_] = np.convolve(rng.normal(0.0, 0.2, n + 8), np.ones(9) / 9.0, 'valid')
            zero_g[r_, rng.integers(0, n, 3)] = True
    zero_g[prof == 0, n // 3] = True
    # gradient vector: true_cos * d + a perpendicular part (so that |g| != 1 and the eikonal term is live)
    a = rng.normal(size=(B, n, 3))
    d64 = d.astype(np.float64)[:, None, :]
    perp = a - (a * d64).sum(-1, keepdims=True) * d64
    perp = perp / np.linalg.norm(perp, axis=-1, keepdims=True) * rng.uniform(0.2, 1.2, (B, n, 1))
    grad = tc[..., None] * d64 + perp
    grad[zero_g] = 0.0
    return dict(rays_o=o, rays_d=d, mid_z=mid_z, dists=dists.astype(np.float32), sdf=sdf, grad=grad.astype(np.float32),
                rgb=rng.uniform(0, 1, (B, n, 3)).astype(np.float32), inv_s=np.array([inv_s], np.float32), profile=prof, k0=k0,
                g_color=rng.normal(size=(B, 3)).astype(np.float32), g_weight_sum=rng.normal(size=(B,)).astype(np.float32),
                g_weights=rng.normal(size=(B, n)).astype(np.float32), g_gradient_error=rng.normal(size=(1,)).astype(np.float32))


ADJOINT_SETS = {'all': ('g_color', 'g_weight_sum', 'g_weights', 'g_gradient_error'), 'color': ('g_color',),
                'weight_sum': ('g_weight_sum',), 'weights': ('g_weights',), 'gradient_error': ('g_gradient_error',)}


def composite_reference(inp, car, bg, dtype, adjoints=()):
    """oracle.geo.composite in `dtype` on the float32 inputs; for every entry of `adjoints` (keys of ADJOINT_SETS) the autograd
    adjoints of loss = <g_color, color> + <g_weight_sum, weight_sum> + <g_weights, weights> + g_gradient_error * gradient_error
    restricted to that set.  -> (forward dict of numpy arrays, {adjoint set: (g_sdf, g_grad, g_rgb, g_inv_s)})."""
    T = lambda k: torch.tensor(inp[k], dtype=dtype)
    sdf, grad, rgb, inv_s = (T(k).requires_grad_(True) for k in ('sdf', 'grad', 'rgb', 'inv_s'))
    B, n = inp['mid_z'].shape
    bgt = None if bg is None else torch.tensor(bg, dtype=dtype).reshape(1, 3)
    c = og.composite(sdf, grad, rgb, inv_s.reshape(()), T('mid_z'), T('dists'), T('rays_o'), T('rays_d'), RADIUS, car, bgt)
    fwd = {k: c[k].detach().numpy() for k in ('color', 'weights', 'cdf', 'inside_sphere', 'surf', 'depth', 'weight_sum', 'weight_max',
                                              'alpha', 'raw_alpha', 'gerr_num', 'gerr_den', 'relax', 'true_cos', 'pts_r')}
    outs = {}
    for name in adjoints:
        on = ADJOINT_SETS[name]
        loss = 0.0
        if 'g_color' in on:
            loss = loss + (T('g_color') * c['color']).sum()
        if 'g_weight_sum' in on:
            loss = loss + (T('g_weight_sum') * c['weight_sum'].reshape(B)).sum()
        if 'g_weights' in on:
            loss = loss + (T('g_weights') * c['weights']).sum()
        if 'g_gradient_error' in on:
            loss = loss + T('g_gradient_error')[0] * c['gradient_error']
        g = torch.autograd.grad(loss, (sdf, grad, rgb, inv_s), retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(g, (sdf, grad, rgb, inv_s))]
        outs[name] = tuple(gi.numpy() for gi in g)
    return fwd, outs


def branch_indicators(fwd):
    """Which side of each kink of the compositing statement every sample is on."""
    tc, r = fwd['true_cos'], fwd['pts_r']
    return np.stack([tc < 0.0, -tc * 0.5 + 0.5 > 0.0, r < RADIUS, r < RADIUS * 1.1, fwd['raw_alpha'] < 0.0, fwd['raw_alpha'] > 1.0])


def composite_margins_ok(inp, f64):
    """The margins the inputs were built with, re-measured on the float64 reference.  Samples whose gradient vector is exactly zero
    have true_cos == 0.0 exactly in every precision (the sub-gradient there is 0 in torch and in the kernel alike)."""
    tc, r = f64['true_cos'], f64['pts_r']
    zg = ~inp['grad'].any(-1)
    ok_tc = ((np.abs(tc) >= MARGIN) & (np.abs(tc - 1.0) >= MARGIN)) | (zg & (tc == 0.0))
    ok_r = (np.abs(r - RADIUS) >= MARGIN) & (np.abs(r - 1.1 * RADIUS) >= MARGIN)
    return bool(ok_tc.all() and ok_r.all())


# ---------------------------------------------------------------------------------------------------------------- shading
LIGHT_GRIDS = {256: (8, 32), 512: (16, 32), 1024: (16, 64)}
EDGES = ('rough0', 'rough1', 'rough002', 'spec0', 'spec1', 'flip', 'grazing', 'all_behind', 'lvis0', 'zero_gsum')


def shade_inputs(N, L, n_sets, with_lvis, shift=0, seed=0):
    """float32 inputs of the shading kernels with the edge points of EDGES mixed in: point i is edge (i + shift) % 10 for
    i < min(N, 10) (every edge once N >= 10).  The two material sets are different draws; edges touch both."""
    rng = np.random.default_rng(100 * seed + N + L)
    pts = od.make_points(N, seed=seed + 3, lvis=with_lvis, n_lights=L)
    xyz, normal, rayo = pts['xyz'].copy(), pts['normal'].copy(), pts['rayo'].copy()
    lvis = pts['lvis'].copy() if with_lvis else None
    mats = [[rng.uniform(0, 1, (N, 3)).astype(np.float32), rng.uniform(0, 1, (N, 3)).astype(np.float32),
             rng.uniform(0.05, 1, (N, 1)).astype(np.float32)] for _ in range(n_sets)]
    g_sums = [rng.normal(size=(N, 3)).astype(np.float32) for _ in range(n_sets)]
    edge = np.full(N, -1)
    for i in range(min(N, len(EDGES))):
        e = EDGES[(i + shift) % len(EDGES)]
        edge[i] = (i + shift) % len(EDGES)
        for s in range(n_sets):
            if e == 'rough0':
                mats[s][2][i] = 0.0
            elif e == 'rough1':
                mats[s][2][i] = 1.0
            elif e == 'rough002':
                mats[s][2][i] = 0.02
            elif e == 'spec0':
                mats[s][1][i] = 0.0
            elif e == 'spec1':
                mats[s][1][i] = 1.0
            elif e == 'zero_gsum':
                g_sums[s][i] = 0.0
        if e == 'flip':
            normal[i] = -normal[i]
        elif e == 'grazing':                                  # view direction (0, 0, 1), normal (1, 0, 0): v.n == 0.0 in every precision
            xyz[i], rayo[i], normal[i] = (0.5, 0.0, 1.0), (0.5, 0.0, 4.0), (1.0, 0.0, 0.0)
        elif e == 'all_behind':                               # outside the light sphere, facing away from it: every cosine < 0
            xyz[i], rayo[i], normal[i] = (0.0, 0.0, 1000.0), (0.0, 0.0, 1004.0), (0.0, 0.0, 1.0)
            if lvis is not None:
                lvis[i] = 1.0
        elif e == 'lvis0' and lvis is not None:
            lvis[i] = 0.0
    lxyz, lareas = od.gen_light_xyz(*LIGHT_GRIDS[L])
    light = rng.uniform(0, 1, (L, 3)).astype(np.float32)
    return dict(xyz=xyz, normal=normal, rayo=rayo, lvis=lvis, mats=mats, g_sums=g_sums, edge=edge,
                lxyz=lxyz.reshape(-1, 3).astype(np.float32), lareas=lareas.reshape(-1).astype(np.float32), light=light)


def shade_reference(inp, dtype, grads=True, gamma=None, clip=False, light=None, chunk=256):
    """oracle.decomp's shading statements in `dtype`, `chunk` points at a time (the [N, L, 3] intermediates of 4,000 points x 1,024
    lights in float64 would not fit otherwise; g_light is accumulated over the chunks).  clip=False: the plain sums over the lights.
    -> dict(rgb=[per set], rgb_diff, rgb_spec, normal, g=[(g_albedo, g_spec, g_rough) per set], g_light)."""
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    N = inp['xyz'].shape[0]
    n_sets = len(inp['mats'])
    lxyz, lareas = T(inp['lxyz']), T(inp['lareas'])
    light_t = T(inp['light'] if light is None else light).requires_grad_(grads)
    out = dict(rgb=[[] for _ in range(n_sets)], rgb_diff=[], rgb_spec=[], normal=[], g=[[[], [], []] for _ in range(n_sets)])
    g_light = torch.zeros_like(light_t)
    for s0 in range(0, N, chunk):
        sl = slice(s0, min(N, s0 + chunk))
        xyz, normal, rayo = T(inp['xyz'][sl]), T(inp['normal'][sl]), T(inp['rayo'][sl])
        lvis = None if inp['lvis'] is None else T(inp['lvis'][sl])
        surf2l, surf2c = od.calc_ldir(lxyz, xyz), od.calc_vdir(rayo, xyz)
        n_pred = od.normal_correct(normal, surf2c)
        out['normal'].append(n_pred.numpy())
        loss, leaves = 0.0, []
        for s in range(n_sets):
            a, f0, r = (T(m[sl]).requires_grad_(grads) for m in inp['mats'][s])
            leaves += [a, f0, r]
            brdf, bs, bd = od.get_brdf(surf2l, surf2c, n_pred, a, r, f0)
            rgb = od.render_integrate(brdf, surf2l, n_pred, lareas, light_t, lvis, gamma, clip=clip)
            out['rgb'][s].append(rgb.detach().numpy())
            if s == 0:
                out['rgb_diff'].append(od.render_integrate(bd, surf2l, n_pred, lareas, light_t, lvis, gamma, clip=clip).detach().numpy())
                out['rgb_spec'].append(od.render_integrate(bs, surf2l, n_pred, lareas, light_t, lvis, gamma, clip=clip).detach().numpy())
            if grads:
                loss = loss + (T(inp['g_sums'][s][sl]) * rgb).sum()
        if grads:
            g = torch.autograd.grad(loss, leaves + [light_t])
            g_light = g_light + g[-1]
            for s in range(n_sets):
                for j in range(3):
                    out['g'][s][j].append(g[3 * s + j].numpy())
    cat = lambda l: np.concatenate(l, 0)
    res = dict(rgb=[cat(x) for x in out['rgb']], rgb_diff=cat(out['rgb_diff']), rgb_spec=cat(out['rgb_spec']), normal=cat(out['normal']))
    if grads:
        res['g'] = [tuple(cat(x) for x in gs) for gs in out['g']]
        res['g_light'] = g_light.numpy()
    return res


def rough0_limit(inp, ref):
    """At rough == 0 exactly the statement's autograd is 0 * inf: torch (like the framework the statement comes from) differentiates
    sqrt|a2 + (1 - a2) c^2| at 0 for every light with c = 0 and returns NaN for g_rough.  The derivative itself exists there:
    d loss / d a2 is finite and d a2 / d rough = 4 rough^3 = 0, so g_rough = 0 -- the value this puts in place of the NaN.  Returns
    the number of replaced entries; every one of them must sit at a rough == 0 point, and no other adjoint may be non-finite."""
    n_fixed = 0
    for s, (ga, gs, gr) in enumerate(ref['g']):
        nan = ~np.isfinite(gr)
        assert not (nan & (inp['mats'][s][2] != 0.0)).any(), 'reference g_rough is not finite away from rough == 0'
        assert np.isfinite(ga).all() and np.isfinite(gs).all()
        gr[nan] = 0.0
        n_fixed += int(nan.sum())
    assert np.isfinite(ref['g_light']).all()
    return n_fixed


# ---------------------------------------------------------------------------------------------------------------- per-ray sampling
def merge_inputs(B, n, m, seed=0):
    """Sorted old depths [B, n] and UNSORTED new depths [B, m] on a coarse grid, so that equal depths occur inside the old samples,
    inside the new ones and across both; sdf values are all distinct (they tell which of two equal depths went where)."""
    rng = np.random.default_rng(50 * seed + 3 * n + m + B)
    grid = max(2, (n + m) // 2)
    z = np.sort(2.0 + 4.0 * rng.integers(0, grid, (B, n)) / grid, 1).astype(np.float32)
    z_new = (2.0 + 4.0 * rng.integers(0, grid, (B, m)) / grid).astype(np.float32)
    copy = rng.uniform(size=(B, m)) < 0.3                                            # ties across old and new for certain
    z_new = np.where(copy, np.take_along_axis(z, rng.integers(0, n, (B, m)), 1), z_new).astype(np.float32)
    if m >= 2:
        z_new[:, m - 1] = z_new[:, 0]                                                # and one inside the new samples
    sdf = rng.permutation(B * (n + m)).astype(np.float32).reshape(B, n + m)
    return z, sdf[:, :n].copy(), z_new, sdf[:, n:].copy()


def merge_reference(z, sdf, z_new, sdf_new):
    """cat + stable sort (old before new on equal keys, new ones in input order) + gather, on the CPU."""
    zc = torch.cat([torch.tensor(z), torch.tensor(z_new)], -1)
    zs, idx = torch.sort(zc, dim=-1, stable=True)
    return zs.numpy(), torch.gather(torch.cat([torch.tensor(sdf), torch.tensor(sdf_new)], -1), -1, idx).numpy()


UPSAMPLE_GRID = [(n, m, s) for n in (2, 3, 65, 129, 200, 256) for m in (1, 16, 64) for s in (64.0, 512.0)]
UPSAMPLE_R_LIMIT = 2.0


def upsample_case(n, n_new, inv_s, B=13):
    """The eight profiles of oracle.geo.make_upsample_profiles tiled to B rays (B = 13: not a multiple of the four rays of a
    workgroup), the float32 and float64 oracle depths, and per ray whether the two oracles agree to 1e-5 on every new depth (the
    inverse CDF is steep where a section's weight is near zero: only rays the oracles agree on are bounded)."""
    o, d, z, sdf = (np.asarray(a)[np.arange(B) % 8] for a in og.make_upsample_profiles(n))
    T = lambda a, dt: torch.tensor(a, dtype=dt)
    ref = {dt: og.up_sample(T(o, dt), T(d, dt), T(z, dt), T(sdf, dt), UPSAMPLE_R_LIMIT, n_new, inv_s).numpy()
           for dt in (torch.float32, torch.float64)}
    agree = np.abs(ref[torch.float32].astype(np.float64) - ref[torch.float64]).max(1) <= 1e-5
    return dict(o=o, d=d, z=z, sdf=sdf, ref32=ref[torch.float32], ref64=ref[torch.float64], agree=agree)
