"""The kernels of the geometry training step on their own, one network shape and one engine at a time: vqn_neus_train_fwd / _x3,
vqn_neus_train_bwd / _x3 (and the weight-gradient contraction behind them) and the interpreted prog_fwd / prog_cbwd / prog_sbwd,
through NeusCoreFunction at explicit points, against the float64 autograd of the statement in tests/neus_train_cases.py (shapes,
points, references and bounds: there; what they rest on: tests/test_neus_train_cases.py, on the CPU).

Per (shape, engine), over P in {1, 33, 65, 161} and the adjoint variants:
  * the entry points of the engine ran, once each, and no other engine's did (exact names);
  * sdf, n, rgb within kernel_cases.yardstick of the float64 statement (3x max / 2x rms of the float32 statement's own error, floor
    8 eps); every parameter gradient within the pooled form of the same (neus_train_cases.pooled_gradient_check);
  * exact relations: zero adjoints give zero gradients; a loss that does not touch n and sdf (the Function sees None) gives the
    bits of explicit zero adjoints; the outputs of the first 33 of 65 points are the first 33 rows of the 65-point run;
  * alloc_tensors filled with NaN and with zeros (P = 33, 161): everything finite, and the same bits under both fills -- whatever
    the weight-gradient contraction reads was written by the kernels."""
import pytest
import torch

from tests import neus_train_cases as nc
from tests.gpu_util import launches, record_observed
from tests.kernel_cases import yardstick

pytestmark = pytest.mark.gpu

NAME = 'test_neus_train_kernels'
# key suffix of the figures that are NOT kernel measurements: the float32 statement's own error against float64 (torch on the CPU),
# recorded next to the bound it produces
REF32 = '#float32_statement_own_error'
_ENGINES = {}
_COMPARISONS = {}


class Miss(Exception):
    """a comparison outside its float32 bound (and inside its cap): the only thing the expected-failure marks below accept"""


# Upper limits of the comparisons listed in KNOWN_MISSES, none of them taken from what the kernels give: a parameter gradient by the
# bound the model-level test already holds the full-size networks' gradients to against the reference (the largest difference over the
# tensor's largest entry), sdf / n / rgb by the absolute tolerances test_render_core_all_keys holds the same three quantities to.
def _caps():
    from tests.test_gpu_neus_render import GRAD_BOUNDS
    return dict(grad=GRAD_BOUNDS['full'], sdf=2e-5, n=3e-4, rgb=2e-4)


# Comparisons that miss the float32 bound: key -> (max error / bound, rms error / bound) of an MI355X run (all figures:
# profiles/observed_errors_neus_train_kernels.json).  Each is ONE tensor of one case; every other tensor of the same case stays asserted.
#
#  * <shape>/<engine>/P1/sdf and w288/*/P65/n -- these measure the yardstick, not the kernels.  The bound is 3 x the float32 statement's
#    error on the very same one (or 195) numbers, and here torch's float32 lands far closer to float64 than float32 arithmetic promises
#    (sdf at one point: 4.5e-10 .. 9.8e-8, where the same statement is 5e-7 .. 1.1e-6 off at every larger P), so the bound sits at or
#    near its 8-eps floor.  The kernels' errors there (8.8e-8 .. 3.8e-7) are below the float32 statement's own error at P >= 33 of
#    the same shape, and every engine, the interpreter included, misses alike.  The float32 reference is evaluated when the test runs
#    (one thread, so the core count does not move it): another BLAS build can move these bounds by more than the 1.01 x .. 1.75 x the
#    kernels miss them by, and a mark that then passes has to be taken off this list.
#
# (The exact-split backward used to be on this list with 39 g_rgb-only gradient tensors: with one accumulator per image it was not odd in
# its adjoints.  It now runs two, as the forward does, and meets the bound: csrc/neus_train_bwd_x3.hip bwd_nacc, DESIGN.md.)
KNOWN_MISSES = {
    'shipped/x3/P1/sdf': (1.45, 1.45),
    'shipped/fused/P1/sdf': (1.45, 1.45),
    'shipped/prog/P1/sdf': (1.45, 1.45),
    'w200/x3/P1/sdf': (1.74, 1.76),
    'w200/fused/P1/sdf': (1.04, 1.05),
    'w200/prog/P1/sdf': (1.74, 1.76),
    'w200/fwd_x3+bwd_fused/P1/sdf': (1.74, 1.76),
    'w200/fwd_fused+bwd_x3/P1/sdf': (1.04, 1.05),
    'w129/prog/P1/sdf': (1.29, 1.31),
    'w288/default/P65/n': (1.01, 0.37),
}


def _why(key):
    mx, rms = KNOWN_MISSES[key]
    kind = 'the float32 statement is unusually exact on these few numbers (the yardstick, not the kernel)'
    return f'{kind}: max {mx:.2f} x, rms {rms:.2f} x the bound'


def _engine(shape):
    """one NeusTrainEngine per shape for the whole module, and the float32 effective weights as CUDA tensors"""
    if shape not in _ENGINES:
        eng = nc.build_engine(shape, 'cuda')
        _ENGINES[shape] = (eng, [[t.cuda() for t in ts] for ts in nc.effective_params(shape)])
    return _ENGINES[shape]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a) and set(a) == set(b)


def _run(shape, engine, x, dirs, adj):
    """forward + one backward of L = <rgb, g_rgb> (+ <n, g_n>) (+ <sdf, g_sdf>) -> dict of CUDA tensors: sdf, n, rgb and every
    gradient by name; asserts that exactly the engine's entry points ran, once each"""
    from vqnerf_release_amd.geo.train_programs import NeusCoreFunction
    eng, params = _engine(shape)
    leaves = [t.clone().requires_grad_(True) for ts in params for t in ts]
    with launches() as rec:
        sdf, n, rgb = NeusCoreFunction.apply(eng, x, dirs, *leaves)
        nc.loss_of(sdf, n, rgb, adj).backward()
    ran, not_ran = nc.expected_entries(engine)
    assert all(rec.counts.get(k) == 1 for k in ran) and not any(k in rec.counts for k in not_ran), (shape, engine, rec.counts)
    assert any(k.startswith('vqn_wgrad_partials') for k in rec.counts)
    out = dict(sdf=sdf.detach(), n=n.detach(), rgb=rgb.detach())
    assert out['sdf'].shape == (x.shape[0], 1) and out['n'].shape == (x.shape[0], 3) and out['rgb'].shape == (x.shape[0], 3)
    for k, t in zip(nc.grad_names(shape), leaves):
        assert t.grad is not None and t.grad.shape == t.shape, k
        out[k] = t.grad.detach()
    return out


def _record(key, r, kinds=(('', 'e_hip', 'e_ref', 'bound'), ('#rms', 'rms_hip', 'rms_ref', 'rms_bound'))):
    for sfx, h, e, b in kinds:
        record_observed(NAME, key + sfx, r[h], r[b])
        record_observed(NAME, key + sfx + REF32, r[e], r[b])
    record_observed(NAME, key + '#ratio', r['e_hip'] / max(r['e_ref'], 1e-300), r['bound'] / max(r['e_ref'], 1e-300))


def _case(shape, engine, monkeypatch):
    """Everything of one (shape, engine): the runs over P and the adjoint variants with their exact relations (asserted here), and
    the accuracy comparisons -> {key: (ok, figures)}, key = shape/engine/P<P>/<sdf|n|rgb> for an output and
    shape/engine/P<P>/grads_<all|rgb>/<tensor> for a parameter gradient (its bound pooled over the tensors of the case).  Computed once per module run."""
    if (shape, engine) in _COMPARISONS:
        return _COMPARISONS[shape, engine]
    nc.select(monkeypatch, engine)
    eng, _ = _engine(shape)
    fmode, bmode = eng.forward_mode(), eng.backward_mode()
    assert (fmode, bmode) == nc.MODES[engine]
    if shape == 'w288' and engine == 'default':
        # 9 tiles under the default environment: all three interpreted programs (vqn_neus_train_fwd refuses 9 tiles; a forward mode
        # that selected it would raise in _run below), and _run asserts that no fused entry ran beside them
        ran, _ = nc.expected_entries(engine)
        assert ran == ('vqn_tile_program:prog_fwd', 'vqn_tile_program:prog_cbwd', 'vqn_tile_program:prog_sbwd')
    # what the fused backward is handed when the loss does not touch n and sdf
    seen = []
    for meth in ('run_fused_backward', 'run_fused_backward_x3'):
        def spy(flat, T, P, g_rgb, g_n, g_sdf, _orig=getattr(eng, meth)):
            seen.append((g_n is None, g_sdf is None))
            return _orig(flat, T, P, g_rgb, g_n, g_sdf)
        monkeypatch.setattr(eng, meth, spy)
    cmp = {}
    for P in nc.POINTS:
        ref = nc.reference(shape, P)
        x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
        g_rgb, g_n, g_sdf = (ref[k].cuda() for k in ('g_rgb', 'g_n', 'g_sdf'))
        zero = lambda t: torch.zeros_like(t)
        got = {'all': _run(shape, engine, x, dirs, (g_rgb, g_n, g_sdf))}
        del seen[:]
        got['rgb'] = _run(shape, engine, x, dirs, (g_rgb, None, None))
        assert seen == ([(True, True)] if bmode is not None else []), seen
        got['rgb0'] = _run(shape, engine, x, dirs, (g_rgb, zero(g_n), zero(g_sdf)))
        assert seen[-1:] == ([(False, False)] if bmode is not None else [])
        got['zero'] = _run(shape, engine, x, dirs, (zero(g_rgb), zero(g_n), zero(g_sdf)))
        tag = f'{shape}/{engine}/P{P}'
        # ---- exact relations
        for v in ('rgb', 'rgb0', 'zero'):                        # one forward, whatever the loss
            assert all(torch.equal(_bits(got[v][k]), _bits(got['all'][k])) for k in ('sdf', 'n', 'rgb')), (tag, v)
        for k in nc.grad_names(shape):
            assert not got['zero'][k].any(), f'{tag}: {k} is not exactly zero under zero adjoints'
        assert _same_bits(got['rgb'], got['rgb0']), f'{tag}: absent adjoints differ from explicit zeros'
        # ---- accuracy of sdf, n, rgb
        for k in ('sdf', 'n', 'rgb'):
            r = yardstick(got['all'][k].cpu().numpy(), ref['f32'][k], ref['f64'][k])
            _record(f'{tag}/{k}', r)
            cmp[f'{tag}/{k}'] = (r['ok'], r)
        # ---- accuracy of every parameter gradient, bound pooled over the case's tensors
        for v in ('all', 'rgb'):
            hip = {k: got[v][k].cpu().numpy() for k in nc.grad_names(shape)}
            res = nc.pooled_gradient_check(hip, ref['f32']['grads'][v], ref['f64']['grads'][v])
            for k, t in res['tensors'].items():
                _record(f'{tag}/grads_{v}/{k}', dict(t, bound=res['bound'], rms_bound=res['rms_bound']))
            for k in nc.grad_names(shape):
                fig = dict(res['tensors'].get(k, {}), bound=res['bound'], rms_bound=res['rms_bound'])
                cmp[f'{tag}/grads_{v}/{k}'] = (k not in res['bad'], fig)
    # ---- the per-point outputs do not depend on how many points follow (the fused forwards)
    if fmode is not None:
        ref = nc.reference(shape, 65)
        x, dirs, g_rgb = ref['x'].cuda(), ref['dirs'].cuda(), ref['g_rgb'].cuda()
        full = _run(shape, engine, x, dirs, (g_rgb, None, None))
        head = _run(shape, engine, x[:33].contiguous(), dirs[:33].contiguous(), (g_rgb[:33], None, None))
        for k in ('sdf', 'n', 'rgb'):
            assert torch.equal(_bits(head[k]), _bits(full[k][:33])), f'{shape}/{engine}: {k} of the first 33 points of 65'
    for k, (ok, fig) in cmp.items():
        if not ok:
            print(f'[miss] {k}: {fig}')
    _COMPARISONS[shape, engine] = cmp
    return cmp


@pytest.mark.parametrize('shape,engine', nc.GPU_CASES, ids=[f'{s}-{e}' for s, e in nc.GPU_CASES])
def test_training_kernels_against_the_float64_statement(shape, engine, monkeypatch):
    cmp = _case(shape, engine, monkeypatch)
    assert len(cmp) == len(nc.POINTS) * (3 + 2 * len(nc.grad_names(shape)))
    bad = [(k, fig) for k, (ok, fig) in cmp.items() if not ok and k not in KNOWN_MISSES]
    assert not bad, '\n'.join(f'{k}: {v}' for k, v in bad)


@pytest.mark.parametrize('key', [pytest.param(k, marks=pytest.mark.xfail(strict=True, raises=Miss, reason=_why(k))) for k in KNOWN_MISSES])
def test_comparison_that_misses_the_float32_bound(key, monkeypatch):
    """The single comparisons of the test above that miss the float32 bound (KNOWN_MISSES: why, and by how much), each under a strict
    expected-failure mark that accepts nothing but that miss: the runs, their launch counts and exact relations, and the cap of the
    comparison are asserted outside it, and a comparison that starts to pass fails the suite until it is taken off the list."""
    shape, engine = key.split('/')[:2]
    ok, fig = _case(shape, engine, monkeypatch)[key]
    caps = _caps()
    if '/grads_' in key:
        assert fig['e_hip'] <= caps['grad'] and fig['rms_hip'] <= caps['grad'], f'{key}: beyond the cap {caps["grad"]}: {fig}'
    else:
        assert fig['e_hip'] <= caps[key.split('/')[-1]], f'{key}: beyond the cap: {fig}'
    if not ok:
        raise Miss(f'{key}: {fig}')


@pytest.mark.parametrize('shape,engine', nc.GPU_CASES, ids=[f'{s}-{e}' for s, e in nc.GPU_CASES])
def test_training_kernels_read_nothing_they_did_not_write(shape, engine, monkeypatch):
    """alloc_tensors hands out torch.empty memory.  Every tensor but X, DIRS and ONES filled with NaN, then with zeros, before use:
    all outputs and gradients are finite and bit for bit the same under both fills (the contraction sums in a fixed order)."""
    nc.select(monkeypatch, engine)
    eng, _ = _engine(shape)
    assert (eng.forward_mode(), eng.backward_mode()) == nc.MODES[engine]
    alloc = eng.alloc_tensors
    fill = [None]

    def filled(P, device):
        T = alloc(P, device)
        for k, t in T.items():
            if k not in ('X', 'DIRS', 'ONES'):
                t.fill_(fill[0])
        return T

    monkeypatch.setattr(eng, 'alloc_tensors', filled)
    for P in nc.POISON_POINTS:
        ref = nc.reference(shape, P)
        x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
        adj = tuple(ref[k].cuda() for k in ('g_rgb', 'g_n', 'g_sdf'))
        runs = {}
        for name, value in (('nan', float('nan')), ('zeros', 0.0)):
            fill[0] = value
            runs[name] = _run(shape, engine, x, dirs, adj)
        for k, t in runs['nan'].items():
            assert bool(torch.isfinite(t).all()), f'{shape}/{engine}/P{P}: {k} is not finite over NaN-filled tensors'
        diff = [k for k in runs['nan'] if not torch.equal(_bits(runs['nan'][k]), _bits(runs['zeros'][k]))]
        assert not diff, f'{shape}/{engine}/P{P}: {diff} depend on what the tensors held before'


@pytest.mark.parametrize('engine', ['x3', 'fused'])
def test_backward_is_the_same_under_one_workgroup_of_scratch(engine, monkeypatch):
    """The backward's grid is sized by its scratch (csrc/neus_launch.h: pair_grid over train_bwd_stash_bytes).  w160 at 161 points is
    three tile pairs: with the scratch the query asks for, three workgroups take one pair each; with exactly one workgroup's -- a fresh
    buffer of that size, handed to the entry in place of the wrapper's cached one -- a single workgroup walks all three.  Every tensor
    the backward writes, and every gradient behind them, has the same bits both ways."""
    from vqnerf_release_amd import _C
    shape, P = 'w160', 161
    nc.select(monkeypatch, engine)
    eng, _ = _engine(shape)
    mode = eng.backward_mode()
    assert mode == nc.MODES[engine][1] and (P + 31) // 32 == 6
    meth, query = {'x3': ('run_fused_backward_x3', 'vqn_neus_train_bwd_x3_scratch_bytes'),
                   'f32': ('run_fused_backward', 'vqn_neus_train_bwd_scratch_bytes')}[mode]
    ref = nc.reference(shape, P)
    x, dirs = ref['x'].cuda(), ref['dirs'].cuda()
    adj = tuple(ref[k].cuda() for k in ('g_rgb', 'g_n', 'g_sdf'))
    desc = eng._bwd_static(x.device, mode)[-1]
    per_wg = 2 * (int(desc[0]) + 1) * 4 * int(desc[6]) * 1024           # two images of S_0..S_{nL-1} and g_feat, 4 max_tiles KB each
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    assert _C._scratch_bytes(query, _C._host(desc)) == cus * per_wg and cus >= 3

    written, sizes = [], []
    orig = getattr(eng, meth)

    def spy(flat, T, Pn, g_rgb, g_n, g_sdf):
        orig(flat, T, Pn, g_rgb, g_n, g_sdf)
        names = ['DC%d' % l for l in range(eng.nC + 1)] + ['GOUTF', 'ED'] + ['UD%d' % (l + 1) for l in range(eng.nL)] + \
            ['AB%d' % l for l in range(eng.nL)]
        written.append({k: T[k].clone() for k in names})

    monkeypatch.setattr(eng, meth, spy)
    real_scratch = _C._scratch

    def scratch(tag, need, device, *a, **kw):
        if tag != 'bwd':
            return real_scratch(tag, need, device, *a, **kw)
        sizes.append(need)
        return torch.empty((small[0] or need,), dtype=torch.uint8, device=device)

    monkeypatch.setattr(_C, '_scratch', scratch)
    small = [None]
    full = _run(shape, engine, x, dirs, adj)
    small[0] = per_wg
    one = _run(shape, engine, x, dirs, adj)
    assert sizes == [cus * per_wg] * 2 and len(written) == 2
    diff = [k for k in written[0] if not torch.equal(_bits(written[0][k]), _bits(written[1][k]))]
    assert not diff, f'{shape}/{engine}: {diff} differ between {cus} workgroups\' scratch and one\'s'
    assert _same_bits(full, one)
