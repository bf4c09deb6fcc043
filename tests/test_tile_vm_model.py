"""The numpy model of the tile-program interpreter (tests/tile_vm_model.py) against torch float64 autograd, and the conditions the
GPU test (tests/test_gpu_tile_vm_ops.py) rests on: the four epilogues per activation on a 2-layer MLP, the posenc Jacobian and VJP,
the exactness of the integer cases, and that every case translates into a Program.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tile_vm_model as vm

TOL = 1e-12
ACTS = (vm.SOFTPLUS, vm.SIGMOID, vm.RELU, vm.NONE)


def _torch_act(a, x):
    if a == vm.SOFTPLUS:
        return F.softplus(x, beta=100, threshold=20)
    if a == vm.SIGMOID:
        return torch.sigmoid(x)
    return torch.relu(x) if a == vm.RELU else x


def _close(got, want, what):
    want = np.asarray(want, np.float64)
    err = float(np.max(np.abs(got - want)))
    assert err <= TOL * max(1.0, float(np.max(np.abs(want)))), f'{what}: {err:.3e}'


def _mlp_case(a, N=37):
    """x (5) -> h = act(W1 x + b1) (19) -> out = W2 h + b2 (7), as one program: forward, the reverse sweep for n = d<out, g>/dx, the
    tangent along v with its second-order source, the double-backward sweep."""
    rng = np.random.default_rng(5 + a)
    P = 32 * ((N + 31) // 32)
    s1 = 0.02 if a == vm.SOFTPLUS else 0.6                   # softplus: 100 a1 inside (-20, 20), where the output determines the derivative
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    mats = {'W1': f(19, 5) * np.float32(s1), 'W2': f(7, 19)}
    mats['W1T'], mats['W2T'] = mats['W1'].T.copy(), mats['W2'].T.copy()
    biases = {'W1': f(19) * np.float32(s1), 'W2': f(7)}
    tensors = {k: ('t', 1) for k in ('X', 'V', 'G', 'G2', 'U1', 'OUT', 'GH', 'NRM', 'UD', 'S', 'AB')}
    inputs = {k: np.where(np.arange(32)[:, None] < n, f(32, P), 0).astype(np.float32) for k, n in (('X', 5), ('V', 5), ('G', 7), ('G2', 7))}
    ld = lambda t, r, feats: [dict(op='alloc', name=r, feats=feats), dict(op='ld_t', t=t, dst=r, rows=vm.rows_for(feats))]
    g = lambda key, src, n_in, n_out, **kw: dict(dict(op='gemm', key=key, segs=[(src, n_in, 0)], out_feats=n_out, epi=vm.EPI_ACT, act=vm.NONE), **kw)
    ops = ld('X', 'x', 5) + [g('W1', 'x', 5, 19, act=a, bias='W1', store='U1', out='h'), g('W2', 'h', 19, 7, bias='W2', store='OUT')]
    ops += ld('G', 'g', 7) + [g('W2T', 'g', 7, 19, epi=vm.EPI_MUL_DACT, act=a, aux1='U1', store='GH', out='gh'), g('W1T', 'gh', 19, 5, store='NRM')]
    ops += ld('V', 'v', 5) + [g('W1', 'v', 5, 19, epi=vm.EPI_TANGENT, act=a, aux1='U1', aux2='GH', store='UD', store2='S')]
    ops += ld('G2', 'g2', 7) + [g('W2T', 'g2', 7, 19, epi=vm.EPI_BWD2, act=a, aux1='U1', aux2='S', store='AB')]
    return dict(name='mlp-' + vm.ACT_NAMES[a], N=N, n_waves=4, tensors=tensors, inputs=inputs, mats=mats, biases=biases, ops=ops,
                outputs=['U1', 'OUT', 'GH', 'NRM', 'UD', 'S', 'AB'])


@pytest.mark.parametrize('a', ACTS, ids=[vm.ACT_NAMES[a] for a in ACTS])
def test_the_four_epilogues_are_autograd_of_a_two_layer_mlp(a):
    case = _mlp_case(a)
    N = case['N']
    T, trace = vm.run_model(case)
    t64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    W1, W2, b1, b2 = (t64(case['mats']['W1']), t64(case['mats']['W2']), t64(case['biases']['W1']), t64(case['biases']['W2']))
    x = t64(case['inputs']['X'][:5, :N].T).requires_grad_(True)
    v, g, g2 = t64(case['inputs']['V'][:5, :N].T), t64(case['inputs']['G'][:7, :N].T), t64(case['inputs']['G2'][:7, :N].T)
    a1 = x @ W1.T + b1
    if a == vm.SOFTPLUS:
        assert float(a1.detach().abs().max()) * 100 < 20
    h = _torch_act(a, a1)
    out = h @ W2.T + b2
    gh, nrm = torch.autograd.grad((out * g).sum(), (a1, x), create_graph=True)          # reverse sweep: adjoint of a1, and n
    ud = torch.autograd.functional.jvp(lambda xx: _torch_act(a, xx @ W1.T + b1), x.detach(), v)[1]
    L2 = (nrm * v).sum()                                                             # <n, v>: its a1-gradient is the second-order source
    S = torch.autograd.grad(L2, a1, retain_graph=True, allow_unused=True)[0] if L2.requires_grad else None
    S = torch.zeros_like(a1) if S is None else S
    ab = torch.autograd.grad((out * g2).sum() + L2, a1, allow_unused=True)[0]         # double backward: first-order adjoint + source
    got = lambda n, k: T[n][0][:k, :N].T
    _close(got('U1', 19), h.detach(), 'ACT: hidden layer')
    _close(got('OUT', 7), out.detach(), 'ACT none + bias: output')
    _close(got('GH', 19), gh.detach(), 'MUL_DACT: reverse sweep')
    _close(got('NRM', 5), nrm.detach(), 'reverse sweep: d<out, g>/dx')
    _close(got('UD', 19), ud, 'TANGENT: JVP')
    _close(got('S', 19), S.detach(), 'TANGENT: second-order source')
    _close(got('AB', 19), ab.detach(), 'BWD2: double-backward sweep')
    # written sets: whole tiles, padding points and padded outputs included, as zero beyond N
    for n in case['outputs']:
        vals, written = T[n]
        assert written.all() and not np.isnan(vals).any() and (vals[:, N:] == 0).all()
    assert sum(1 for op, wr in trace if wr) == 6 and set(trace[2][1]) == {'U1'} and set(trace[10][1]) == {'UD', 'S'}


def test_softplus_past_the_threshold_is_the_identity_and_padded_outputs_hold_act_of_zero():
    x = np.array([0.2, 0.2001, 0.5, 3.0])
    assert np.array_equal(vm.act(vm.SOFTPLUS, x)[1:], x[1:]) and abs(vm.act(vm.SOFTPLUS, x)[0] - 0.2) < 1e-10
    case = vm.pair_case(vm.EPI_ACT, vm.SIGMOID)
    case['mats']['W'][40:] = 0
    case['biases']['W'][40:] = 0
    T, _ = vm.run_model(case)
    assert (T['Y'][0][40:, :33] == 0.5).all() and (T['Y'][0][:, 33:] == 0).all()


@pytest.mark.parametrize('n_freqs,scale', [(0, 1.0), (1, 1.0), (6, 1.0), (10, 0.5)])
def test_posenc_jacobian_and_vjp_are_autograd_of_the_embedding(n_freqs, scale):
    """x in float32 and scale a power of two: x * scale is exact, so the model's argument is autograd's.  The Jacobian is taken with
    respect to the SCALED argument (what the kernel computes: the callers fold the scale in elsewhere)."""
    case = vm.posenc_case(n_freqs, scale, 33)
    N, feats = 33, 3 + 6 * n_freqs
    T, _ = vm.run_model(case)
    xs = torch.tensor(case['inputs']['X'][:, :3].astype(np.float64) * scale, requires_grad=True)
    emb = torch.cat([xs] + [fn(xs * 2.0 ** k) for k in range(n_freqs) for fn in (torch.sin, torch.cos)], 1)
    assert emb.shape[1] == feats
    v = torch.tensor(case['inputs']['V'][:, :3].astype(np.float64))
    G = torch.tensor(case['inputs']['G'][:feats, :N].T.astype(np.float64))
    jvp = torch.autograd.functional.jvp(lambda z: torch.cat([z] + [fn(z * 2.0 ** k) for k in range(n_freqs) for fn in (torch.sin, torch.cos)], 1),
                                        xs.detach(), v)[1]
    vjp = torch.autograd.grad((emb * G).sum(), xs)[0]
    _close(T['E'][0][:feats, :N].T, emb.detach(), 'posenc')
    _close(T['ED'][0][:feats, :N].T, jvp, 'posenc JVP')
    _close(T['N'][0][:, :3], vjp, 'posenc VJP')
    rows = vm.rows_for(feats)
    for n in ('E', 'ED'):                       # written: the op's rows of every point of the tiles, and nothing of the spare feature tile
        vals, written = T[n]
        assert written[:8 * rows].all() and not written[8 * rows:].any() and (vals[feats:8 * rows] == 0).all()
    assert T['N'][1][:, :3].all() and not T['N'][1][:, 3:].any()


def test_ld_vec_zero_fills_below_f0_and_writes_only_its_rows():
    T, _ = vm.run_model(vm.ld_vec_case(3, 29, 0.25, 33))
    vals, written = T['ST']
    assert written[:32].all() and not written[32:].any()
    assert (vals[:29] == 0).all() and np.array_equal(vals[29:32, :33], vm.ld_vec_case(3, 29, 0.25, 33)['inputs']['V'][:, :3].T * 0.25)
    T, _ = vm.run_model(vm.ld_vec_case(8, 29, 1.0, 33))
    assert T['ST'][1][:40].all() and not T['ST'][1][40:].any()


def test_every_case_runs_in_both_precisions_and_the_exact_ones_are_exact():
    cases = vm.all_small_cases()
    assert len({c['name'] for c in cases}) == len(cases)
    for c in cases:
        T64, _ = vm.run_model(c)
        T32, _ = vm.run_model(c, prec='f32')                      # (asserts that every accumulator is exact in float32)
        for n in c['outputs']:
            v64, w = T64[n]
            assert w.any() and not np.isnan(v64[w]).any(), (c['name'], n)
            assert np.array_equal(w, T32[n][1])
        if c['name'].startswith(('gemm-', 'ld_t-', 'ld_vec-')):
            for n in c['outputs']:
                assert np.array_equal(T64[n][0][T64[n][1]], T32[n][0][T32[n][1]].astype(np.float64)), (c['name'], n)
    # the integer GEMM cases stay far below 2^24
    big = vm.gemm_case(vm.GEMM_SHAPES[2], 65)
    assert float(np.abs(vm.run_model(big)[0]['S_ACC'][0]).max()) < 2 ** 20


def test_the_model_refuses_what_the_entry_point_must_refuse():
    c = vm.posenc_case(6, 1.0, 33)
    c['tensors']['E'] = ('t', 1)                              # 39 features into one feature tile
    with pytest.raises(vm.Refused):
        vm.run_model(c)
    c = vm.posenc_case(1, 1.0, 33)
    c['tensors']['X'], c['inputs']['X'] = ('vec', 2), c['inputs']['X'][:, :2].copy()
    with pytest.raises(vm.Refused):
        vm.run_model(c)
    c = vm.st_vec_case(2, 0, vm.NONE, 33)
    c['ops'][-1]['f0'] = -2
    with pytest.raises(vm.Refused):
        vm.run_model(c)
    c = vm.extras_case(True, 4, 33)
    c['ops'][-1]['feats'] = 30
    with pytest.raises(vm.Refused):
        vm.run_model(c)


def test_every_case_translates_into_a_program_of_the_shipped_builder():
    """the translator emits Program calls; the descriptor it yields has the op kinds, the wave count and the row budget of the case"""
    from vqnerf_release_amd import tile_program as tp
    kinds = dict(posenc=tp.K_LD_POSENC, posenc_jvp=tp.K_LD_POSENC_JVP, ld_t=tp.K_LD_T, ld_vec=tp.K_LD_VEC, extras=tp.K_LD_EXTRAS,
                 gemm=tp.K_GEMM, st_vec=tp.K_ST_VEC, posenc_vjp=tp.K_POSENC_VJP)
    seen = set()
    for c in [vm.gemm_case(s, 33) for s in vm.GEMM_SHAPES] + [vm.pair_case(vm.EPI_TANGENT, vm.SIGMOID), vm.posenc_case(6, 0.5, 33),
                                                               vm.extras_case(True, 4, 33), vm.ld_vec_case(3, 29, 0.25, 33),
                                                               vm.st_vec_case(4, 30, vm.RELU, 33), vm.persistent_case(65, 8)]:
        b = vm.build_program(c, per_workgroup=c.get('scratch', ()))
        d = b['desc']
        want = [kinds[o['op']] for o in c['ops'] if o['op'] != 'alloc']
        assert d[0] == len(want) and d[2] == c['n_waves'] and 1 <= d[1] <= 160
        assert [int(d[16 + 16 * i]) for i in range(len(want))] == want
        assert int(b['gidx'].max()) < b['flat'].size and [abs(x) for x in b['ld']] == [w for _, w in c['tensors'].values()]
        # the descriptor obeys the contract the entry point now enforces: no GEMM dst of several tiles shares a row with its K segments
        for i in range(len(want)):
            o = d[16 + 16 * i: 32 + 16 * i]
            if o[0] == tp.K_GEMM and o[8] >= 0 and o[1] > 1:
                for r0, n in ((o[2], o[3]), (o[4], o[5])):
                    assert n == 0 or o[8] + 4 * o[1] <= r0 or r0 + n <= o[8], (c['name'], i)
        seen |= set(want)
    assert seen == set(kinds.values())
