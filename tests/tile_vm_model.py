"""A plain numpy statement of every op of include/vqn_vm_desc.h (the tile-program interpreter, csrc/tile_vm.hip), the cases of
tests/test_gpu_tile_vm_ops.py, and the translator that turns a case into tile_program.Program calls.  Nothing here touches a
GPU; tests/test_tile_vm_model.py checks the model against torch float64 autograd, so that it is a reference of its own and not a
transcription of the kernel.

The model works on an abstract tile image: a region is an array [features, P] (P = the points padded to whole 32-point tiles), a
global tensor is either VEC [N, ld] or TFMT, held densely as [32 * feature tiles, P].  One case (a dict: N, n_waves, tensors, inputs, mats, biases, ops, outputs) drives both
the model (`run_model`) and the translator (`build_program`), so the two cannot drift apart.

run_model(case) -> (tensors, trace): tensors[name] = (values, written) after the whole program, `written` a bool array of the same
shape: the elements some op wrote (padding points of the last tile are written as zero in TFMT and not at all in VEC; everything
else is untouched); trace = per op, {tensor: (the values that op alone wrote, the slice of features / components they occupy)}.
prec='f64' is the reference.  prec='f32' restates the kernel's own formulas (exp2 / log2 / reciprocal forms, one float32 rounding per
operation) in numpy float32: its error against 'f64' is what a float32 evaluation costs, the yardstick of the tolerance cases."""

import numpy as np

NONE, RELU, SOFTPLUS, SIGMOID = 0, 1, 2, 3                      # eng::Act of csrc/mlp_prims.h
EPI_ACT, EPI_MUL_DACT, EPI_TANGENT, EPI_BWD2 = 0, 1, 2, 3       # VmEpi
ACT_NAMES = {NONE: 'none', RELU: 'relu', SOFTPLUS: 'softplus', SIGMOID: 'sigmoid'}
EPI_NAMES = {EPI_ACT: 'act', EPI_MUL_DACT: 'mul_dact', EPI_TANGENT: 'tangent', EPI_BWD2: 'bwd2'}
U = 2.0 ** -24
F32 = np.float32
LOG2E, LN2 = F32(1.4426950408889634), F32(0.6931471805599453)


def rows_for(feats):
    """8-feature rows of an image of `feats` features"""
    return (feats + 7) // 8


# ------------------------------------------------------------------------------------------------------------- activations
def _exp32(x):
    return np.exp2((x * LOG2E).astype(F32)).astype(F32)


def _log32(x):
    return (np.log2(x).astype(F32) * LN2).astype(F32)


def act(a, x, prec='f64'):
    """the activation `a` of x: softplus is nn.Softplus(beta=100, threshold=20)"""
    if a == NONE:
        return x
    if a == RELU:
        return np.maximum(x, 0)
    with np.errstate(over='ignore', invalid='ignore'):
        if prec == 'f32':
            x = x.astype(F32)
            if a == SOFTPLUS:
                t = (F32(100) * x).astype(F32)
                return np.where(t > F32(20), x, F32(0.01) * _log32(F32(1) + _exp32(t))).astype(F32)
            return (F32(1) / (F32(1) + _exp32(-x))).astype(F32)
        if a == SOFTPLUS:
            t = 100.0 * x
            return np.where(t > 20.0, x, np.log1p(np.exp(np.minimum(t, 20.0))) / 100.0)
        return 1.0 / (1.0 + np.exp(-x))


def dact(a, o, prec='f64'):
    """act'(pre-activation), expressed through the activation's OUTPUT o"""
    if a == RELU:
        return (o > 0).astype(o.dtype)
    if a == SIGMOID:
        return o * (1 - o)
    if a == SOFTPLUS:
        return F32(1) - _exp32(F32(-100) * o) if prec == 'f32' else -np.expm1(-100.0 * o)
    return np.ones_like(o)


def d2ratio(a, o, prec='f64'):
    """act'' / act' through the output"""
    if a == SIGMOID:
        return 1 - 2 * o
    if a == SOFTPLUS:
        return F32(100) * _exp32(F32(-100) * o) if prec == 'f32' else 100.0 * np.exp(-100.0 * o)
    return np.zeros_like(o)


def epilogue(epi, a, acc, aux1=None, aux2=None, prec='f64'):
    """-> (y, y2 | None) of one GEMM epilogue on the accumulator values acc"""
    if epi == EPI_ACT:
        return act(a, acc, prec), None
    d1 = dact(a, aux1, prec)
    if epi == EPI_MUL_DACT:
        return acc * d1, None
    if epi == EPI_TANGENT:
        return acc * d1, aux2 * acc * d2ratio(a, aux1, prec)
    return acc * d1 + aux2, None


# ------------------------------------------------------------------------------------------------------------- posenc
def posenc(xs, n_freqs, prec='f64'):
    """xs [3, P] float32 (the argument the kernel forms: x * scale, rounded once) -> (features [3 + 6 n, P], Jacobian entries
    d feature / d xs_c [3 + 6 n, P], c per feature): [x, sin(2^k x), cos(2^k x)]_k.  2^k x is exact in float32."""
    dt = F32 if prec == 'f32' else np.float64
    feats, jac, comp = [xs[c].astype(dt) for c in range(3)], [np.ones(xs.shape[1], dt)] * 3, [0, 1, 2]
    for k in range(n_freqs):
        fr = F32(2 ** k)
        arg = (xs * fr).astype(F32).astype(dt)
        s, c = np.sin(arg).astype(dt), np.cos(arg).astype(dt)
        feats += [s[i] for i in range(3)] + [c[i] for i in range(3)]
        jac += [dt(fr) * c[i] for i in range(3)] + [-dt(fr) * s[i] for i in range(3)]
        comp += [0, 1, 2, 0, 1, 2]
    return np.stack(feats), np.stack(jac), comp


# ------------------------------------------------------------------------------------------------------------- the model
class Refused(Exception):
    """the descriptor of this case is one vqn_tile_program must refuse"""


def run_model(case, prec='f64'):
    dt = F32 if prec == 'f32' else np.float64
    N = case['N']
    P = 32 * ((N + 31) // 32)
    pidx, valid = np.minimum(np.arange(P), N - 1), np.arange(P) < N
    T = {}
    for name, (kind, w) in case['tensors'].items():
        shape = (N, w) if kind == 'vec' else (32 * w, P)
        if name in case['inputs']:
            x = np.asarray(case['inputs'][name])
            assert x.dtype == F32 and x.shape == shape, (name, x.shape, shape)
            T[name] = [x.astype(dt), None]
        else:
            T[name] = [np.full(shape, np.nan, dt), np.zeros(shape, bool)]
    regions, feats_of, trace = {}, {}, []

    def vec(name, width):
        kind, ld = case['tensors'][name]
        if kind != 'vec' or ld < width:
            raise Refused(f'{name}: not a VEC tensor of at least {width} components')
        return T[name][0]

    def store_t(wr, name, vals):
        """TFMT store of the features [0, len(vals)): padding points as zero"""
        if name is None:
            return
        v, m = T[name]
        if case['tensors'][name][0] == 'vec' or vals.shape[0] > v.shape[0]:
            raise Refused(f'{name}: fewer feature tiles than the op writes')
        v[:vals.shape[0]] = np.where(valid, vals, 0)
        m[:vals.shape[0]] = True
        wr[name] = (np.where(valid, vals, 0).astype(dt), slice(0, vals.shape[0]))

    def region_write(name, vals):
        if vals.shape[0] > regions[name].shape[0]:
            raise Refused(f'region {name}: {vals.shape[0]} features written into {regions[name].shape[0]}')
        regions[name][:vals.shape[0]] = vals

    for op in case['ops']:
        k, wr = op['op'], {}
        if k == 'alloc':
            rows = 4 * op['tiles'] if op.get('tiles') else rows_for(op['feats'])
            regions[op['name']], feats_of[op['name']] = np.full((8 * rows, P), np.nan, dt), op['feats']
        elif k in ('posenc', 'posenc_jvp'):
            if op['n_freqs'] < 0:
                raise Refused('n_freqs < 0')
            xs = (vec(op['x'], 3)[pidx, :3].T.astype(F32) * F32(op['scale'])).astype(F32)
            f, jac, comp = posenc(xs, op['n_freqs'], prec)
            if k == 'posenc_jvp':
                v = vec(op['v'], 3)[pidx, :3].T.astype(dt)
                f = (jac * v[comp]).astype(dt)
            vals = np.zeros((8 * rows_for(f.shape[0]), P), dt)
            vals[:f.shape[0]] = f
            region_write(op['dst'], vals)
            store_t(wr, op.get('store'), vals)
        elif k == 'ld_t':
            kind, w = case['tensors'][op['t']]
            if kind != 't' or 4 * w < op['rows']:
                raise Refused('VM_LD_T: more rows than the tensor has')
            region_write(op['dst'], T[op['t']][0][:8 * op['rows']].astype(dt))
        elif k == 'ld_vec':
            c, f0 = op['c'], op['f0']
            if not (1 <= c <= 8 and f0 >= 0):
                raise Refused('VM_LD_VEC: 1 <= c <= 8, f0 >= 0')
            vals = np.zeros((8 * rows_for(f0 + c), P), dt)                       # features [0, f0) and the row padding: zero
            vals[f0:f0 + c] = (vec(op['t'], c)[pidx, :c].T.astype(dt) * dt(op['scale'])).astype(dt)
            region_write(op['dst'], vals)
            store_t(wr, op.get('store'), vals)
        elif k == 'extras':
            nvf, nrm = op['n_view_freqs'], op.get('normals')
            if nvf < 0:
                raise Refused('n_view_freqs < 0')
            parts = [vec(op['x'], 3)[pidx, :3].T.astype(dt)]
            if nvf > 0:
                parts.append(posenc(vec(op['dirs'], 3)[pidx, :3].T.astype(F32), nvf, prec)[0])
            else:
                vec(op['dirs'], 3)
            if nrm is not None:
                parts.append(vec(nrm, 3)[pidx, :3].T.astype(dt))
            f = np.concatenate(parts)
            if op.get('feats', f.shape[0]) != f.shape[0]:
                raise Refused('VM_LD_EXTRAS: feats != 3 + n_view + (3 with normals)')
            vals = np.zeros((8 * rows_for(f.shape[0]), P), dt)
            vals[:f.shape[0]] = f
            region_write(op['dst'], vals)
            store_t(wr, op.get('store'), vals)
        elif k == 'gemm':
            M = np.asarray(case['mats'][op['key']], np.float64)
            out = op['out_feats']
            assert M.shape[0] == out
            OF = 32 * ((out + 31) // 32)
            dst = op.get('dst', op.get('out'))
            if dst is not None and dst not in regions:
                regions[dst], feats_of[dst] = np.full((OF, P), np.nan, dt), out
            acc = np.zeros((OF, P))
            if op.get('accumulate'):
                acc = regions[dst][:OF].astype(np.float64)
            elif op.get('bias') is not None:
                acc[:out] = np.asarray(case['biases'][op['bias']], np.float64)[:, None]
            with np.errstate(invalid='ignore'):
                for rname, n_valid, base in op['segs']:
                    R = regions[rname][:8 * rows_for(feats_of[rname])].astype(np.float64)
                    Mp = np.zeros((OF, R.shape[0]))
                    Mp[:out, :n_valid] = M[:, base:base + n_valid]
                    acc = acc + Mp @ R                                           # (zero weights times the padding features: NaN stays NaN)
            if prec == 'f32':
                a32 = acc.astype(F32)
                assert np.array_equal(a32.astype(np.float64), acc, equal_nan=True), 'accumulator values are not exact in float32'
                acc = a32
            a1 = T[op['aux1']][0][:OF].astype(dt) if op.get('aux1') else None
            a2 = T[op['aux2']][0][:OF].astype(dt) if op.get('aux2') else None
            if (op['epi'] != EPI_ACT and a1 is None) or (op['epi'] in (EPI_TANGENT, EPI_BWD2) and a2 is None):
                raise Refused('epilogue operand missing')
            y, y2 = epilogue(op['epi'], op['act'], acc.astype(dt), a1, a2, prec)
            y = y.astype(dt)
            store_t(wr, op.get('store'), y)
            if y2 is not None:
                store_t(wr, op.get('store2'), y2.astype(dt))
            if dst is not None:
                region_write(dst, y)
        elif k == 'st_vec':
            c, f0 = op['c'], op['f0']
            if not (1 <= c <= 4 and f0 >= 0):
                raise Refused('VM_ST_VEC: 1 <= c <= 4, f0 >= 0')
            o, m = T[op['t']]
            vec(op['t'], c)
            o[:, :c] = (act(op['act'], regions[op['src']][f0:f0 + c, :N].T, prec).astype(dt) * dt(op['scale'])).astype(dt)
            m[:, :c] = True
            wr[op['t']] = (o[:, :c].copy(), slice(0, c))
        elif k == 'posenc_vjp':
            xs = (vec(op['x'], 3)[pidx, :3].T.astype(F32) * F32(op['scale'])).astype(F32)
            _, jac, comp = posenc(xs, op['n_freqs'], prec)
            G = regions[op['src']][:jac.shape[0]].astype(dt)
            g = G[:3].copy()
            for f in range(3, jac.shape[0]):                                      # the kernel's order: k ascending, sin before cos
                g[comp[f]] = (g[comp[f]] + (G[f] * jac[f]).astype(dt)).astype(dt)
            o, m = T[op['out']]
            vec(op['out'], 3)
            o[:, :3], m[:, :3] = g[:, :N].T, True
            wr[op['out']] = (o[:, :3].copy(), slice(0, 3))
        else:
            raise KeyError(k)
        trace.append((op, wr))
    return {n: tuple(v) for n, v in T.items()}, trace


# ------------------------------------------------------------------------------------------------------------- layouts
def dense_to_tfmt(d):
    """[32 w, P] -> the tile format [P / 32, w, 32 features, 32 points]"""
    w, nt = d.shape[0] // 32, d.shape[1] // 32
    return np.ascontiguousarray(d.reshape(w, 32, nt, 32).transpose(2, 0, 1, 3))


def tfmt_to_dense(t):
    nt, w = t.shape[:2]
    return np.ascontiguousarray(t.transpose(1, 2, 0, 3).reshape(32 * w, 32 * nt))


# ------------------------------------------------------------------------------------------------------------- translator
def _name(key):
    return key if isinstance(key, str) else '_'.join(str(k) for k in key)


def build_program(case, per_workgroup=()):
    """case -> dict(prog, desc [int32], gidx, flat [float32: the weight buffer is flat[gidx]], names, ld): the Program calls the
    shipped engines make (alloc, gemm, op, finalize, materialize, build_static_packs with a FlatLayout).  per_workgroup: tensors
    handed over with a negative ld."""
    from vqnerf_release_amd import tile_program as tp
    from vqnerf_release_amd.geo.packing import FlatLayout
    names = list(case['tensors'])
    Pg = tp.Program(names)
    reg = {}
    live = lambda op: [reg[n] for n in op.get('live', ())]
    for op in case['ops']:
        k = op['op']
        if k == 'alloc':
            reg[op['name']] = Pg.alloc(op['feats'], live(op), tiles=op.get('tiles'))
        elif k == 'posenc':
            Pg.op(tp.K_LD_POSENC, Pg.t(op['x']), Pg.row(reg[op['dst']]), op['n_freqs'], 3 + 6 * op['n_freqs'], Pg.t(op.get('store')),
                  tp._f2i(op['scale']))
        elif k == 'posenc_jvp':
            Pg.op(tp.K_LD_POSENC_JVP, Pg.t(op['x']), Pg.t(op['v']), Pg.row(reg[op['dst']]), op['n_freqs'], 3 + 6 * op['n_freqs'],
                  Pg.t(op.get('store')), tp._f2i(op['scale']))
        elif k == 'ld_t':
            Pg.op(tp.K_LD_T, Pg.t(op['t']), Pg.row(reg[op['dst']]), op['rows'])
        elif k == 'ld_vec':
            Pg.op(tp.K_LD_VEC, Pg.t(op['t']), Pg.row(reg[op['dst']]), op['c'], tp._f2i(op['scale']), Pg.t(op.get('store')), op['f0'])
        elif k == 'extras':
            nvf = op['n_view_freqs']
            feats = op.get('feats', 3 + (3 + 6 * nvf if nvf > 0 else 0) + (3 if op.get('normals') else 0))
            Pg.op(tp.K_LD_EXTRAS, Pg.t(op['x']), Pg.t(op['dirs']), Pg.t(op.get('normals')), Pg.row(reg[op['dst']]), nvf,
                  Pg.t(op.get('store')), feats)
        elif k == 'gemm':
            M = case['mats'][op['key']]
            segs = [reg[s[0]] for s in op['segs']]
            dst = Pg.gemm(('M', op['key']), M.shape, segs, [(s[1], s[2]) for s in op['segs']], op['out_feats'], live(op), epi=op['epi'],
                          act=op['act'], bias_key=('b', op['bias']) if op.get('bias') is not None else None, aux1=op.get('aux1'),
                          aux2=op.get('aux2'), store=op.get('store'), store2=op.get('store2'),
                          dst=reg[op['dst']] if op.get('dst') else None, accumulate=bool(op.get('accumulate')),
                          want_dst=bool(op.get('out') or op.get('dst')))
            if op.get('out'):
                reg[op['out']] = dst
        elif k == 'st_vec':
            Pg.op(tp.K_ST_VEC, Pg.row(reg[op['src']]), op['f0'], op['c'], Pg.t(op['t']), op['act'], tp._f2i(op['scale']))
        elif k == 'posenc_vjp':
            Pg.op(tp.K_POSENC_VJP, Pg.row(reg[op['src']]), Pg.t(op['x']), Pg.t(op['out']), op['n_freqs'], tp._f2i(op['scale']))
        else:
            raise KeyError(k)
    Pg.finalize(n_waves=case['n_waves']).materialize()
    src = [('M_' + _name(k), np.asarray(m, F32)) for k, m in case['mats'].items()] + \
          [('b_' + _name(k), np.asarray(b, F32)) for k, b in case['biases'].items()]
    if not src:
        src = [('none', np.zeros(4, F32))]
    L = FlatLayout([(n, a.shape) for n, a in src])
    if Pg.gathers:
        gidx, descs = tp.build_static_packs({'p': Pg}, L, lambda key: L[('M_' if key[0] == 'M' else 'b_') + _name(key[1])])
        desc = descs['p']
    else:                                       # a program without a GEMM has no pack to build: the descriptor as build_static_packs lays it out
        gidx, desc = np.full(4, L.zero, np.int64), np.zeros(tp.DESC_INTS, np.int32)
        desc[0:4] = [len(Pg.ops), Pg.total_rows, Pg.n_waves, len(Pg.tn)]
        for i, o in enumerate(Pg.ops):
            desc[16 + 16 * i: 32 + 16 * i] = o
    flat = np.concatenate([a.reshape(-1) for _, a in src] + [np.zeros(1, F32)])
    ld = [(-w if n in per_workgroup else w) for n, (_, w) in case['tensors'].items()]
    return dict(prog=Pg, desc=desc, gidx=gidx, flat=flat, names=names, ld=ld, regions=reg)


# ------------------------------------------------------------------------------------------------------------- the cases
POINT_COUNTS = (1, 31, 32, 33, 65)


def _ints(rng, shape, m):
    return rng.integers(-m, m + 1, shape).astype(F32)


def _P(N):
    return 32 * ((N + 31) // 32)


def _seed(*parts):
    """a seed that depends on the case only (not on the process: no hash())"""
    return sum((i + 1) * 7919 * sum(map(ord, str(p))) for i, p in enumerate(parts)) % (2 ** 31)


# (segment A features, segment B features | None, outputs, waves)
GEMM_SHAPES = [(8, None, 32, 4), (39, None, 64, 4), (32, 39, 33, 4), (64, None, 257, 4), (24, 8, 544, 8)]


def gemm_shape_id(s):
    return '%d+%s-%d-w%d' % (s[0], s[1] if s[1] else 0, s[2], s[3])


def gemm_case(shape, N):
    """One program per shape: every way a GEMM op starts (bias, zero, accumulate into a preloaded dst) and ends (store, dst, both).
    Integer inputs, weights and biases: every partial sum is an integer float32 holds exactly, whatever the summation order.
      S_BIAS  <- bias, store and dst          S_ONLY <- no bias, store only (dst = -1)
      S_ACC   <- accumulate into dst preloaded from D0, no store; read back through an identity GEMM
      S_DST   <- bias, dst only; read back through an identity GEMM"""
    fa, fb, out, waves = shape
    rng = np.random.default_rng(_seed('gemm', shape, N))
    P, tiles = _P(N), (out + 31) // 32
    kin = fa + (fb or 0)
    tensors = {'A': ('t', (fa + 31) // 32), 'D0': ('t', tiles)}
    inputs = {'A': _ints(rng, (32 * tensors['A'][1], P), 3), 'D0': _ints(rng, (32 * tiles, P), 3)}
    ops = [dict(op='alloc', name='a', feats=fa), dict(op='ld_t', t='A', dst='a', rows=rows_for(fa))]
    segs, keep = [('a', fa, 0)], ['a']
    if fb:
        tensors['B'] = ('t', (fb + 31) // 32)
        inputs['B'] = _ints(rng, (32 * tensors['B'][1], P), 3)
        ops += [dict(op='alloc', name='b', feats=fb, live=['a']), dict(op='ld_t', t='B', dst='b', rows=rows_for(fb))]
        segs.append(('b', fb, fa))
        keep.append('b')
    for n in ('S_BIAS', 'S_ONLY', 'S_ACC', 'S_DST'):
        tensors[n] = ('t', tiles)
    mats = {'W': _ints(rng, (out, kin), 2), 'I': np.eye(out, dtype=F32)}
    biases = {'W': _ints(rng, (out,), 5)}
    g = dict(op='gemm', key='W', segs=segs, out_feats=out, epi=EPI_ACT, act=NONE, live=keep)
    ident = lambda src, st: dict(op='gemm', key='I', segs=[(src, out, 0)], out_feats=out, epi=EPI_ACT, act=NONE, live=keep + [src], store=st)
    ops += [dict(g, bias='W', store='S_BIAS', out='y1'),
            dict(g, store='S_ONLY'),
            dict(op='alloc', name='acc', feats=out, tiles=tiles, live=keep), dict(op='ld_t', t='D0', dst='acc', rows=4 * tiles),
            dict(g, dst='acc', accumulate=True, live=keep + ['acc']), ident('acc', 'S_ACC'),
            dict(g, bias='W', out='y4'), ident('y4', 'S_DST')]
    return dict(name='gemm-%s-N%d' % (gemm_shape_id(shape), N), N=N, n_waves=waves, tensors=tensors, inputs=inputs, mats=mats, biases=biases,
                ops=ops, outputs=['S_BIAS', 'S_ONLY', 'S_ACC', 'S_DST'])


PAIRS = [(e, a) for e in (EPI_ACT, EPI_MUL_DACT, EPI_TANGENT, EPI_BWD2) for a in (NONE, RELU, SOFTPLUS, SIGMOID)]
PAIR_TABLE = {(EPI_ACT, NONE), (EPI_ACT, RELU), (EPI_ACT, SOFTPLUS), (EPI_ACT, SIGMOID), (EPI_MUL_DACT, RELU), (EPI_MUL_DACT, SOFTPLUS),
              (EPI_MUL_DACT, SIGMOID), (EPI_TANGENT, SOFTPLUS), (EPI_BWD2, SOFTPLUS)}          # VM_PAIR of csrc/tile_vm.hip


def pair_id(p):
    return EPI_NAMES[p[0]] + '-' + ACT_NAMES[p[1]]


def pair_kind(epi, a):
    """'exact' (ReLU / none: no or one rounding), 'sigmoid_forms' (pure float32 arithmetic: at most 4 roundings) or 'transcendental'"""
    if a in (NONE, RELU):
        return 'exact'
    return 'sigmoid_forms' if (a == SIGMOID and epi != EPI_ACT) else 'transcendental'


def aux1_for(a, rng, shape):
    """activation outputs, inside the activation's range"""
    if a == RELU:
        return np.where(rng.random(shape) < 0.4, 0.0, rng.random(shape) * 2 + 0.01).astype(F32)
    if a == SIGMOID:
        return rng.uniform(0.02, 0.98, shape).astype(F32)
    if a == SOFTPLUS:                                   # softplus of pre-activations on both sides of zero and past the threshold
        z = rng.uniform(-0.08, 0.08, shape)
        z[rng.random(shape) < 0.1] = 0.25
        return act(SOFTPLUS, z).astype(F32)
    return rng.standard_normal(shape).astype(F32)


def pair_case(epi, a, N=33):
    """(39 + 32 -> 64): one GEMM per (epilogue, activation) pair, store (+ store2 of the tangent epilogue) and dst, the dst read
    back through VM_ST_VEC.  Weights are integers times a power of two, so the accumulator is exact; the power puts the
    pre-activations where the activation bends (softplus: 100 a across [-20, 20] and past the threshold)."""
    rng = np.random.default_rng(_seed('pair', epi, a, N))
    P = _P(N)
    wscale = {NONE: 1.0, RELU: 1.0, SIGMOID: 2.0 ** -3, SOFTPLUS: 2.0 ** -7 if epi == EPI_ACT else 2.0 ** -3}[a]
    tensors = {'A': ('t', 2), 'B': ('t', 1), 'AUX1': ('t', 2), 'AUX2': ('t', 2), 'Y': ('t', 2), 'Y2': ('t', 2), 'OUT': ('vec', 5)}
    inputs = {'A': _ints(rng, (64, P), 3), 'B': _ints(rng, (32, P), 3), 'AUX1': aux1_for(a, rng, (64, P)),
              'AUX2': rng.standard_normal((64, P)).astype(F32)}
    mats = {'W': (_ints(rng, (64, 71), 2) * F32(wscale)).astype(F32)}
    biases = {'W': (_ints(rng, (64,), 3) * F32(wscale)).astype(F32)}
    ops = [dict(op='alloc', name='a', feats=39), dict(op='ld_t', t='A', dst='a', rows=5),
           dict(op='alloc', name='b', feats=32, live=['a']), dict(op='ld_t', t='B', dst='b', rows=4),
           dict(op='gemm', key='W', segs=[('a', 39, 0), ('b', 32, 39)], out_feats=64, epi=epi, act=a, bias='W', live=['a', 'b'],
                aux1='AUX1' if epi != EPI_ACT else None, aux2='AUX2' if epi in (EPI_TANGENT, EPI_BWD2) else None, store='Y',
                store2='Y2' if epi == EPI_TANGENT else None, out='y'),
           dict(op='st_vec', src='y', f0=30, c=4, t='OUT', act=NONE, scale=1.0)]
    outs = ['Y', 'OUT'] + (['Y2'] if epi == EPI_TANGENT else [])
    return dict(name='pair-' + pair_id((epi, a)), N=N, n_waves=4, tensors=tensors, inputs=inputs, mats=mats, biases=biases, ops=ops, outputs=outs)


def persistent_case(N, waves, per_tile_only=False):
    """A GEMM stores S, a later GEMM of the same program reads it back as aux2 (per-workgroup or per-tile: the same results); run
    at the smallest N for which the grid is smaller than the number of tiles, so that workgroups loop over tiles."""
    rng = np.random.default_rng(_seed('persistent', waves))
    P = _P(N)
    tensors = {'A': ('t', 1), 'AUX1': ('t', 2), 'S': ('t', 2), 'Y': ('t', 2), 'OUT': ('vec', 2)}
    inputs = {'A': _ints(rng, (32, P), 3), 'AUX1': aux1_for(RELU, rng, (64, P))}
    mats = {'W1': _ints(rng, (33, 24), 2), 'W2': _ints(rng, (40, 33), 2)}
    biases = {'W1': _ints(rng, (33,), 3)}
    ops = [dict(op='alloc', name='a', feats=24), dict(op='ld_t', t='A', dst='a', rows=3),
           dict(op='gemm', key='W1', segs=[('a', 24, 0)], out_feats=33, epi=EPI_ACT, act=NONE, bias='W1', live=['a'], store='S', out='h'),
           dict(op='gemm', key='W2', segs=[('h', 33, 0)], out_feats=40, epi=EPI_BWD2, act=RELU, aux1='AUX1', aux2='S', live=['h'], store='Y',
                out='y'),
           dict(op='st_vec', src='y', f0=38, c=2, t='OUT', act=NONE, scale=1.0)]
    return dict(name='persistent-w%d-N%d' % (waves, N), N=N, n_waves=waves, tensors=tensors, inputs=inputs, mats=mats, biases=biases, ops=ops,
                outputs=['Y', 'OUT'], scratch=['S'])


LD_T_ROWS = (1, 4, 5, 8)


def ld_t_case(rows, N):
    """VM_LD_T of `rows` rows, then an identity GEMM with a store: exact"""
    rng = np.random.default_rng(_seed('ld_t', rows, N))
    feats = 8 * rows
    tensors = {'A': ('t', 3), 'Y': ('t', (feats + 31) // 32)}
    inputs = {'A': _ints(rng, (96, _P(N)), 3)}
    ops = [dict(op='alloc', name='a', feats=feats), dict(op='ld_t', t='A', dst='a', rows=rows),
           dict(op='gemm', key='I', segs=[('a', feats, 0)], out_feats=feats, epi=EPI_ACT, act=NONE, live=['a'], store='Y')]
    return dict(name='ld_t-r%d-N%d' % (rows, N), N=N, n_waves=4, tensors=tensors, inputs=inputs, mats={'I': np.eye(feats, dtype=F32)}, biases={},
                ops=ops, outputs=['Y'])


LD_VEC_CASES = [(c, f0, s) for c in (1, 3, 8) for f0 in (0, 5, 29) for s in (1.0, 0.25)]


def ld_vec_case(c, f0, scale, N, waves=4):
    """VM_LD_VEC from a source with ld > c and a TFMT store of two feature tiles: the op writes rows_for(f0 + c) rows of the store
    ([0, f0) and the row padding as zero) and nothing else; the LDS image is read back through an identity GEMM."""
    rng = np.random.default_rng(_seed('ld_vec', c, f0, scale, N))
    feats = f0 + c
    tensors = {'V': ('vec', c + 2), 'ST': ('t', 2), 'Y': ('t', 2)}
    inputs = {'V': _ints(rng, (N, c + 2), 100)}
    ops = [dict(op='alloc', name='a', feats=feats), dict(op='ld_vec', t='V', dst='a', c=c, scale=scale, store='ST', f0=f0),
           dict(op='gemm', key='I', segs=[('a', feats, 0)], out_feats=feats, epi=EPI_ACT, act=NONE, live=['a'], store='Y')]
    return dict(name='ld_vec-c%d-f%d-s%g-N%d-w%d' % (c, f0, scale, N, waves), N=N, n_waves=waves, tensors=tensors, inputs=inputs,
                mats={'I': np.eye(feats, dtype=F32)}, biases={}, ops=ops, outputs=['ST', 'Y'])


ST_VEC_CASES = [(c, f0, a) for c in (1, 2, 4) for f0 in (0, 30, 36) for a in (NONE, RELU, SOFTPLUS, SIGMOID)]


def st_vec_case(c, f0, a, N):
    """VM_ST_VEC of c features at f0 (30 + 4 crosses a 32-feature tile) with every activation, scale 0.5, destination ld = c + 3"""
    rng = np.random.default_rng(_seed('st_vec', c, f0, a, N))
    src = (rng.standard_normal((64, _P(N))) * (0.1 if a == SOFTPLUS else 2.0)).astype(F32)
    tensors = {'A': ('t', 2), 'OUT': ('vec', c + 3)}
    ops = [dict(op='alloc', name='a', feats=40), dict(op='ld_t', t='A', dst='a', rows=5),
           dict(op='st_vec', src='a', f0=f0, c=c, t='OUT', act=a, scale=0.5)]
    return dict(name='st_vec-c%d-f%d-%s-N%d' % (c, f0, ACT_NAMES[a], N), N=N, n_waves=4, tensors=tensors, inputs={'A': src}, mats={}, biases={},
                ops=ops, outputs=['OUT'])


POSENC_CASES = [(n, s) for n in (0, 1, 6, 10) for s in (1.0, 0.5)]


def posenc_case(n_freqs, scale, N, waves=4):
    """VM_LD_POSENC and VM_LD_POSENC_JVP with a store of one feature tile more than they write, and VM_POSENC_VJP of an adjoint
    loaded by VM_LD_T; x has ld 4."""
    rng = np.random.default_rng(_seed('posenc', n_freqs, scale, N))
    feats = 3 + 6 * n_freqs
    ft = (feats + 31) // 32
    tensors = {'X': ('vec', 4), 'V': ('vec', 5), 'G': ('t', ft), 'E': ('t', ft + 1), 'ED': ('t', ft + 1), 'N': ('vec', 4), 'X2': ('vec', 4)}
    inputs = {'X': rng.uniform(-1, 1, (N, 4)).astype(F32), 'V': rng.standard_normal((N, 5)).astype(F32),
              'G': rng.standard_normal((32 * ft, _P(N))).astype(F32)}
    inputs['X2'] = inputs['X'].copy()                   # (no op reads it: the refusal tests point one op at a time at it)
    ops = [dict(op='alloc', name='e', feats=feats), dict(op='posenc', x='X', dst='e', n_freqs=n_freqs, store='E', scale=scale),
           dict(op='alloc', name='ed', feats=feats), dict(op='posenc_jvp', x='X', v='V', dst='ed', n_freqs=n_freqs, store='ED', scale=scale),
           dict(op='alloc', name='g', feats=feats), dict(op='ld_t', t='G', dst='g', rows=rows_for(feats)),
           dict(op='posenc_vjp', src='g', x='X', out='N', n_freqs=n_freqs, scale=scale)]
    return dict(name='posenc-n%d-s%g-N%d-w%d' % (n_freqs, scale, N, waves), N=N, n_waves=waves, tensors=tensors, inputs=inputs, mats={}, biases={}, ops=ops,
                outputs=['E', 'ED', 'N'])


EXTRAS_CASES = [(nrm, nvf) for nrm in (True, False) for nvf in (0, 4)]


def extras_case(normals, nvf, N):
    rng = np.random.default_rng(_seed('extras', normals, nvf, N))
    feats = 3 + (3 + 6 * nvf if nvf else 0) + (3 if normals else 0)
    tensors = {'X': ('vec', 3), 'D': ('vec', 4), 'NR': ('vec', 5), 'EX': ('t', 2)}
    inputs = {'X': rng.standard_normal((N, 3)).astype(F32), 'D': rng.uniform(-1, 1, (N, 4)).astype(F32),
              'NR': rng.standard_normal((N, 5)).astype(F32)}
    ops = [dict(op='alloc', name='e', feats=feats),
           dict(op='extras', x='X', dirs='D', normals='NR' if normals else None, dst='e', n_view_freqs=nvf, store='EX')]
    return dict(name='extras-%s-v%d-N%d' % ('nrm' if normals else 'nonrm', nvf, N), N=N, n_waves=4, tensors=tensors, inputs=inputs, mats={},
                biases={}, ops=ops, outputs=['EX'], exact_feats=[f for f in range(feats) if f < (6 if nvf else 3) or (normals and f >= feats - 3)])


def with_counts(params):
    """the point counts dealt round-robin over a list of parameter tuples: every count meets every op without crossing the lists"""
    return [tuple(p) + (POINT_COUNTS[i % len(POINT_COUNTS)],) for i, p in enumerate(params)]


LD_T_RUNS = with_counts([(r,) for r in LD_T_ROWS] * 2)
LD_VEC_RUNS = with_counts(LD_VEC_CASES)
ST_VEC_RUNS = with_counts(ST_VEC_CASES)
POSENC_RUNS = with_counts(POSENC_CASES)
EXTRAS_RUNS = with_counts(EXTRAS_CASES)


def all_small_cases():
    """every case of the GPU test below the persistent-loop sizes (the CPU test runs the model over all of them)"""
    out = [gemm_case(s, N) for s in GEMM_SHAPES for N in POINT_COUNTS]
    out += [pair_case(e, a) for e, a in PAIRS]
    out += [ld_t_case(*r) for r in LD_T_RUNS]
    out += [ld_vec_case(*r) for r in LD_VEC_RUNS]
    out += [st_vec_case(*r) for r in ST_VEC_RUNS]
    out += [posenc_case(*r) for r in POSENC_RUNS]
    out += [extras_case(*r) for r in EXTRAS_RUNS]
    out += [posenc_case(6, 1.0, 33, waves=8), ld_vec_case(8, 29, 1.0, 65, waves=8)]
    return out


# ------------------------------------------------------------------------------------------------------------- bounds
def own_error_bound(v64, v32, factor=8.0):
    """Bound of a tolerance case: `factor` x the float32 restatement's own maximum error against the float64 model, with a floor of
    4 * 2^-24 * max|model| (the hardware exp2 / log / reciprocal are not correctly rounded, and the t * log2(e) pre-multiply adds
    |t| 2^-24 in the exponent).  -> (bound, restatement error)"""
    own = float(np.max(np.abs(v32.astype(np.float64) - v64))) if v64.size else 0.0
    scale = float(np.max(np.abs(v64))) if v64.size else 0.0
    return max(factor * own, 4 * U * scale), own
