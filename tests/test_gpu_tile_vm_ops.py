"""The tile-program interpreter (csrc/tile_vm.hip, vqn_tile_program) op by op against the float64 model of tests/tile_vm_model.py.

Every program is built by the translator of the model from the same case the model runs (tile_program.Program calls, the
packs by build_static_packs), runs once (the launch count is asserted), and writes into NaN-prefilled tensors between NaN guards:
  * written set -- the elements that are no longer NaN are exactly the ones the model says the ops write;
  * exact cases -- integer K inputs, weights and biases: every partial sum is exact in float32, so the output EQUALS the float64
    value (epilogues of ReLU / none: the float32 restatement, which rounds at most once);
  * sigmoid derivative forms -- pure float32 arithmetic of at most 4 roundings: 4 * 2^-24 * the sum of the terms' magnitudes;
  * transcendental cases (softplus / sigmoid forward, softplus derivative forms, sin / cos) -- 8 x the error of the float32
    restatement of the same formula against the float64 model, floor 4 * 2^-24 * max|model|, per feature; every figure recorded
    (profiles/observed_errors_tile_vm_ops.json).
Descriptors the entry point must refuse are handed real allocations large enough for the access a missing check would make."""
import numpy as np
import pytest
import torch

from tests import tile_vm_model as vm
from tests.gpu_util import launches, record_observed
from tests.test_gpu_wgrad_kernels import Guarded
from vqnerf_release_amd import _C

pytestmark = pytest.mark.gpu

F32 = np.float32
VQN_ESHAPE = -2
OWN = '#float32_restatement_own_error'          # key suffix of the figures that are the numpy float32 restatement's, not the kernel's
MARGIN, POISON = 64, 7.0e4                      # floats of a finite poison value before and behind every input tensor


def _upload(x):
    """x on the device between two margins of POISON: an op that reads a few elements outside its operand (a feature offset applied
    without its guard, a point past N) gets a value that shows in the result, not a neighbouring allocation's -> (buffer, pointer)"""
    buf = torch.full((x.size + 2 * MARGIN,), POISON, dtype=torch.float32)
    buf[MARGIN:MARGIN + x.size] = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1)
    buf = buf.cuda()
    return buf, buf.data_ptr() + 4 * MARGIN


class Run:
    """A case on the device: inputs uploaded, every other tensor NaN-filled between guards (per-workgroup ones sized by the grid)."""

    def __init__(self, case, per_workgroup=(), built=None):
        self.case, self.N = case, case['N']
        self.b = built or vm.build_program(case, per_workgroup)
        self.nt = (self.N + 31) // 32
        self.desc = np.ascontiguousarray(self.b['desc'], np.int32)
        self.ld = list(self.b['ld'])
        self.wbuf = torch.from_numpy(self.b['flat'][self.b['gidx']]).cuda()
        self.keep = []                               # device copies of descriptors, alive until the run is dropped
        grid = _C.tile_program_grid(self.desc, self.N)
        self.inputs, self.outputs = {}, {}
        for name, (kind, w) in case['tensors'].items():
            if name in case['inputs']:
                x = case['inputs'][name]
                self.inputs[name] = _upload(x if kind == 'vec' else vm.dense_to_tfmt(x))
            else:
                n_img = grid if name in per_workgroup else self.nt
                self.outputs[name] = Guarded(self.N * w if kind == 'vec' else n_img * w * 1024)

    def pointers(self):
        return [self.inputs[n][1] if n in self.inputs else self.outputs[n].ptr for n in self.case['tensors']]

    def launch(self):
        """through the package's entry; asserts ONE launch of vqn_tile_program and intact guards"""
        self.keep.append(torch.from_numpy(self.desc).cuda())
        with launches() as rec:
            _C.tile_program('case', self.keep[-1], self.desc, self.wbuf, self.pointers(), self.ld, self.N)
        assert rec.counts == {'vqn_tile_program:case': 1}, rec.counts
        for n, g in self.outputs.items():
            assert g.intact(), f'{self.case["name"]}: written outside {n}'
        return self

    def raw(self, desc=None, ld=None):
        """the C entry point itself, unclocked -> (return code, names launched meanwhile)"""
        desc = self.desc if desc is None else np.ascontiguousarray(desc, np.int32)
        ld = np.ascontiguousarray(self.ld if ld is None else ld, np.int32)
        dev = torch.from_numpy(desc).cuda()
        self.keep.append(dev)
        ptrs = self.pointers()
        with launches() as rec:
            rc = _C.lib().vqn_tile_program(dev.data_ptr(), desc.ctypes.data, self.wbuf.data_ptr(), _C._ptrs(ptrs), ld.ctypes.data, len(ptrs), self.N,
                                           torch.cuda.current_stream().cuda_stream)
        return rc, rec.counts

    def got(self, name):
        """an output in the model's dense form (NaN where nothing was written)"""
        kind, w = self.case['tensors'][name]
        g = self.outputs[name]
        if kind == 'vec':
            return g.view(self.N, w).cpu().numpy()
        return vm.tfmt_to_dense(g.view(self.nt, w, 32, 32).cpu().numpy())

    def nothing_written(self):
        return all(bool(torch.isnan(g.full).all()) for g in self.outputs.values())


def _written_sets(run, T64, skip=()):
    """every tensor the program may write: the elements written are the model's, no more and no fewer"""
    got = {}
    for name in run.outputs:
        if name in skip:
            continue
        got[name] = g = run.got(name)
        want = T64[name][1]
        wrong = np.isnan(g) == want
        assert not wrong.any(), f'{run.case["name"]}: {name}: {int(wrong.sum())} elements written / left unlike the model ' \
                                f'(first at {tuple(int(i[0]) for i in np.nonzero(wrong))})'
    return got


def _exact(case, name, got, ref, written):
    """got == ref on the written set, ref exactly representable in float32"""
    r32 = ref[written].astype(F32)
    assert np.array_equal(r32.astype(np.float64), ref[written].astype(np.float64)), f'{case["name"]}: {name}: reference not exact in float32'
    bad = got[written] != r32
    assert not bad.any(), f'{case["name"]}: {name}: {int(bad.sum())} of {bad.size} written elements differ from the exact value'


def _tolerance(test, case, name, got, v64, v32, written, feature_axis):
    """per feature: |got - model| <= max(8 x the float32 restatement's own error, 4 * 2^-24 * max|model|); the worst feature recorded"""
    worst = None
    for f in range(v64.shape[feature_axis]):
        sl = (f, slice(None)) if feature_axis == 0 else (slice(None), f)
        w = written[sl]
        if not w.any():
            continue
        bound, own = vm.own_error_bound(v64[sl][w], v32[sl][w])
        err = float(np.max(np.abs(got[sl][w].astype(np.float64) - v64[sl][w])))
        rec = (err / bound if bound > 0 else (0.0 if err == 0 else np.inf), err, bound, own, f)
        worst = rec if worst is None or rec[0] > worst[0] else worst
    _, err, bound, own, f = worst
    key = f'{case["name"]}/{name}'
    record_observed(test, key + OWN, own, bound)
    record_observed(test, key, err, bound)
    assert err <= bound, f'{key}: feature {f}: error {err:.3e} above {bound:.3e} (float32 restatement: {own:.3e})'


def _model(case):
    return vm.run_model(case)[0], vm.run_model(case, prec='f32')[0]


# --------------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize('N', vm.POINT_COUNTS)
@pytest.mark.parametrize('shape', vm.GEMM_SHAPES, ids=vm.gemm_shape_id)
def test_gemm_of_integers_equals_the_float64_product(shape, N):
    """Single K row, ragged K, two segments with padded outputs, a third round of output tiles, 17 tiles on 8 waves -- each with
    bias + store + dst, store only, accumulate into a preloaded dst, and dst only (the last two read back through an identity GEMM)."""
    case = vm.gemm_case(shape, N)
    T64, _ = vm.run_model(case)
    run = Run(case).launch()
    got = _written_sets(run, T64)
    for name in case['outputs']:
        _exact(case, name, got[name], T64[name][0], T64[name][1])


@pytest.mark.parametrize('pair', vm.PAIRS, ids=vm.pair_id)
def test_every_epilogue_activation_pair(pair):
    """All 16 pairs at (39 + 32 -> 64), N = 33: the nine of the kernel's instantiation table (vm.PAIR_TABLE) and the seven that run
    its generic body; aux1 / aux2 given directly.  Y2 is written by the tangent epilogue alone."""
    epi, a = pair
    case = vm.pair_case(epi, a)
    T64, T32 = _model(case)
    run = Run(case).launch()
    got = _written_sets(run, T64)
    kind = vm.pair_kind(epi, a)
    for name in case['outputs']:
        v64, w = T64[name]
        if kind == 'exact':
            assert np.array_equal(got[name][w], T32[name][0][w]), f'{case["name"]}: {name} differs from the float32 restatement'
        elif kind == 'sigmoid_forms':
            if name == 'Y2':
                mag = np.abs(v64)
            elif name == 'Y' and epi == vm.EPI_BWD2:
                aux2 = case['inputs']['AUX2'].astype(np.float64) * (np.arange(v64.shape[1]) < case['N'])
                mag = np.abs(v64 - aux2) + np.abs(aux2)
            elif name == 'OUT' and epi == vm.EPI_BWD2:
                aux2 = case['inputs']['AUX2'].astype(np.float64)[30:34, :case['N']].T
                mag = np.abs(v64[:, :4] - aux2) + np.abs(aux2)
                mag = np.concatenate([mag, np.zeros((mag.shape[0], 1))], 1)
            else:
                mag = np.abs(v64)
            err = np.abs(got[name][w].astype(np.float64) - v64[w])
            bound = 4 * vm.U * mag[w]
            k = int(np.argmax(err / np.where(bound > 0, bound, np.inf)))          # (padding points: zero against a zero bound)
            record_observed('test_every_epilogue_activation_pair', f'{case["name"]}/{name}', err[k], bound[k])
            assert (err <= bound).all(), f'{case["name"]}: {name}: {err[k]:.3e} above 4 roundings of {mag[w][k]:.3e}'
        else:
            _tolerance('test_every_epilogue_activation_pair', case, name, got[name], v64, T32[name][0], w, 0 if name != 'OUT' else 1)


@pytest.mark.parametrize('waves', (4, 8))
def test_persistent_loop_and_per_workgroup_tensors(waves):
    """The smallest N at which the grid is smaller than the number of tiles: workgroups loop over tiles.  A GEMM stores S, a later
    GEMM of the same program reads it back as aux2; with S per workgroup (negative ld) the results are bit-equal to S per tile."""
    probe = vm.build_program(vm.persistent_case(33, waves))
    full = _C.tile_program_grid(probe['desc'], 2 ** 40)
    N = 32 * full + 1
    assert 0 < _C.tile_program_grid(probe['desc'], N) < (N + 31) // 32 and _C.tile_program_grid(probe['desc'], N - 1) == (N + 30) // 32
    case = vm.persistent_case(N, waves)
    T64, T32 = _model(case)
    per_tile = Run(case).launch()
    got = _written_sets(per_tile, T64)
    for name in ('S', 'Y', 'OUT'):
        assert np.array_equal(got[name][T64[name][1]], T32[name][0][T64[name][1]]), name
    _exact(case, 'S', got['S'], T64['S'][0], T64['S'][1])
    per_wg = Run(case, per_workgroup=('S',)).launch()
    assert per_wg.ld[list(case['tensors']).index('S')] == -2 and per_wg.outputs['S'].used == full * 2 * 1024
    got_wg = _written_sets(per_wg, T64, skip=('S',))
    assert not bool(torch.isnan(per_wg.outputs['S'].view(full, 2, 32, 32)).any())
    for name in ('Y', 'OUT'):
        assert np.array_equal(got_wg[name].view(np.int32), got[name].view(np.int32)), f'{name}: per-workgroup S changes the result'


# --------------------------------------------------------------------------------------------------------------------- non-GEMM ops
@pytest.mark.parametrize('rows,N', vm.LD_T_RUNS)
def test_ld_t_rows(rows, N):
    case = vm.ld_t_case(rows, N)
    T64, _ = vm.run_model(case)
    got = _written_sets(Run(case).launch(), T64)
    _exact(case, 'Y', got['Y'], T64['Y'][0], T64['Y'][1])


@pytest.mark.parametrize('c,f0,scale,N,waves', [r + (4,) for r in vm.LD_VEC_RUNS] + [(8, 29, 1.0, 65, 8)], ids=lambda v: str(v))
def test_ld_vec_zero_fills_below_f0_and_stores_only_its_rows(c, f0, scale, N, waves):
    """source ld = c + 2, store of two feature tiles: rows_for(f0 + c) rows written, [0, f0) and the row padding as zero"""
    case = vm.ld_vec_case(c, f0, scale, N, waves)
    T64, _ = vm.run_model(case)
    got = _written_sets(Run(case).launch(), T64)
    for name in ('ST', 'Y'):
        _exact(case, name, got[name], T64[name][0], T64[name][1])
    assert not T64['ST'][1][8 * vm.rows_for(f0 + c):].any() and (got['ST'][:f0] == 0).all()


@pytest.mark.parametrize('c,f0,a,N', vm.ST_VEC_RUNS, ids=lambda v: str(v))
def test_st_vec_components_offsets_and_activations(c, f0, a, N):
    case = vm.st_vec_case(c, f0, a, N)
    T64, T32 = _model(case)
    got = _written_sets(Run(case).launch(), T64)
    v64, w = T64['OUT']
    if a in (vm.NONE, vm.RELU):
        _exact(case, 'OUT', got['OUT'], v64, w)
    else:
        _tolerance('test_st_vec_components_offsets_and_activations', case, 'OUT', got['OUT'], v64, T32['OUT'][0], w, 1)


@pytest.mark.parametrize('n_freqs,scale,N,waves', [r + (4,) for r in vm.POSENC_RUNS] + [(6, 1.0, 33, 8)])
def test_posenc_its_jvp_and_its_vjp(n_freqs, scale, N, waves):
    """against float64 sin / cos of the float32 argument x * scale; the stores have a spare feature tile that stays untouched"""
    case = vm.posenc_case(n_freqs, scale, N, waves)
    T64, T32 = _model(case)
    got = _written_sets(Run(case).launch(), T64)
    assert np.array_equal(got['E'][:3][T64['E'][1][:3]], T32['E'][0][:3][T64['E'][1][:3]])           # x * scale itself: one rounding
    for name, axis in (('E', 0), ('ED', 0), ('N', 1)):
        _tolerance('test_posenc_its_jvp_and_its_vjp', case, name, got[name], T64[name][0], T32[name][0], T64[name][1], axis)


@pytest.mark.parametrize('normals,nvf,N', vm.EXTRAS_RUNS)
def test_extras_copies_exactly_and_encodes_the_view_direction(normals, nvf, N):
    case = vm.extras_case(normals, nvf, N)
    T64, T32 = _model(case)
    got = _written_sets(Run(case).launch(), T64)
    v64, w = T64['EX']
    ex = case['exact_feats']
    _exact(case, 'EX[copied]', got['EX'][ex], v64[ex], w[ex])
    feats = 3 + (3 + 6 * nvf if nvf else 0) + (3 if normals else 0)
    assert (got['EX'][feats:8 * vm.rows_for(feats)] == 0).all()
    if nvf:
        _tolerance('test_extras_copies_exactly_and_encodes_the_view_direction', case, 'EX', got['EX'], v64, T32['EX'][0], w, 0)


# --------------------------------------------------------------------------------------------------------------------- refusals
def _op_index(case, i):
    """position in the descriptor of the i-th entry of case['ops'] (allocations are no ops of the descriptor)"""
    return sum(1 for o in case['ops'][:i] if o['op'] != 'alloc')


def _find(case, kind, nth=0):
    return [i for i, o in enumerate(case['ops']) if o['op'] == kind][nth]


def _refusal(case, patch):
    """patch(run, desc, ld): make the descriptor / the declared leading dimensions invalid -- the allocations stay as the VALID case
    sized them, and every patch shrinks what is declared, so a missing check shows as a launch and written outputs, never as an
    access outside an allocation"""
    run = Run(case)
    rc, counts = run.raw()
    assert rc == 0 and run.outputs and not run.nothing_written(), 'the unpatched descriptor must run'
    run = Run(case)
    desc, ld = run.desc.copy(), list(run.ld)
    patch(run, desc, ld)
    rc, counts = run.raw(desc, ld)
    torch.cuda.synchronize()
    assert rc == VQN_ESHAPE, f'return code {rc}: {_C.lib().vqn_last_error().decode()}'
    assert counts == {} and run.nothing_written()
    assert b'unsupported shape' in _C.lib().vqn_last_error()


def _declare(name, width):
    def patch(run, desc, ld):
        i = list(run.case['tensors']).index(name)
        assert 0 < width < ld[i]
        ld[i] = width
    return patch


def _point_at(op_kind, p, name, width):
    """operand p of the op reads tensor `name` instead, declared `width` wide (allocated as wide as the case says)"""
    def patch(run, desc, ld):
        o = 16 + 16 * _op_index(run.case, _find(run.case, op_kind))
        desc[o + 1 + p] = list(run.case['tensors']).index(name)
        _declare(name, width)(run, desc, ld)
    return patch


def _set(op_kind, **fields):
    def patch(run, desc, ld):
        o = 16 + 16 * _op_index(run.case, _find(run.case, op_kind))
        for p, v in fields.items():
            desc[o + 1 + int(p[1:])] = v
    return patch


REFUSED = {
    # a TFMT store of fewer feature tiles than the op writes (allocated with the tiles it needs and one to spare)
    'posenc store of 1 tile for 39 features': (lambda: vm.posenc_case(6, 1.0, 33), _declare('E', 1)),
    'posenc_jvp store of 1 tile for 39 features': (lambda: vm.posenc_case(6, 1.0, 33), _declare('ED', 1)),
    'ld_vec store of 1 tile for 37 features': (lambda: vm.ld_vec_case(8, 29, 1.0, 33), _declare('ST', 1)),
    'extras store of 1 tile for 33 features': (lambda: vm.extras_case(True, 4, 33), _declare('EX', 1)),
    # a VEC input of fewer than three components (allocated with 3 to 5)
    'posenc x of ld 2': (lambda: vm.posenc_case(1, 1.0, 33), _point_at('posenc', 0, 'X2', 2)),
    'posenc_jvp x of ld 2': (lambda: vm.posenc_case(1, 1.0, 33), _point_at('posenc_jvp', 0, 'X2', 2)),
    'posenc_jvp v of ld 2': (lambda: vm.posenc_case(1, 1.0, 33), _declare('V', 2)),
    'posenc_vjp x of ld 2': (lambda: vm.posenc_case(1, 1.0, 33), _point_at('posenc_vjp', 1, 'X2', 2)),
    'extras x of ld 2': (lambda: vm.extras_case(True, 4, 33), _declare('X', 2)),
    'extras dirs of ld 2': (lambda: vm.extras_case(True, 4, 33), _declare('D', 2)),
    'extras normals of ld 2': (lambda: vm.extras_case(True, 4, 33), _declare('NR', 2)),
    # VM_LD_EXTRAS: feats tied to 3 + n_view + (3 with normals), n_view_freqs >= 0
    'extras feats 30 for 33': (lambda: vm.extras_case(True, 4, 33), _set('extras', p6=30)),
    'extras n_view_freqs -1': (lambda: vm.extras_case(True, 0, 33), _set('extras', p4=-1)),
}


@pytest.mark.parametrize('which', list(REFUSED))
def test_refused_descriptor(which):
    """VQN_ESHAPE before anything is launched: nothing clocked, every output still NaN"""
    make, patch = REFUSED[which]
    _refusal(make(), patch)


def test_negative_f0_of_st_vec_is_refused():
    """f0 = -3, c = 1: (f0 + c + 7) / 8 is 0 rows, which the row check alone lets through.  Judged by the return code, on a program whose
    source region is not at row 0 (the feature the op would read lies in the rows before it)."""
    case = vm.pair_case(vm.EPI_ACT, vm.NONE)

    def patch(run, desc, ld):
        o = 16 + 16 * _op_index(case, _find(case, 'st_vec'))
        assert desc[o] == 7 and desc[o + 1] >= 4, 'the source region must not be at row 0'
        desc[o + 2], desc[o + 3] = -3, 1
    _refusal(case, patch)


@pytest.mark.parametrize('seg', ('A', 'B'))
def test_gemm_dst_over_its_k_rows_is_refused_with_several_output_tiles(seg):
    """(32 + 39 -> 33): two output tiles, dst moved onto the rows of K segment A / B (inside the row budget: only the race is at stake)"""
    case = vm.gemm_case(vm.GEMM_SHAPES[2], 33)

    def patch(run, desc, ld):
        o = 16 + 16 * _op_index(case, _find(case, 'gemm'))
        assert desc[o] == 6 and desc[o + 1] == 2 and desc[o + 8] >= 0
        r0 = desc[o + 2] if seg == 'A' else desc[o + 4]
        assert r0 + 8 <= desc[1]
        desc[o + 8] = r0
    _refusal(case, patch)


def test_gemm_of_one_output_tile_may_run_in_place():
    """(8 -> 32): with ONE output tile the wave that writes dst has read all of K: dst on the K row itself is accepted and exact"""
    case = vm.gemm_case(vm.GEMM_SHAPES[0], 33)
    T64, _ = vm.run_model(case)
    run = Run(case)
    desc = run.desc.copy()
    o = 16 + 16 * _op_index(case, _find(case, 'gemm'))
    assert desc[o + 1] == 1 and desc[o + 2] + 4 <= desc[1]
    desc[o + 8] = desc[o + 2]
    run.desc = desc
    run.launch()
    _exact(case, 'S_BIAS', run.got('S_BIAS'), T64['S_BIAS'][0], T64['S_BIAS'][1])
