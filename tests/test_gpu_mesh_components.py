"""GPU: connected components and compaction of a device mesh -- csrc/mesh_components.hip through geo/mesh.py components and
filter_components.

The oracle is tests/mesh_cc_model.py, a plain union-find canonicalised like the kernel (label = smallest vertex index of the
component), so every comparison of labels is exact equality; the filtered meshes are compared with its host statement of the filter,
exactly as well (vertices are copied, never recomputed).  The meshes come from mesh.marching_cubes on analytic fields, whose CPU
statement (tests/mc_model.py, tests/test_mesh_cc_model.py) says what pieces to expect."""
import numpy as np
import pytest
import torch

from tests import mc_model
from tests import mesh_cc_model as cc
from tests.gpu_util import launches

pytestmark = pytest.mark.gpu
_cache = {}


def _dev(a, dtype=torch.int32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda:0')


def _labels(tris, n_verts):
    from vqnerf_release_amd.geo.mesh import components
    with launches() as rec:
        labels = components(_dev(np.asarray(tris, np.int32).reshape(-1, 3)), n_verts)
    assert 'vqn_mesh_components' in rec.names
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (n_verts,)
    return labels.cpu().numpy()


def _mesh(name):
    """(vertices, triangles) device tensors, their host copies, the oracle's labels; computed once"""
    if name not in _cache:
        from vqnerf_release_amd.geo.mesh import marching_cubes
        u = cc.two_spheres() if name == 'two_spheres' else cc.sphere_lattice()
        v, t = marching_cubes(_dev(u, torch.float32), 0.0)
        vn, tn = v.cpu().numpy(), t.cpu().numpy()
        _cache[name] = (v, t, vn, tn, cc.components(tn, len(vn)))
    return _cache[name]


def _check_filtered(got, want_v, want_t):
    fv, ft, _ = got
    assert fv.is_cuda and ft.is_cuda and fv.dtype == torch.float32 and ft.dtype == torch.int32
    fv, ft = fv.cpu().numpy(), ft.cpu().numpy()
    assert fv.shape == want_v.shape and ft.shape == want_t.shape
    assert np.array_equal(fv.view(np.int32), want_v.view(np.int32)) and np.array_equal(ft, want_t)
    if len(ft):
        assert ft.min() >= 0 and ft.max() < len(fv)                               # every index < V'
    assert np.array_equal(np.unique(ft), np.arange(len(fv)))                      # every kept vertex is referenced
    return fv, ft


def test_two_spheres():
    from vqnerf_release_amd.geo.mesh import filter_components
    v, t, vn, tn, want = _mesh('two_spheres')
    labels = _labels(tn, len(vn))
    assert len(np.unique(labels)) == 2 and np.array_equal(labels, want)
    with launches() as rec:
        got = filter_components(v, t, keep_largest=1)
    assert {'vqn_mesh_components', 'vqn_mesh_remap_tris'} <= rec.names
    want_v, want_t, sizes, kept = cc.filter_components(vn, tn, keep_largest=1)
    assert sizes[0] > sizes[1]
    fv, ft = _check_filtered(got, want_v, want_t)
    assert got[2] == dict(n_components=2, sizes=sizes, kept=1)
    once, bad = mc_model.boundary_and_bad_edges(ft)
    assert not once and not bad and mc_model.euler_characteristic(len(fv), ft) == 2      # closed: every edge twice
    # the larger sphere's triangles in their original relative order: the same rows of vertex POSITIONS as the input's kept rows
    big = want[tn[:, 0]] == kept[0]
    assert np.array_equal(fv[ft].view(np.int32), vn[tn[big]].view(np.int32))


@pytest.mark.parametrize('ids', ['permuted', 'decreasing'])
def test_long_chain_with_adversarial_ids(ids):
    n = 4096
    rng = np.random.default_rng(17)
    name = rng.permutation(n) if ids == 'permuted' else n - 1 - np.arange(n)      # decreasing: the minimum travels the full length
    tris = name[cc.strip(n)][rng.permutation(n - 2)]
    labels = _labels(tris, n)
    assert (labels == 0).all()


def test_many_small_components():
    from vqnerf_release_amd.geo.mesh import filter_components
    v, t, vn, tn, want = _mesh('lattice')
    labels = _labels(tn, len(vn))
    assert len(np.unique(labels)) == 216 and np.array_equal(labels, want)
    sizes = np.unique(want[tn[:, 0]], return_counts=True)[1]
    smallest = int(sizes.min())
    n_small = int((sizes == smallest).sum())
    assert 0 < n_small < 216
    got = filter_components(v, t, min_faces=smallest + 1)
    want_v, want_t, order, kept = cc.filter_components(vn, tn, min_faces=smallest + 1)
    assert len(kept) == 216 - n_small and len(want_t) == len(tn) - n_small * smallest
    _check_filtered(got, want_v, want_t)
    assert got[2] == dict(n_components=216, sizes=order[:16], kept=216 - n_small)
    # both filters: a piece has to pass both; ties in size go to the smaller label
    got = filter_components(v, t, keep_largest=3, min_faces=smallest + 1)
    want_v, want_t, _, kept = cc.filter_components(vn, tn, keep_largest=3, min_faces=smallest + 1)
    assert len(kept) == 3
    _check_filtered(got, want_v, want_t)
    got = filter_components(v, t, keep_largest=110)                                # reaches into the smaller size by label order
    _check_filtered(got, *cc.filter_components(vn, tn, keep_largest=110)[:2])
    assert got[2]['kept'] == 110


def test_degenerate_inputs():
    from vqnerf_release_amd.geo.mesh import components, filter_components
    empty = torch.zeros((0, 3), dtype=torch.int32, device='cuda:0')
    assert components(empty, 5).cpu().tolist() == [0, 1, 2, 3, 4]                  # T = 0
    assert components(empty, 0).shape == (0,)
    for tris, n in (([[2, 4, 3]], 6),                                             # a single triangle; 0, 1, 5 unreferenced
                    ([[1, 2, 3], [1, 2, 3], [3, 2, 1], [6, 5, 4]], 8),             # duplicates
                    ([[4, 4, 1], [2, 2, 2], [5, 3, 5]], 7)):                       # repeated vertices
        got = _labels(tris, n)
        assert np.array_equal(got, cc.components(np.array(tris), n)), tris
    assert _labels([[2, 4, 3]], 6).tolist() == [0, 1, 2, 2, 2, 5]
    # unreferenced vertices keep their own label, and any active filter drops them
    verts = torch.arange(24, dtype=torch.float32, device='cuda:0').reshape(8, 3)
    tris = _dev([[1, 2, 3], [1, 2, 3], [3, 2, 1], [6, 5, 4]])
    fv, ft, info = filter_components(verts, tris, min_faces=0)
    assert np.array_equal(fv.cpu().numpy(), verts.cpu().numpy()[1:7]) and ft.cpu().tolist() == [[0, 1, 2], [0, 1, 2], [2, 1, 0], [5, 4, 3]]
    assert info == dict(n_components=2, sizes=[3, 1], kept=2)
    fv, ft, info = filter_components(verts, tris, keep_largest=1)
    assert np.array_equal(fv.cpu().numpy(), verts.cpu().numpy()[1:4]) and ft.cpu().tolist() == [[0, 1, 2], [0, 1, 2], [2, 1, 0]]
    # nothing survives / nothing to filter: shapes (0, 3)
    for fv, ft, info in (filter_components(verts, tris, min_faces=4), filter_components(verts, tris, keep_largest=0),
                         filter_components(verts, empty, keep_largest=1), filter_components(verts[:0], empty, min_faces=1)):
        assert tuple(fv.shape) == (0, 3) and tuple(ft.shape) == (0, 3) and fv.dtype == torch.float32 and ft.dtype == torch.int32
        assert info['kept'] == 0


def test_partition_does_not_depend_on_the_numbering():
    _, _, vn, tn, want = _mesh('two_spheres')
    rng = np.random.default_rng(23)
    new_of_old = rng.permutation(len(vn))
    old_of_new = np.argsort(new_of_old)
    labels = _labels(new_of_old[tn][rng.permutation(len(tn))], len(vn))
    assert cc.partition(labels, names=old_of_new) == cc.partition(want)


def test_two_calls_give_the_same_bits():
    from vqnerf_release_amd.geo.mesh import components
    _, t, vn, _, _ = _mesh('lattice')
    a, b = components(t, len(vn)), components(t, len(vn))
    assert torch.equal(a, b)


def test_no_filter_is_the_identity():
    from vqnerf_release_amd.geo.mesh import filter_components
    v, t, _, _, _ = _mesh('two_spheres')
    with launches() as rec:
        fv, ft, info = filter_components(v, t)
    assert fv is v and ft is t and not rec.names and isinstance(info, dict)


def test_argument_errors():
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo.mesh import components, filter_components
    with pytest.raises(_C.VqnError):
        components(torch.zeros((4, 3), dtype=torch.int32), 5)                      # a host tensor: no CPU path
    with pytest.raises(_C.VqnError):
        components(torch.zeros((4, 3), dtype=torch.int64, device='cuda:0'), 5)
    with pytest.raises(_C.VqnError):
        filter_components(torch.zeros((5, 3), device='cuda:0'), torch.zeros((4, 3), dtype=torch.int32, device='cuda:0'), keep_largest=-1)
    lib = _C.lib()
    assert lib.vqn_mesh_components(None, 4, 5, None, None) == -1
    assert lib.vqn_mesh_components(None, -1, 5, None, None) == -1
    assert lib.vqn_mesh_remap_tris(None, 4, None, None, None, 5, None, 2, None) == -1
