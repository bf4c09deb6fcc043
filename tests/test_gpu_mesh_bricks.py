"""GPU: the sparse mesh export -- csrc/marching_cubes_bricks.hip through geo/mesh.py marching_cubes_bricks / extract_geometry_sparse,
NeuSRenderer.extract_geometry(sparse=True) and Runner.validate_mesh(sparse=True).

The reference is the dense route (tests/test_gpu_mesh.py holds that one to the field and to the NumPy model): the sparse route has to
return the same bytes, so every comparison here is torch.equal / array_equal on the bit patterns, with no tolerance.  Past the size
the dense route refuses there is nothing to compare with; there the mesh of an analytic sphere is held to its topology and to the
distance of its vertices from the sphere.
"""
import os

import numpy as np
import pytest
import torch

from tests import mc_model
from tests.gpu_util import launches
from tests.mesh_bricks_util import FIELDS, GRIDS, THRESHOLD, brick_list, crossing_bricks, field, gather_bricks
from tests.test_gpu_mesh import neus  # noqa: F401  (the fixture: the geometric-init test network, seed 11)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = 'cuda:0'
ORIGIN, STEP = np.array([-1.0, 0.5, 2.0]), np.array([0.25, 0.5, 2.0])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('name', FIELDS)
def test_bricks_give_the_dense_mesh_bit_for_bit(name, shape):
    from vqnerf_release_amd.geo.mesh import marching_cubes, marching_cubes_bricks
    u, thr = field(name, shape, DEV), THRESHOLD[name]
    cross = crossing_bricks(u, thr)
    assert cross.any()
    if name == 'noise':
        assert cross.all()                                                   # every brick is active ...
    if name == 'noise' and min(shape) > 30:
        un = u.cpu().numpy() > np.float32(thr)
        case = sum(un[x: shape[0] - 1 + x, y: shape[1] - 1 + y, z: shape[2] - 1 + z].astype(np.int64) << c
                   for c, (x, y, z) in enumerate(map(mc_model.corner_offset, range(8))))
        assert len(np.unique(case)) == 256                                   # ... and every case occurs
    dense = marching_cubes(u, thr)
    dense_w = marching_cubes(u, thr, origin=ORIGIN, step=STEP)
    assert dense[1].shape[0] > 0
    extra = np.random.default_rng(7).random(cross.shape) < 0.25              # (b): the crossing bricks and a random quarter of the others
    for mask in (np.ones_like(cross), cross | extra):
        ijk = brick_list(mask, DEV)
        ub = gather_bricks(u, ijk)                                           # NaN in the padding of clipped bricks: must not be read
        with launches() as rec:
            v, t, leaks = marching_cubes_bricks(ub, ijk, shape, thr)
        assert {'vqn_mc_brick_classify', 'vqn_mc_brick_emit'} <= rec.names
        assert leaks == 0 and v.dtype == torch.float32 and t.dtype == torch.int32
        assert torch.equal(t, dense[1]) and torch.equal(_bits(v), _bits(dense[0]))
        vw, tw, leaks = marching_cubes_bricks(ub, ijk, shape, thr, origin=ORIGIN, step=STEP)
        assert leaks == 0 and torch.equal(tw, dense_w[1]) and torch.equal(_bits(vw), _bits(dense_w[0]))


@pytest.mark.parametrize('value', [1.0, -1.0])
def test_nothing_crosses(value):
    from vqnerf_release_amd.geo.mesh import marching_cubes_bricks
    u = torch.full((17, 9, 12), value, device=DEV)
    for mask in (np.ones((2, 1, 2), bool), np.zeros((2, 1, 2), bool)):       # all bricks, and an empty list
        ijk = brick_list(mask, DEV)
        v, t, leaks = marching_cubes_bricks(gather_bricks(u, ijk), ijk, u.shape, 0.0)
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32 and leaks == 0


def test_a_surface_cut_by_a_missing_brick_is_reported_and_stays_in_bounds():
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo.mesh import brick_offsets, marching_cubes_bricks
    shape = (38, 38, 38)
    u = field('sphere', shape, DEV)
    cross = crossing_bricks(u, 0.0)
    where = np.argwhere(cross)
    cross[tuple(where[len(where) // 2])] = False                             # one brick the surface passes through, left out
    ijk = brick_list(cross, DEV)
    ub = gather_bricks(u, ijk)
    v, t, leaks = marching_cubes_bricks(ub, ijk, shape, 0.0)                 # an error path, not a fault: it completes
    assert leaks > 0 and v.shape[0] > 0 and t.shape[0] > 0
    assert int(t.min()) >= 0 and int(t.max()) < v.shape[0]                   # every index in range, also next to the hole
    # the same emit into arrays one element larger: the guard elements stay as they were
    slot, voff, toff, n_verts, n_tris, leaks2 = brick_offsets(ub, ijk, shape, 0.0)
    assert leaks2 == leaks and (n_verts, n_tris) == (v.shape[0], t.shape[0])
    gv = torch.full((n_verts + 1, 3), 777.0, device=DEV)
    gt = torch.full((n_tris + 1, 3), -777, dtype=torch.int32, device=DEV)
    _C.mc_brick_emit(ub, ijk, slot, shape, 0.0, voff, toff, n_verts, n_tris, out=(gv, gt))
    assert (gv[-1] == 777.0).all() and (gt[-1] == -777).all()
    assert torch.equal(gt[:-1], t) and torch.equal(_bits(gv[:-1]), _bits(v))


# ---- a real network ---------------------------------------------------------------------------------------------------------------
BMIN, BMAX = [-1.0, -0.9, -1.1], [1.0, 1.1, 0.9]


@pytest.mark.parametrize('resolution', [65, 38])
def test_sparse_extract_geometry_equals_the_dense_call(neus, resolution):  # noqa: F811
    from vqnerf_release_amd.geo.mesh import extract_geometry_sparse
    bmin, bmax = torch.tensor(BMIN), torch.tensor(BMAX)
    v, t = neus.extract_geometry(bmin, bmax, resolution=resolution, threshold=0.0)
    with launches() as rec:
        vs, ts = neus.extract_geometry(bmin, bmax, resolution=resolution, threshold=0.0, sparse=True)
    assert {'vqn_neus_sdf_points', 'vqn_mc_brick_points', 'vqn_mc_brick_classify', 'vqn_mc_brick_emit'} <= rec.names
    assert 'vqn_mc_classify' not in rec.names
    assert len(t) > 100 and np.array_equal(ts, t) and np.array_equal(vs.view(np.int32), v.view(np.int32))
    _, _, info = extract_geometry_sparse(bmin, bmax, resolution, 0.0, neus.sdf_network)
    print(f'[info] resolution {resolution}: {info}')
    assert info['leaks'] == 0 and info['bricks_total'] == (-(-(resolution - 1) // 8)) ** 3
    assert info['points_evaluated'] == info['bricks_total'] + 729 * info['bricks_active']
    if resolution == 65:
        assert info['bricks_active'] < info['bricks_total']


def test_a_lipschitz_bound_that_is_too_small_raises(neus):  # noqa: F811
    from vqnerf_release_amd import _C
    with pytest.raises(_C.VqnError, match='lipschitz'):
        neus.extract_geometry(torch.tensor(BMIN), torch.tensor(BMAX), resolution=65, threshold=0.0, sparse=True, lipschitz=1.0)


def test_validate_mesh_writes_the_same_bytes(tmp_path):
    from vqnerf_release_amd.geo.nerf_runner import Runner, SyntheticDataset
    text = open(os.path.join(HERE, 'golden', 'neus_like.conf')).read().replace('./exp/', str(tmp_path) + '/exp/')
    torch.manual_seed(3)
    r = Runner(conf_text=text, case='mesh', dataset=SyntheticDataset(n_images=2, H=32, W=32))
    for kwargs in (dict(), dict(keep_largest=1, normals=True, colors=True)):
        dense = open(r.validate_mesh(resolution=32, **kwargs), 'rb').read()
        with launches() as rec:
            path = r.validate_mesh(resolution=32, sparse=True, **kwargs)
        assert 'vqn_mc_brick_emit' in rec.names and 'vqn_mc_emit' not in rec.names
        sparse = open(path, 'rb').read()
        assert len(dense) > 1000 and sparse == dense


# ---- past the dense limit ---------------------------------------------------------------------------------------------------------
def test_a_sphere_on_a_grid_the_dense_route_refuses():
    """R = 1297: 1297^3 > 2^31 grid points.  A sphere of radius 0.4 R around (760, 648, 648) in index coordinates: it lies inside the
    grid and reaches i = 1278, so owned points with a linear index above 2^31 (i >= 1277) carry vertices.  Only the bricks that
    intersect the shell are listed (picked from the bricks' boxes: nearest point <= r <= farthest point, with one cell of slack), the
    field on them is built by formula; 1297^3 values would be 8.7 GB."""
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo.mesh import components, marching_cubes_bricks
    R, r = 1297, 0.4 * 1297
    c = (760.0, 648.0, 648.0)
    assert _C.lib().vqn_mc_classify(None, R, R, R, 0.0, None, None, None) == -2          # the dense route refuses this shape
    nb = -(-(R - 1) // 8)
    b = torch.arange(nb, device=DEV, dtype=torch.float64)
    lo, hi = 8 * b, torch.clamp(8 * b + 8, max=R - 1)
    near2, far2 = [], []
    for a in range(3):
        near2.append(torch.clamp(torch.maximum(lo - c[a], c[a] - hi), min=0.0) ** 2)
        far2.append(torch.maximum((lo - c[a]).abs(), (hi - c[a]).abs()) ** 2)
    near = torch.sqrt(near2[0][:, None, None] + near2[1][None, :, None] + near2[2][None, None, :])
    far = torch.sqrt(far2[0][:, None, None] + far2[1][None, :, None] + far2[2][None, None, :])
    ijk = torch.nonzero((near <= r + 1.0) & (far >= r - 1.0)).to(torch.int32).contiguous()   # sorted by brick linear index
    n = ijk.shape[0]
    assert 50_000 < n and n * 729 < 1 << 31
    l = torch.arange(9, device=DEV, dtype=torch.float32)
    x, y, z = [(8 * ijk[:, a].float())[:, None] + l[None, :] - c[a] for a in range(3)]     # one formula per grid point: equal bits in every brick
    ub = (r - torch.sqrt(x[:, :, None, None] ** 2 + y[:, None, :, None] ** 2 + z[:, None, None, :] ** 2)).contiguous()
    v, t, leaks = marching_cubes_bricks(ub, ijk, (R, R, R), 0.0)
    assert leaks == 0
    V, T = v.shape[0], t.shape[0]
    assert V > 1_000_000 and int(t.min()) >= 0 and int(t.max()) == V - 1
    assert float(v[:, 0].max()) > 1277.0                                                   # vertices owned by points past 2^31
    labels = components(t, V)
    assert bool((labels == 0).all())                                                       # one piece
    assert 2 * V - T == 4                                                                  # V - T / 2 = 2: a closed surface of genus 0
    d = torch.sqrt(((v.double() - torch.tensor(c, device=DEV, dtype=torch.float64)) ** 2).sum(1))
    assert float((d - r).abs().max()) <= 1.0                                               # every vertex within one cell of the sphere


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from vqnerf_release_amd import _C
    from vqnerf_release_amd.geo.mesh import marching_cubes_bricks
    ijk = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    ub = torch.zeros((1, 9, 9, 9), device=DEV)
    with pytest.raises(_C.VqnError, match=r'rc=-2'):
        marching_cubes_bricks(ub, ijk, (1, 8, 8), 0.0)
    with pytest.raises(_C.VqnError):
        marching_cubes_bricks(ub.cpu(), ijk, (9, 9, 9), 0.0)                                # a host tensor: no CPU path
    with pytest.raises(_C.VqnError, match='origin and step'):
        marching_cubes_bricks(ub, ijk, (9, 9, 9), 0.0, origin=[0.0, 0.0, 0.0])
    with pytest.raises(_C.VqnError, match='9, 9, 9'):
        marching_cubes_bricks(ub, torch.zeros((2, 3), dtype=torch.int32, device=DEV), (9, 9, 9), 0.0)    # ub does not match the list
    lib = _C.lib()
    err = lambda: lib.vqn_last_error().decode()
    # dimensions < 2
    assert lib.vqn_mc_brick_points(None, None, None, 8, 1, 8, None, 1, 0, 729, None, None) == -2 and '>= 2' in err()
    assert lib.vqn_mc_brick_classify(None, None, 1, None, 8, 8, 1, 0.0, None, None, None, None, None) == -2 and '>= 2' in err()
    assert lib.vqn_mc_brick_emit(None, None, 1, None, 1, 8, 8, 0.0, None, None, 4, 4, None, None, None, None, None) == -2 and '>= 2' in err()
    # a brick grid of 2^31 entries (8 * 2^11 + 1 points along x and y, 8 * 2^9 + 1 along z)
    big = (16385, 16385, 4097)
    assert lib.vqn_mc_brick_classify(None, None, 1, None, *big, 0.0, None, None, None, None, None) == -2 and 'brick grid' in err()
    assert lib.vqn_mc_brick_emit(None, None, 1, None, *big, 0.0, None, None, 4, 4, None, None, None, None, None) == -2 and 'brick grid' in err()
    assert lib.vqn_mc_brick_points(None, None, None, *big, None, 1, 0, 729, None, None) == -2 and 'brick grid' in err()
    # n_bricks * 729 >= 2^31
    many = -(-(1 << 31) // 729)
    assert lib.vqn_mc_brick_classify(None, None, many, None, 65, 65, 65, 0.0, None, None, None, None, None) == -2 and '729' in err()
    assert lib.vqn_mc_brick_emit(None, None, many, None, 65, 65, 65, 0.0, None, None, 4, 4, None, None, None, None, None) == -2 and '729' in err()
    assert lib.vqn_mc_brick_points(None, None, None, 65, 65, 65, None, many, 0, 729, None, None) == -2 and '729' in err()
    # totals outside int32, a range outside the list, negative sizes
    assert lib.vqn_mc_brick_emit(None, None, 1, None, 65, 65, 65, 0.0, None, None, 1 << 31, 4, None, None, None, None, None) == -1 and '2^31' in err()
    assert lib.vqn_mc_brick_emit(None, None, 1, None, 65, 65, 65, 0.0, None, None, 4, -1, None, None, None, None, None) == -1
    assert lib.vqn_mc_brick_points(None, None, None, 65, 65, 65, None, 1, 1, 729, None, None) == -1 and 'first' in err()
    assert lib.vqn_mc_brick_classify(None, None, -1, None, 65, 65, 65, 0.0, None, None, None, None, None) == -1
    # null pointers
    assert lib.vqn_mc_brick_points(None, None, None, 65, 65, 65, None, 1, 0, 729, None, None) == -1 and 'null' in err()
    assert lib.vqn_mc_brick_classify(None, None, 1, None, 65, 65, 65, 0.0, None, None, None, None, None) == -1 and 'null' in err()
    assert lib.vqn_mc_brick_emit(None, None, 1, None, 65, 65, 65, 0.0, None, None, 4, 4, None, None, None, None, None) == -1 and 'null' in err()
