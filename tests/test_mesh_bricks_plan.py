"""CPU: the brick plan of the sparse mesh export (geo/mesh.py plan_bricks) -- ownership, storage, clipping, centres and radii -- the
ABI rows of its three entry points, and the sparse option on a network that has no device route."""
import numpy as np
import pytest
import torch

from vqnerf_release_amd import _C
from vqnerf_release_amd.geo.mesh import BRICK, plan_bricks

RESOLUTIONS = (2, 9, 10, 17, 38, 65)


@pytest.mark.parametrize('R', RESOLUTIONS)
def test_every_point_has_one_owner_and_every_cell_one_brick_that_stores_its_corners(R):
    plan = plan_bricks(R)
    assert plan.dims == (R, R, R) and plan.brick == BRICK == 8
    for a in range(3):
        nb, lo, hi, owner = plan.nb[a], plan.lo[a], plan.hi[a], plan.owner[a]
        assert nb == -(-(R - 1) // 8) and len(lo) == len(hi) == nb and len(owner) == R
        # clipped extents: brick b stores 8 b .. min(8 b + 8, R - 1); only the last one may be short, with 1..8 cells
        assert np.array_equal(lo, 8 * np.arange(nb)) and np.array_equal(hi, np.minimum(lo + 8, R - 1))
        assert ((hi - lo)[:-1] == 8).all() and 1 <= hi[-1] - lo[-1] <= 8 and hi[-1] == R - 1 and lo[0] == 0
        # every point: exactly one owner, which stores it; the last point of the grid goes to the last brick
        assert np.array_equal(owner, np.minimum(np.arange(R) // 8, nb - 1)) and owner[-1] == nb - 1
        stores = (lo[:, None] <= np.arange(R)[None]) & (np.arange(R)[None] <= hi[:, None])                 # [brick, point]
        assert stores[owner, np.arange(R)].all()
        # every cell (its minimum corner i, i < R - 1): its owner's brick stores i and i + 1, and no other brick holds the cell
        cell = np.arange(R - 1)
        holds = (lo[:, None] <= cell[None]) & (cell[None] + 1 <= hi[:, None])                              # brick holds both ends
        assert holds[owner[:-1], cell].all() and (holds.sum(0) == 1).all()
    # the three axes are independent, so the statements hold for the products: points, cells and their 8 corners


def test_unequal_dimensions():
    plan = plan_bricks((17, 9, 12))
    assert plan.nb == (2, 1, 2) and [list(h) for h in plan.hi] == [[8, 16], [8], [8, 11]]
    assert [list(c) for c in plan.centre] == [[4, 12], [4], [4, 9]]
    with pytest.raises(ValueError):
        plan_bricks(1)


@pytest.mark.parametrize('R', RESOLUTIONS)
def test_centres_are_grid_points_and_the_radius_covers_every_stored_point(R):
    bmin, bmax = torch.tensor([-1.0, -0.35, -2.2]), torch.tensor([1.3, 0.4, 2.2])                          # anisotropic
    axes = [torch.linspace(bmin[a], bmax[a], R).numpy() for a in range(3)]                                 # as mesh._axes builds them
    plan = plan_bricks(R, axes=axes)
    assert plan.h.dtype == np.float32 and plan.h.shape == plan.nb
    for a in range(3):
        c = plan.centre[a]
        assert np.array_equal(c, plan.lo[a] + (plan.hi[a] - plan.lo[a]) // 2) and (plan.lo[a] <= c).all() and (c <= plan.hi[a]).all()
    ax64 = [x.astype(np.float64) for x in axes]
    worst = np.inf
    for bi in range(plan.nb[0]):
        for bj in range(plan.nb[1]):
            for bk in range(plan.nb[2]):
                b = (bi, bj, bk)
                pts = np.stack(np.meshgrid(*[ax64[a][plan.lo[a][b[a]]: plan.hi[a][b[a]] + 1] for a in range(3)], indexing='ij'), -1)
                centre = np.array([ax64[a][plan.centre[a][b[a]]] for a in range(3)])
                far = np.sqrt(((pts - centre) ** 2).sum(-1)).max()
                h = float(plan.h[b])
                assert h >= far
                worst = min(worst, h - far)
                assert h <= far * (1 + 2.0 ** -22)                                                          # rounded up, not padded
    assert worst >= 0


def test_the_new_entry_points_are_declared_in_both_places():
    from tests import abi_headers
    declared = abi_headers.prototypes('vqn_mesh.h')
    for name in ('vqn_mc_brick_points', 'vqn_mc_brick_classify', 'vqn_mc_brick_emit'):
        assert name in declared and _C.ABI_BY_HEADER['vqn_mesh.h'][name] == declared[name] and name not in _C.ABI


def test_sparse_needs_the_device_route():
    from vqnerf_release_amd.geo.models.fields import SDFNetwork
    from vqnerf_release_amd.geo.models.renderer import NeuSRenderer
    torch.manual_seed(0)
    sdf = SDFNetwork(d_out=65, d_in=3, d_hidden=64, n_layers=4, skip_in=(2,), multires=6, bias=0.5, scale=1.0, geometric_init=True,
                     weight_norm=True)                                                                      # on the CPU: the mcubes route
    ren = NeuSRenderer(None, sdf, None, None, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=1.0)
    with pytest.raises(_C.VqnError, match='sparse'):
        ren.extract_geometry(torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=8, sparse=True)
