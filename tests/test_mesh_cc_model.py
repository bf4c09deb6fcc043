"""CPU: tests/mesh_cc_model.py, the oracle of the device mesh components -- its labels are the component minima, and the fields it
hands the GPU tests are what their docstrings say (through tests/mc_model.py, the CPU statement of the device mesher)."""
import numpy as np

from tests import mc_model
from tests import mesh_cc_model as cc


def test_labels_are_component_minima():
    tris = np.array([[5, 3, 4], [4, 6, 6], [1, 2, 1], [8, 8, 8]], np.int32)
    assert cc.components(tris, 10).tolist() == [0, 1, 1, 3, 3, 3, 3, 7, 8, 9]
    assert cc.components(np.zeros((0, 3), np.int32), 4).tolist() == [0, 1, 2, 3]
    assert cc.partition([0, 1, 1, 3], names=[7, 8, 9, 4]) == {frozenset({7}), frozenset({8, 9}), frozenset({4})}


def test_strip_in_decreasing_ids_is_one_component():
    n = 257
    assert (cc.components(n - 1 - cc.strip(n), n) == 0).all()


def test_lattice_is_216_closed_pieces_of_two_sizes():
    v, t = mc_model.marching_cubes(cc.sphere_lattice(), 0.0, np.float32)
    labels = cc.components(t, len(v))
    assert len(np.unique(labels)) == 216
    once, bad = mc_model.boundary_and_bad_edges(t)
    assert not once and not bad and mc_model.euler_characteristic(len(v), t) == 2 * 216
    sizes = np.unique(labels[t[:, 0]], return_counts=True)[1]
    assert sorted(np.unique(sizes, return_counts=True)[1].tolist()) == [108, 108] and sizes.min() >= 8


def test_filter_statement_keeps_order_and_references():
    v, t = mc_model.marching_cubes(cc.two_spheres(), 0.0, np.float32)
    fv, ft, sizes, kept = cc.filter_components(v, t, keep_largest=1)
    assert len(sizes) == 2 and sizes[0] > sizes[1] and len(kept) == 1 and len(ft) == sizes[0]
    assert sorted(np.unique(ft).tolist()) == list(range(len(fv)))
    once, bad = mc_model.boundary_and_bad_edges(ft)
    assert not once and not bad and mc_model.euler_characteristic(len(fv), ft) == 2
