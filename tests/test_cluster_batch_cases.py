"""The batches of tests/cluster_batch_cases.py are in the regimes the GPU tests claim: shown with the numpy models alone (no GPU)."""
import numpy as np
import pytest

from tests import cluster_batch_cases as B
from tests import cluster_cases as CC
from tests import cluster_grid_cases as G
from tests import depth_captures as D
from tests import grid_scale_clouds as gs
from tests import mask_cases as M


def test_the_twelve_cases_and_their_lists():
    batch = B.small_batch()
    assert tuple(n for n, _ in batch) == B.SMALL_ORDER and len(batch) == 12
    assert tuple(c["cp"]["max_objects"] for _, c in CC.cases().items()) == B.SMALL_MAX_OBJECTS == (4, 4, 4, 4, 4, 4, 3, 64, 4, 2, 5, 4)
    assert sum(c["cp"]["max_objects"] for _, c in batch) == 64  # seventy_components lowered to 22 lists: exactly L = 64
    assert sum(c["cp"]["max_objects"] for _, c in B.small_batch(23)) == 65
    first = B.first_lists(batch)
    assert first.tolist() == [0, 4, 8, 12, 16, 20, 24, 27, 49, 53, 55, 60, 64]
    assert B.SMALL_ORDER.index("no_foreground") == 8  # in the middle: captures with lists on both sides
    assert len({c["cell"] for _, c in batch}) == 1
    assert B.small_samples(batch) == [7, 7, 7, 7, 40, 7, 7, 7, 7, 7, 7, 7]
    assert sum(c["cp"]["max_objects"] * S for (_, c), S in zip(batch, B.small_samples(batch))) <= 1 << 24


def test_seventy_components_with_22_lists():
    c = dict(B.small_batch())["seventy_components"]
    xyz, _ = CC.voxel_cloud(c)
    m = CC.cluster_model(xyz, c["cp"])
    assert c["cp"]["max_objects"] == 22 and c["cp"]["min_voxels"] == 3
    assert (m["n_components"], m["n_qualifying"], m["n_objects"]) == (75, 70, 22)
    assert (m["sizes"] >= 3).all() and (np.diff(m["sizes"]) <= 0).all()


def test_the_threshold_captures_are_the_same_points_with_two_tolerances():
    cases = dict(B.small_batch())
    a, b = cases["threshold_neighbours"], cases["threshold_neighbours_above"]
    assert np.array_equal(a["points"], b["points"]) and len(a["points"]) == 9
    assert a["cp"]["tolerance"] != b["cp"]["tolerance"]
    assert {k: v for k, v in a["cp"].items() if k != "tolerance"} == {k: v for k, v in b["cp"].items() if k != "tolerance"}
    xyz, _ = CC.voxel_cloud(a)
    assert CC.cluster_model(xyz, a["cp"])["n_components"] == 1 and CC.cluster_model(xyz, b["cp"])["n_components"] == 2


def test_the_grid_batch_has_cells_of_four_sizes_and_reach_2_3_1_1():
    batch = B.grid_batch()
    assert tuple(n for n, _ in batch) == B.GRID_ORDER
    assert all(c["cell"] == 0.01 for _, c in batch)  # 1 cm voxels throughout
    clouds = [CC.voxel_cloud(c)[0] for _, c in batch]
    descs = gs.GridModel().build(clouds)
    assert tuple(d.cell for d, _ in descs) == B.GRID_CELLS == (0.04, 0.02, 0.08, 0.02)
    assert tuple(G.reach_of(c["cp"]["tolerance"], d.cell) for (_, c), (d, _) in zip(batch, descs)) == B.GRID_REACH == (2, 3, 1, 1)
    assert [len(x) for x in clouds] == [5332, 620, 5332, 16]  # uneven sizes: the launches are sized from the largest
    assert sum(c["cp"]["max_objects"] for _, c in batch) <= 64


@pytest.mark.parametrize("k, want", [(0, (20488, [1928, 902, 473])), (1, (20502, [1929, 931, 470])), (2, (20404, [1907, 906, 470]))])
def test_the_table_scenes_have_three_objects_each(k, want):
    s = B.table_scenes()[k]
    assert (B.TABLE_SEEDS, B.TABLE_K, B.TABLE_S) == ((5, 6, 7), (4, 3, 5), (60, 45, 60))
    cams = M.camera_ids(s["xyz"], s["size_left"], True)
    xyz, _ = D.voxel_model(np.asarray(s["xyz"]), cams, s["ws"], 0.003)
    m = CC.cluster_model(xyz, s["cp"])
    assert (len(xyz), m["sizes"][:3].tolist()) == want and m["n_objects"] == 3
    assert m["n_qualifying"] == 3  # K = 3 is exactly enough, K = 4 and 5 leave empty lists
