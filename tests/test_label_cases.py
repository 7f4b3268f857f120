"""tests/label_cases.py: every case is in the regime its name claims, by the numpy model alone (no GPU, no library)."""
import numpy as np
import pytest

from tests import depth_captures as D
from tests import label_cases as L
from tests import mask_cases as M

CASES = L.point_cases()


def _model(name):
    c = CASES[name]
    cams = L.cams_of(c)
    return c, cams, L.eligible_lists(c, cams)


def _bits(c, cams):
    """raw index -> (camera, bit position in the camera's lattice)"""
    out = {}
    for sel, cam, pos, _dim in M.bit_positions(c["points"], cams, c["workspace"], c["cell"]):
        for i, p in zip(sel, pos):
            out[int(i)] = (cam, int(p))
    return out


def test_the_cases_the_issue_names_exist():
    want = {"k1", "dup_voxel", "values", "word_edge", "block_edge", "dense_block", "two_cameras_same_lattice", "rank_cameras",
            "dropped", "all_dropped", "stride32", "k64"} | {"row_%d" % n for n in L.ROWS}
    assert set(CASES) == want
    for name, c in CASES.items():
        assert 1 <= c["n_objects"] <= 64 and c["labels"].dtype == np.uint8, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_are_ascending_and_inside_the_cloud(name):
    c, cams, E = _model(name)
    keep = cams >= 0
    nv = len(D.voxel_model(c["points"][keep, :3], cams[keep], c["workspace"], c["cell"])[0])
    assert len(E) == c["n_objects"]
    for e in E:
        assert np.all(np.diff(e) > 0) and (len(e) == 0 or (0 <= e[0] and e[-1] < nv))
    # a raw point adds at most one (voxel, object) pair: the lists share a buffer of n entries
    assert sum(len(e) for e in E) <= len(c["points"])


def test_one_voxel_in_two_lists():
    c, cams, E = _model("dup_voxel")
    assert len(np.intersect1d(E[0], E[1])) == 1 and len(E[0]) == len(E[1]) == 1


def test_bytes_above_n_objects_belong_to_no_object():
    c, cams, E = _model("values")
    assert c["n_objects"] == 2 and (c["labels"] == 255).sum() > 10
    only = M.eligible_model(c["points"], cams, c["labels"] == 255, c["workspace"], c["cell"])
    assert len(np.setdiff1d(only, np.concatenate(E))) > 0  # voxels that a mask would make eligible and no object has
    assert len(E[0]) > 10 and len(E[1]) > 10


def test_word_and_block_seams_separate_objects():
    c, cams, E = _model("word_edge")
    bits = _bits(c, cams)
    assert bits[1 + 31] == (0, 31) and bits[1 + 32] == (0, 32) and c["labels"][32] == 1 and c["labels"][33] == 2
    assert list(E[0]) == [31] and list(E[1]) == [32]
    c, cams, E = _model("block_edge")
    bits = _bits(c, cams)
    assert bits[2] == (0, 131071) and bits[3] == (0, 131072) and c["labels"][2] == 1 and c["labels"][3] == 2
    assert [len(e) for e in E] == [2, 2, 1]


def test_dense_block_fills_every_wave():
    c, cams, E = _model("dense_block")
    assert sum(len(e) for e in E) == 33 * 64 * 64 >= 131072  # every voxel of the lattice belongs to exactly one object
    assert all(len(e) > 40000 for e in E)
    both = np.sort(np.concatenate(E))
    assert np.array_equal(both, np.arange(33 * 64 * 64))


def test_camera_blocks():
    c, cams, E = _model("two_cameras_same_lattice")
    n0 = M.voxel_counts(c["points"], cams, c["workspace"], c["cell"])[0]
    assert n0 > 0 and all(len(e) > 3 and e[0] >= n0 for e in E)  # objects in camera 1's block only
    c, cams, E = _model("rank_cameras")
    by_raw = (np.arange(len(c["points"])) >= c["size_left"]).astype(np.int32)
    assert not np.array_equal(cams[cams >= 0], by_raw[cams >= 0])  # the rank rule, not the raw index
    assert [len(e) for e in E] == [1, 2]  # (raw point 0, a NaN with label 1, is dropped)
    assert E[1][0] < M.voxel_counts(c["points"], cams, c["workspace"], c["cell"])[0] <= E[1][1]  # object 1 in both blocks


def test_dropped_points_make_an_empty_object_between_two_others():
    c, cams, E = _model("dropped")
    assert [len(e) for e in E] == [1, 0, 1] and (c["labels"] == 2).sum() > 5
    c, cams, E = _model("all_dropped")
    assert [len(e) for e in E] == [0, 0, 0] and all((c["labels"] == j + 1).sum() > 0 for j in range(3))


def test_strides_and_object_counts():
    c, cams, E = _model("stride32")
    assert c["points"].shape[1] == 8 and c["n_objects"] == 4 and all(len(e) > 5 for e in E)
    c, cams, E = _model("k64")
    assert c["n_objects"] == 64 and [len(e) for e in E] == [1] * 64 and len(set(int(e[0]) for e in E)) == 64
    c, cams, E = _model("k1")
    assert c["n_objects"] == 1 and len(E[0]) == 1


@pytest.mark.parametrize("n", L.ROWS)
def test_rows_alternate(n):
    c, cams, E = _model("row_%d" % n)
    assert np.array_equal(E[0], np.arange(0, n, 2)) and np.array_equal(E[1], np.arange(1, n, 2))


def test_tiled_labels():
    t = L.tiled_labels((240, 320))
    assert t.min() == 1 and t.max() == 12 and t[0, 0] == 1 and t[0, -1] == 4 and t[-1, 0] == 9 and t[-1, -1] == 12
    assert all((t == k).sum() == 240 * 320 // 12 for k in range(1, 13))
