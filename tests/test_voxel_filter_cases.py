"""tests/voxel_filter_cases.py on the CPU: the numpy model of agh_set_voxel_filter's rules 1 to 3 against an O(N^2) restatement,
and every case in the regime it is named for -- its predicate holds for the model alone, and it both prunes and keeps something
unless it is named otherwise."""
import numpy as np
import pytest

from tests import voxel_filter_cases as VF

CASES = VF.cases()


def test_ball_sizes_are_the_headers():
    assert [VF.B(r) for r in (1, 2, 3, 4)] == [7, 33, 123, 257]
    assert [len({(dx, dy) for dx, dy, _ in VF.ball_offsets(r)}) for r in (1, 2, 3, 4)] == [5, 13, 29, 49]  # the z-runs


@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_model_equals_the_brute_force_count(r):
    rng = np.random.default_rng(r)
    dim = np.array([9, 7, 11])
    ijk = np.unique(rng.integers(0, dim, (300, 3)), axis=0)
    assert np.array_equal(VF.support(ijk, dim, r), VF.support_brute(ijk, r))
    assert VF.support(ijk, dim, r).max() > 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_in_its_regime(name):
    c = CASES[name]
    m = VF.case_model(c)
    print(name, "points", len(c["points"]), "dims", [None if d is None else d.tolist() for d in m["dims"]], "counts", m["counts"].tolist())
    assert c["check"](c, m)
    assert 1 <= c["radius"] <= 4 and 1 <= c["min_neighbors"] <= VF.B(c["radius"]) - 1
    assert np.array_equal(m["counts"][:2], m["counts"][2:4] + m["counts"][4:])
    if c.get("all_pruned"):
        assert not m["keep"].any() and len(m["keep"]) > 0
    else:
        assert m["keep"].any() and not m["keep"].all()
    if len(m["ijk"]) <= 3000:
        for cam in (0, 1):
            sel = m["cam"] == cam
            assert np.array_equal(m["support"][sel], VF.support_brute(m["ijk"][sel], c["radius"]))
    xyz, cam = VF.filtered_cloud(c["points"], VF.case_cams(c), c["workspace"], c["cell"], m["keep"])
    assert len(xyz) == m["counts"][4:].sum() and np.array_equal(np.bincount(cam, minlength=2), m["counts"][4:])


def test_cameras_cases_put_camera_1_behind_a_block_of_camera_0():
    for name in ("cam1_seams", "cam1_wrap_pairs", "cam1_wrap_filled_box", "cam1_block_neighbours"):
        m = VF.case_model(CASES[name])
        assert m["dims"][0] is not None and m["dims"][1] is not None and m["counts"][0] > 0 and m["counts"][1] > 0
    m = VF.case_model(CASES["only_cam1_wrap_pairs"])
    assert m["dims"][0] is None and m["counts"][0] == 0
    assert all(VF.case_model(CASES[n])["dims"][1] is None for n in ("seams", "dense_block", "last_word"))  # no camera-1 point


def test_speckle_parameters_prune_the_injected_voxels_and_spare_the_rest():
    c = VF.speckle_capture()
    cams = VF.case_cams(c)
    m = VF.case_model(c)
    # a voxel is "injected" iff only injected kept points fall into it
    clean = VF.filter_model(c["points"][~c["injected"]], cams[~c["injected"]], c["workspace"], c["cell"], 1, 1)
    n_clean = len(clean["keep"])
    full = {(int(k), *v) for k, v in zip(m["cam"], m["ijk"].tolist())}
    # (the injected points lie inside the box of the kept ones: the minima, so the lattices, are the clean capture's)
    base = {(int(k), *v) for k, v in zip(clean["cam"], clean["ijk"].tolist())}
    assert base <= full
    inj = np.array([(int(k), *v) not in base for k, v in zip(m["cam"], m["ijk"].tolist())])
    pruned_inj = (~m["keep"][inj]).mean()
    pruned_rest = (~m["keep"][~inj]).mean()
    print("voxels", len(full), "clean", n_clean, "injected", int(inj.sum()), "pruned of injected", pruned_inj, "of the rest", pruned_rest)
    assert inj.sum() >= 0.9 * VF.SPECKLE["n_injected"]
    assert pruned_inj >= 0.9 and pruned_rest <= 0.01
