"""The cases of tests/cluster_cases.py are in the regimes their names say: shown with the numpy model alone (no GPU)."""
import numpy as np

from tests import cluster_cases as CC

CASES = CC.cases()
F32 = np.float32


def _model(name):
    c = CASES[name]
    xyz, cams = CC.voxel_cloud(c)
    return c, xyz, cams, CC.cluster_model(xyz, c["cp"])


def test_every_case_is_named():
    assert set(CASES) == {"threshold_neighbours", "threshold_neighbours_above", "strict_heights", "strict_heights_inside", "snake",
                          "both_cameras", "size_ties", "seventy_components", "no_foreground", "all_one_component",
                          "fewer_objects_than_K", "non_finite"}
    for c in CASES.values():
        assert 0 < c["cp"]["tolerance"] <= 0.05 and c["cp"]["min_height"] < c["cp"]["max_height"]


def test_threshold_neighbours_sit_on_the_bound_and_one_float_above_it():
    c, xyz, _, m = _model("threshold_neighbours")
    a, b = CC.bridge_pair(xyz)
    d2 = CC.d2_f32(xyz[a:a + 1], xyz[b:b + 1])[0, 0]
    assert d2 == CC.tol2(c["cp"]["tolerance"])
    # no other pair across the two lines is that close: the bridge alone joins them
    fg = np.flatnonzero(CC.foreground(xyz, c["cp"]))
    left, right = fg[:4], fg[4:]
    across = CC.d2_f32(xyz[left], xyz[right])
    assert (across <= d2).sum() == 1 and len(fg) == 8
    assert m["n_components"] == 1 and m["sizes"][0] == 8
    c2, xyz2, _, m2 = _model("threshold_neighbours_above")
    assert np.array_equal(xyz, xyz2)
    assert d2 == np.nextafter(CC.tol2(c2["cp"]["tolerance"]), F32(np.inf))
    assert m2["n_components"] == 2 and list(m2["sizes"][:2]) == [4, 4] and m2["ids"][0] < m2["ids"][1]


def test_strict_heights_exclude_the_bounds_themselves():
    c, xyz, _, m = _model("strict_heights")
    h = CC.heights(xyz, c["cp"]["plane"])
    assert (h == c["cp"]["min_height"]).sum() == 9 and (h == c["cp"]["max_height"]).sum() == 9
    assert m["n_foreground"] == 27 and m["n_components"] == 1
    assert (m["labels"][(h == c["cp"]["min_height"]) | (h == c["cp"]["max_height"])] == 0).all()
    c2, xyz2, _, m2 = _model("strict_heights_inside")
    assert np.array_equal(xyz, xyz2)
    # the bounds one double outwards: the same voxels are now inside the band
    assert m2["n_foreground"] == 45 and m2["sizes"][0] == 45


def test_snake_is_one_long_chain():
    c, xyz, _, m = _model("snake")
    path = CC.snake_path()
    assert len(path) == 619 >= 600
    assert m["n_foreground"] == 619 and m["n_components"] == 1 and m["sizes"][0] == 619
    # one voxel wide: every voxel of the path has two neighbours, its ends one
    fg = np.flatnonzero(CC.foreground(xyz, c["cp"]))
    deg = (CC.d2_f32(xyz[fg], xyz[fg]) <= CC.tol2(c["cp"]["tolerance"])).sum(1) - 1
    assert sorted(np.unique(deg)) == [1, 2] and (deg == 1).sum() == 2
    # the voxel indices along the walk go up and down (x-major order against rows walked in alternating directions)
    lookup = {tuple(np.round((p - np.asarray(CC.ORIGIN)) / CC.CELL).astype(int)): i for i, p in enumerate(xyz.astype(np.float64))}
    idx = np.array([lookup[q] for q in path])
    steps = np.sign(np.diff(idx))
    assert (steps > 0).sum() > 100 and (steps < 0).sum() > 100
    # it winds through far more than 8 cells of the 2 cm search grid and more than one work-group's 256 voxels
    cells = {tuple(np.floor(np.asarray(q) * CC.CELL / 0.02).astype(int)) for q in path}
    assert len(cells) >= 8 and len(path) > 2 * 256


def test_both_cameras_alternate_along_the_component():
    c, xyz, cams, m = _model("both_cameras")
    members = m["lists"][0]
    assert m["n_components"] == 1 and len(members) == 12
    order = members[np.argsort(xyz[members, 0])]
    assert list(cams[order]) == [0, 1] * 6


def test_size_ties_go_to_the_smaller_id():
    _, _, _, m = _model("size_ties")
    assert list(m["sizes"]) == [5, 5, 5] and m["ids"][0] < m["ids"][1] < m["ids"][2] and m["n_objects"] == 3


def test_seventy_components_drop_six_by_rank_and_five_by_size():
    c, _, _, m = _model("seventy_components")
    assert m["n_components"] == 75 and m["n_qualifying"] == 70 and m["n_objects"] == 64 == c["cp"]["max_objects"]
    assert (np.diff(m["sizes"]) <= 0).all() and m["sizes"].min() >= 3
    for a in range(63):  # ties by id
        assert m["sizes"][a] > m["sizes"][a + 1] or m["ids"][a] < m["ids"][a + 1]
    assert (m["labels"] > 0).sum() == m["sizes"].sum() < m["n_foreground"]


def test_the_small_regimes():
    _, xyz, _, m = _model("no_foreground")
    assert len(xyz) == 16 and m["n_foreground"] == 0 and m["n_objects"] == 0 and (m["ids"] == -1).all()
    _, _, _, m = _model("all_one_component")
    assert m["n_components"] == 1 and m["sizes"][0] == 108 and m["sizes"][1] == 0
    _, _, _, m = _model("fewer_objects_than_K")
    assert m["n_objects"] == 2 and list(m["sizes"]) == [6, 3, 0, 0, 0] and len(m["lists"]) == 5


def test_non_finite_points_with_dense_zero():
    c, xyz, cams, m = _model("non_finite")
    assert np.isnan(c["points"]).any() and np.isinf(c["points"]).any() and not c["dense"]
    assert np.isfinite(xyz).all() and set(cams) == {0, 1}
    # the line 0 .. 7 along x is split between the cameras by RANK (two NaNs lie ahead of size_left), and stays one component
    assert list(m["sizes"][:2]) == [8, 3]
    members = m["lists"][0]
    assert set(cams[members]) == {0, 1}
