"""tests/plane_fit_cases.py: every case is in the regime it is named after, shown from the numpy model alone.  Needs no GPU."""
import numpy as np
import pytest

from tests import cluster_cases as CC
from tests import depth_captures as D
from tests import mask_cases as M
from tests import plane_fit_cases as PF

CASES = PF.cases()


@pytest.fixture(scope="module")
def models():
    return {name: PF.case_model(c) for name, c in CASES.items()}


def _xyz(name):
    return PF.voxel_cloud(CASES[name])[0]


def test_floor_blocks_sizes(models):
    small, large = models["floor_blocks_small"], models["floor_blocks_large"]
    assert 3 <= small["n_voxels"] < 256  # one partial work-group
    assert large["n_voxels"] > 3 * 512 and large["n_voxels"] % 64 != 0  # several work-groups, a partial last wave
    for m, floor in ((small, 144), (large, 40 * 41)):
        assert m["found"] and m["refined"] and m["n_inliers"] == m["n_refit"] == floor
        assert m["plane"][2] > 0.999999  # the floor's normal, towards the camera over it


def test_ties(models):
    m = models["ties"]
    top = np.flatnonzero(m["counts"] == m["counts"].max())
    assert len(top) >= 2 and top[0] != 0 and m["best_candidate"] == top[0]
    assert m["n_inliers"] == 144 and PF.is_level(m["planes"][top[0]])


def test_threshold_twins(models):
    a, b = models["threshold_exact"], models["threshold_below"]
    xyz = _xyz("threshold_exact")
    layer = int((xyz[:, 2] == np.unique(xyz[:, 2])[1]).sum())
    assert layer == 8
    assert CASES["threshold_below"]["fp"]["distance_threshold"] == np.nextafter(CASES["threshold_exact"]["fp"]["distance_threshold"], 0.0)
    for m in (a, b):
        assert PF.is_level(m["planes"][m["best_candidate"]])
    # h = z - z0 exactly: the layer's height is the threshold itself
    h = np.abs(CC.heights(xyz, a["planes"][a["best_candidate"]]))
    assert set(np.unique(h)) == {0.0, CASES["threshold_exact"]["fp"]["distance_threshold"]}
    assert a["n_inliers"] - b["n_inliers"] == layer and b["n_inliers"] == 144


@pytest.mark.parametrize("name,N", [("too_few_0", 0), ("too_few_1", 1), ("too_few_2", 2), ("too_few_3", 3), ("collinear", 30)])
def test_no_plane(models, name, N):
    m = models[name]
    assert m["n_voxels"] == N
    assert (m["counts"] == 0).all() and (m["planes"] == 0).all()
    assert (m["found"], m["best_candidate"], m["n_inliers"], m["refined"]) == (0, -1, 0, 0) and (m["plane"] == 0).all()
    assert (m["idx"] == -1).all() if N < 3 else (m["idx"] >= 0).all()


def test_three_voxels_span_a_plane(models):
    m = models["three_voxels"]
    assert m["n_voxels"] == 3 and m["found"] and m["n_inliers"] == 3 and m["n_refit"] == 3
    assert 0 < (m["counts"] > 0).sum() < len(m["counts"])  # valid candidates and invalid ones (a repeated index)


def test_min_inliers(models):
    a, e = models["min_inliers_above"], models["min_inliers_equal"]
    assert a["n_inliers"] == e["n_inliers"] == 25
    assert CASES["min_inliers_above"]["fp"]["min_inliers"] == 26 and CASES["min_inliers_equal"]["fp"]["min_inliers"] == 25
    assert (a["found"], e["found"]) == (0, 1) and a["best_candidate"] >= 0 and (a["plane"] == 0).all()


def test_camera_sides(models):
    up, down, on = models["floor_blocks_small"], models["camera_below"], models["camera_on_plane"]
    assert np.array_equal(down["plane"], -up["plane"]) and up["s"] != 0 and down["plane"][2] < 0
    assert on["found"] and on["refined"] == 0 and on["s"] == 0.0
    assert np.array_equal(on["plane"], on["planes"][on["best_candidate"]])


def test_far_inliers(models):
    m = models["far_inliers"]
    xyz = _xyz("far_inliers")
    assert (xyz[:, 0] > 8.5).sum() == 2 and xyz[m["idx"][m["best_candidate"], 0], 0] < 1.0
    members = np.flatnonzero(PF.inliers(xyz, m["planes"][m["best_candidate"]], CASES["far_inliers"]["fp"]["distance_threshold"]))
    assert (xyz[members, 0] > 8.5).sum() == 2
    assert m["n_refit"] == m["n_inliers"] - 2 and m["refined"]


def test_parameter_edges(models):
    assert models["refine_off"]["refined"] == 0 and models["refine_off"]["found"]
    assert np.array_equal(np.abs(models["refine_off"]["plane"]), np.abs(models["refine_off"]["planes"][models["refine_off"]["best_candidate"]]))
    assert len(models["one_candidate"]["counts"]) == 1 and models["one_candidate"]["found"]
    assert len(models["max_candidates"]["counts"]) == 256
    assert np.array_equal(models["max_candidates"]["idx"][:128], models["floor_blocks_small"]["idx"])
    assert CASES["seed_zero"]["fp"]["seed"] == 0 and CASES["seed_max"]["fp"]["seed"] == 2 ** 64 - 1
    for name in ("seed_zero", "seed_max"):
        assert models[name]["found"] and not np.array_equal(models[name]["idx"], models["floor_blocks_small"]["idx"])


def test_both_cameras(models):
    c = CASES["both_cameras"]
    xyz, cams = CC.voxel_cloud(c)
    m = models["both_cameras"]
    floor = xyz[:, 2] == xyz[:, 2].min()
    assert (cams[floor] == 0).sum() >= 72 and (cams[floor] == 1).sum() >= 72
    assert m["found"] and m["n_inliers"] == int(floor.sum())


def test_no_sum_can_overflow(models):
    """the bound of rule 5, and the sums of the widest case, in Python integers"""
    assert (2 ** 19) ** 2 * 2 ** 24 < 2 ** 63 and 8 * 65536 == 2 ** 19
    m, xyz = models["far_inliers"], _xyz("far_inliers")
    members = np.flatnonzero(PF.inliers(xyz, m["planes"][m["best_candidate"]], CASES["far_inliers"]["fp"]["distance_threshold"]))
    n, S, qmax = PF.refit_sums(xyz, members, xyz[m["idx"][m["best_candidate"], 0]])
    assert n == m["n_refit"] and qmax < 2 ** 19 and all(abs(s) < 2 ** 62 for s in S)


@pytest.fixture(scope="module")
def scene():
    pts, size_left, ws, origins, cp, centre = PF.rotated_scene()
    cams = M.camera_ids(pts, size_left, True)
    xyz, _ = D.voxel_model(pts, cams, ws, 0.003)
    return dict(xyz=xyz, origins=origins, cp=cp, centre=centre, truth=CC.cluster_model(xyz, cp))


@pytest.mark.parametrize("threshold", [0.004, 0.01])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_rotated_scene(scene, threshold, seed):
    xyz, cp = scene["xyz"], scene["cp"]
    assert len(xyz) == 26399  # (x first, then y, in double, rounded to float32 once)
    m = PF.fit_model(xyz, dict(distance_threshold=threshold, seed=seed), scene["origins"][0])
    assert m["found"] and m["refined"]
    n_true, d_true = np.array(cp["plane"][:3]), cp["plane"][3]
    angle = np.degrees(np.arccos(min(1.0, float(m["plane"][:3] @ n_true))))
    offset = abs(float(m["plane"][:3] @ scene["centre"] + m["plane"][3]))
    print("threshold", threshold, "seed", seed, "angle", angle, "deg, offset at the centre", offset * 1e3, "mm, inliers", m["n_inliers"])
    assert abs(float(n_true @ scene["centre"] + d_true)) < 1e-9
    assert angle < 0.25 and offset < 0.0015
    assert float(m["plane"][:3] @ scene["origins"][0] + m["plane"][3]) > 0
    got = CC.cluster_model(xyz, dict(cp, plane=tuple(m["plane"])))
    want = scene["truth"]
    assert got["n_objects"] == want["n_objects"] == 3
    assert np.all(np.abs(got["sizes"][:3] - want["sizes"][:3]) <= 0.1 * want["sizes"][:3])
