"""The cases of tests/taubin_surface_cases.py are in the regime they name, and the oracle is right there: from O.find_hands and
O.fit_frames alone (numpy, no GPU).

Per case: every sample has a finite frame; its neighbour count lies in the capacity class the case is named after; the number of
columns of quadric.cpp:283-284 that the kernels' filter (1e-9 n + 1e-7 max) cannot tell from the best one, counted here in float64
numpy from the frame's own quadric, is what the case is for (every column but at most one on a plane, dozens on the cylinder and
the ridge, one on the sphere cap and the saddle); the frame's normal is the lattice normal of every plane and its axis the axis
of the cylinder.

One case yields non-finite gradient normals: `many-x` (taubin_surface_cases.NONFINITE_CASES), where fifteen of the 5184 samples
have a neighbour at which their quadric's gradient is exactly zero.  Their frames are NaN with valid = 1, and
test_many_samples_on_a_singular_pencil asserts that these are exactly the samples whose gradient normals, computed here, are not
finite.  There the column estimates of k_taubin_frame are NaN as well, so its filter has nothing to go by.  `sparse-110` has
the same in neighbourhoods of three points (test_zero_gradients_in_neighbourhoods_of_three).  Every other case, sample and point
has finite normals and a finite frame, asserted per sample.
"""
import numpy as np
import pytest

from tests import taubin_surface_cases as ts

SAMPLE_PASS_CASES = ts.DET_CASES + ts.HUGE_CASES + ts.FAR_CASES + (ts.CLUSTER_CASE,)


def _finite(fr):
    return bool(ts.finite_rows(fr).all())


def _in_class(n_nb, classes, ranges=ts.CLASS_RANGE):
    return all(ranges[c][0] <= n <= ranges[c][1] for n, c in zip(n_nb, classes))


def _cos_to(v, direction):
    d = np.asarray(direction, np.float64)
    return np.abs(np.asarray(v) @ (d / np.linalg.norm(d)))


def _angle_to(v, direction):
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    return np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(np.asarray(v), d), axis=-1)))


def test_cases_are_exact_in_float32_and_cached():
    for name in ts.ALL_CASES:
        c = ts.case(name)
        assert c is ts.case(name)
        assert c.xyz.dtype == np.float32 and len(c.cam) == len(c.xyz) and len(c.classes) == len(c.samples)
        assert 0 < c.cam.sum() < len(c.cam) and np.array_equal(np.flatnonzero(c.cam), np.arange(0, len(c.cam), 3))
        q = c.xyz.astype(np.float64) * 2.0 ** 20
        assert np.array_equal(q, np.round(q))  # on the 2^-20 m lattice
        if c.normal is not None:
            assert np.ptp(c.xyz.astype(np.float64) @ np.asarray(c.normal, np.float64)) == 0.0  # a plane to the last bit


@pytest.mark.parametrize("name", SAMPLE_PASS_CASES)
def test_every_sample_has_a_finite_frame_in_its_class(name):
    c, fr = ts.case(name), ts.reference(name)["frames"]
    assert (fr["valid"] == 1).all() and _finite(fr)
    assert _in_class(fr["n_nb"], c.classes), fr["n_nb"]
    if name == ts.CLUSTER_CASE:
        assert fr["n_nb"].tolist() == list(ts.CLUSTER_SIZES)
        assert set(range(3, 9)) <= set(ts.CLUSTER_SIZES)
    if name == "plane-4096-z":  # one launch holds samples the 4096 class's list walk takes and one it does not
        assert c.classes == ("4096",) * 3 + ("1152",)
    for k, s in enumerate(c.samples):
        nrm = ts.gradient_normals(c.xyz, c.xyz[s], fr["params"][k])
        assert len(nrm) == fr["n_nb"][k] and np.isfinite(nrm).all()
        if c.normal is None and c.ties is None:
            continue
        tied = ts.tied_columns(nrm)
        if c.normal is not None:
            assert tied >= len(nrm) - 1, (k, tied)
        else:
            least, most = c.ties
            assert tied >= least and (most is None or tied <= most), (k, tied)


@pytest.mark.parametrize("name", [n for n in SAMPLE_PASS_CASES if ts.case(n).normal is not None])
def test_plane_frames_have_the_lattice_normal(name):
    c, fr = ts.case(name), ts.reference(name)["frames"]
    assert (_cos_to(fr["normal"], c.normal) > 1 - 1e-9).all()
    if c.normal == (0, 0, 1):
        assert (fr["max_index"] == 0).all()  # every column sum is the same number: the first column wins


def test_rounding_level_ties_decide_on_planes_off_the_z_axis():
    """On a plane whose normal is not z the column sums differ in their last bits, and the first maximum is not column 0: only a
    sum in the oracle's exact order of additions picks the same column."""
    x_planes = [n for n in ts.PLANE_CASES + ts.HUGE_CASES if n.endswith("-x")]
    assert len(x_planes) == 4
    for name in x_planes:
        assert (ts.reference(name)["frames"]["max_index"] != 0).any(), name
    assert ts.reference("plane-huge-x")["frames"]["max_index"].max() > 64  # (beyond the first wave's columns)
    for name in ("plane-4096-110", "plane-4096-10m1", "plane-4096-111"):
        assert (ts.reference(name)["frames"]["max_index"] > 0).all(), name


def test_cylinder_frame_has_the_cylinders_axis():
    c, fr = ts.case("cylinder"), ts.reference("cylinder")["frames"]
    assert (_angle_to(fr["axis"], c.axis) < 1e-6).all()  # (a wrong axis is O(1) away)
    # 7 m from the origin the un-centred fit resolves the patch's curvature (|c| / r)^4 = (7 / 0.03)^4 = 3e9 times worse than
    # the n eps = 3e-13 its sums start with: 1e-3 rad; ten times that is still far from a wrong axis
    far = ts.reference("far-cylinder")["frames"]
    assert (_angle_to(far["axis"], c.axis) < 1e-2).all()


@pytest.mark.parametrize("name", ts.RAND50_CASES)
def test_rand50_references_draw_from_every_neighbourhood(name):
    from oracle import oracle_py as O

    for seed in ts.RAND50_SEEDS:
        fr = ts.reference(name, mode=O.NORMALS_RAND50, seed=seed)["frames"]
        assert (fr["valid"] == 1).all() and _finite(fr) and (fr["n_nb"] > 50).all()
        assert np.array_equal(fr["n_nb"], ts.reference(name)["frames"]["n_nb"])
        assert (_cos_to(fr["normal"], ts.case(name).normal) > 1 - 1e-9).all()


@pytest.mark.parametrize("name", ts.MANY_CASES)
def test_many_samples_on_a_singular_pencil(name):
    """5184 samples, every one on an exact plane; the frames of the first 4096 do not depend on how many follow them (samples
    are independent: this proves the two lists, not the oracle)."""
    from oracle import oracle_py as O

    c, ref = ts.case(name), ts.reference(name)
    fr = ref["frames"]
    assert len(c.samples) == ts.MANY_SIDE ** 2 > 4096 >= ts.MANY_FIRST
    assert (fr["valid"] == 1).all() and _in_class(fr["n_nb"], c.classes)
    assert 150 < np.median(fr["n_nb"]) < 256
    ok = ts.finite_rows(fr)
    zero_gradient = np.array([not np.isfinite(ts.gradient_normals(c.xyz, c.xyz[s], fr["params"][k])).all()
                              for k, s in enumerate(c.samples)])
    assert np.array_equal(~ok, zero_gradient)
    if name in ts.NONFINITE_CASES:
        bad = np.flatnonzero(~ok)
        assert 0 < len(bad) < 32 and bad.max() < ts.MANY_FIRST  # (both sample counts of the GPU test meet them)
        assert np.isfinite(fr["params"][bad]).all() and np.isnan(fr["normal"][bad]).all() and np.isnan(fr["axis"][bad]).all()
        assert not np.isin(ref["hyps"]["sample"], bad).any()
    else:
        assert ok.all()
    assert (_cos_to(fr["normal"][ok], c.normal) > 1 - 1e-9).all()
    first = O.find_hands(ts.params(), c.xyz, c.cam, c.samples[:ts.MANY_FIRST])
    assert first["frames"].tobytes() == fr[:ts.MANY_FIRST].tobytes()
    h = ref["hyps"]
    assert first["hyps"].tobytes() == h[h["sample"] < ts.MANY_FIRST].tobytes()


def test_zero_gradients_in_neighbourhoods_of_three():
    """The sparse (1,1,0) plane under a Taubin radius of 0.01: no neighbourhood holds more than a handful of points, and the
    samples with a NaN frame are those with a neighbour at which their quadric's gradient is exactly zero, three collinear
    points each."""
    c, ref = ts.case(ts.SPARSE_CASE), ts.sparse_reference()
    fr = ref["frames"]
    assert (fr["valid"] == 1).all() and 1 <= fr["n_nb"].min() and fr["n_nb"].max() < 16
    ok = ts.finite_rows(fr)
    zero_gradient = np.array([not np.isfinite(ts.gradient_normals(c.xyz, c.xyz[s], fr["params"][k], ts.SPARSE_RADIUS)).all()
                              for k, s in enumerate(c.samples)])
    assert np.array_equal(~ok, zero_gradient) and 8 <= (~ok).sum() < 64
    assert (fr["n_nb"][~ok] == 3).all() and (fr["max_index"][~ok] == 0).all()
    assert not np.isin(ref["hyps"]["sample"], np.flatnonzero(~ok)).any()
    # the all-points pass runs at the same radius here: every point's frame is its sample frame
    assert ts.params().nn_radius_normals == ts.SPARSE_RADIUS
    assert ts.all_points_frames(ts.SPARSE_CASE).tobytes() == fr.tobytes()


@pytest.mark.parametrize("name", ts.ALLPOINTS_CASES)
def test_all_points_pass_cases(name):
    """The r = 0.01 ball of the points away from the lattice's edge lies in the frame class of the all-points pass the case is
    named after, no ball is larger, and the points of the cloud get the plane's normal."""
    c = ts.case(name)
    cls = name.split("-")[1]
    fr = ts.all_points_frames(name)
    lo, hi = ts.ALLPOINTS_RANGE[cls]
    assert (fr["valid"] == 1).all() and _finite(fr)
    assert fr["n_nb"].max() <= hi and lo <= np.median(fr["n_nb"]) and (fr["n_nb"][c.samples] >= lo).all()
    # The chosen column decides the normal, and with every column tied it may be one next to the zero line of the fit's second
    # linear factor, where the gradient is rounding noise over almost nothing (a handful of points of the x planes, up to
    # 1.6e-2 rad): the thresholds of test_exactly_planar_lattice_patch_yields_the_planes_normal for such points.
    cos = _cos_to(fr["normal"], c.normal)
    assert np.median(cos) > 1 - 1e-9 and (cos > 1 - 1e-6).mean() > 0.95
    ref = ts.reference(name, antipodal=True)["frames"]
    assert (ref["valid"] == 1).all() and _finite(ref) and _in_class(ref["n_nb"], c.classes)
    assert (_cos_to(ref["normal"], c.normal) > 1 - 1e-9).all()


def test_scaled_scene_keeps_every_neighbourhood():
    """A power of two as the unit changes no float's mantissa: the scaled scene's balls hold the points they held."""
    from agile_grasp_amd import synthetic
    from oracle import oracle_py as O

    sc = synthetic.config("tiny")
    xyz, cam, cams, s = ts.scaled_scene()
    assert np.array_equal(xyz.astype(np.float64), sc.xyz.astype(np.float64) * ts.UNIT) and np.array_equal(cams, sc.cam_origins * 8.0)
    assert set(ts.scaled_lengths()) == set(ts.LENGTHS) and ts.scaled_lengths()["nn_radius_hands"] == 0.64
    ref = ts.scaled_reference()
    base = O.find_hands(O.default_params(sc.cam_origins, num_threads=16), sc.xyz, sc.cam, sc.samples)
    assert (ref["frames"]["valid"] == 1).all() and _finite(ref["frames"]) and len(ref["hyps"]) > 10
    assert np.array_equal(ref["frames"]["n_nb"], base["frames"]["n_nb"]) and np.array_equal(ref["nh"], base["nh"])
    # the frames agree with the metre-scale ones as far as the un-centred fit's conditioning lets them
    # (tests/test_taubin_solver.py::test_solver_is_scale_covariant: 1e-3)
    assert (np.abs((ref["frames"]["normal"] * base["frames"]["normal"]).sum(1)) > 1 - 1e-6).mean() > 0.9
