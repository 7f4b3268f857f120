"""The Taubin frame stage on exact, tied and singular surfaces, against the oracle with exact equality: no tolerance anywhere.

tests/taubin_surface_cases.py builds the clouds and tests/test_taubin_surface_cases.py proves on the CPU what each is for: planes
on which every column of quadric.cpp:283-284 is a candidate of k_taubin_frame's filter and the last bits of the exact sums pick
the winner, surfaces with dozens of tied columns, singular pencils in every lattice orientation, more than 4096 samples of
them, the all-points pass, neighbourhoods of 3 .. 8 points, coordinates 7 m out and in another unit.  Each test here also proves
from the context that it reached its path: the neighbour counts are the oracle's and lie in the capacity class, or S does.
"""
import numpy as np
import pytest

from tests import capacity_clouds as cc
from tests import taubin_surface_cases as ts
from tests.test_gpu_parity import assert_frames_equal, assert_hyps_equal

pytestmark = pytest.mark.gpu

FRAME_FIELDS = ("valid", "n_nb", "majority_cam", "max_index", "sample", "params", "eigenvalue", "normal", "axis", "binormal")


def _ctx(**kw):
    from agile_grasp_amd import binding

    return binding.Context(cc.cams(), **kw)


def _assert_reached(ctx, ref, classes, ranges=ts.CLASS_RANGE):
    """The context's neighbour counts are the oracle's, and each lies in the class the case is named after."""
    nt, nh = ctx.neighbor_counts()
    assert np.array_equal(nt, ref["frames"]["n_nb"]) and np.array_equal(nh, ref["nh"])
    for n, c in zip(nt, classes):
        assert ranges[c][0] <= n <= ranges[c][1], (n, c)


def _assert_result(ctx, hyps, ref):
    assert_frames_equal(ctx.frames(), ref["frames"])
    assert_hyps_equal(hyps, ref["hyps"])


@pytest.mark.parametrize("name", ts.DET_CASES)
def test_planes_and_symmetric_surfaces_det(name):
    """Exact discs in the 1152, 4096 and 6144 classes (normal z: all sums equal, the first column wins; normal x, (1,1,0),
    (1,0,-1), (1,1,1): the sums differ in their last bits and other pivots deflate), the cylinder, the ridge, and the sphere cap
    and the saddle as controls.  Twice on one context: the first call switches the larger classes on, the second starts with
    them on."""
    c, ref = ts.case(name), ts.reference(name)
    ctx = _ctx()
    ctx.set_cloud(c.xyz, c.cam)
    for _ in range(2):
        hyps = ctx.find_hands(c.samples)
        _assert_reached(ctx, ref, c.classes)
        _assert_result(ctx, hyps, ref)


@pytest.mark.parametrize("name", ts.HUGE_CASES)
def test_planes_beyond_the_lds_classes_det(name):
    """11 873 tied columns in k_taubin_frame_huge (four columns per wave, first maximum kept); then the context, its scratch
    re-sized, on an ordinary scene."""
    from agile_grasp_amd import synthetic
    from oracle import oracle_py as O

    c, ref = ts.case(name), ts.reference(name)
    ctx = _ctx()
    ctx.set_cloud(c.xyz, c.cam)
    for _ in range(2):
        hyps = ctx.find_hands(c.samples)
        _assert_reached(ctx, ref, c.classes)
        _assert_result(ctx, hyps, ref)
    sc = synthetic.config("tiny")
    ctx.set_cloud(sc.xyz, sc.cam)
    hyps = ctx.find_hands(sc.samples)
    ref2 = O.find_hands(ts.params(), sc.xyz, sc.cam, sc.samples)
    assert len(hyps) > 10
    _assert_result(ctx, hyps, ref2)


@pytest.mark.parametrize("seed", ts.RAND50_SEEDS)
@pytest.mark.parametrize("name", ts.RAND50_CASES)
def test_planes_rand50(name, seed):
    """The production mode on exact planes: 50 tied columns, one per lane (the bit-reversed leaf walk and the shuffle argmax)."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    c, ref = ts.case(name), ts.reference(name, mode=O.NORMALS_RAND50, seed=seed)
    ctx = _ctx(normals_mode=binding.NORMALS_RAND50, rand_seed=seed)
    ctx.set_cloud(c.xyz, c.cam)
    for _ in range(2):
        hyps = ctx.find_hands(c.samples)
        _assert_reached(ctx, ref, c.classes)
        assert (ctx.neighbor_counts()[0] > 50).all()  # every sample draws
        _assert_result(ctx, hyps, ref)


def _assert_frames_equal_where_finite(got, ref):
    """assert_frames_equal on the frames whose entries are finite; the others (taubin_surface_cases.NONFINITE_CASES) hold NaN
    where the oracle's do and are equal everywhere else."""
    ok = ts.finite_rows(ref)
    assert_frames_equal(got[ok], ref[ok])
    for f in FRAME_FIELDS:
        assert np.array_equal(got[f][~ok], ref[f][~ok], equal_nan=True), f


@pytest.mark.parametrize("name", ts.MANY_CASES)
def test_more_than_4096_samples_on_a_singular_pencil(name):
    """5184 samples on an exact plane, then the first 4096 of them: k_taubin_eigen's serial bisection (one lane per sample
    beyond 4096 samples) and its eight-lane tree replay on the same deflated pencils."""
    c, ref = ts.case(name), ts.reference(name)
    first = ts.MANY_FIRST
    ok = ts.finite_rows(ref["frames"])
    assert ok.all() == (name not in ts.NONFINITE_CASES)
    ctx = _ctx()
    ctx.set_cloud(c.xyz, c.cam)
    hyps = ctx.find_hands(c.samples)
    assert ctx.last_samples == len(c.samples) > 4096
    _assert_reached(ctx, ref, c.classes)
    all_frames = ctx.frames()
    _assert_frames_equal_where_finite(all_frames, ref["frames"])
    assert len(hyps) > 1000
    assert_hyps_equal(hyps, ref["hyps"])
    hyps = ctx.find_hands(c.samples[:first])
    assert ctx.last_samples == first <= 4096
    assert np.array_equal(ctx.neighbor_counts()[0], ref["frames"]["n_nb"][:first])
    first_frames = ctx.frames()
    _assert_frames_equal_where_finite(first_frames, ref["frames"][:first])
    assert_hyps_equal(hyps, ref["hyps"][ref["hyps"]["sample"] < first])
    for f in FRAME_FIELDS:
        assert np.array_equal(first_frames[f], all_frames[f][:first], equal_nan=True), f


def test_zero_gradients_in_neighbourhoods_of_three():
    """NaN column sums where the columns are summed one at a time (fewer than 16 of them in the 1152 class: the sample pass
    under a Taubin radius of 0.01) and a column per lane (the all-points pass): column 0 stays, as in the oracle."""
    c, ref = ts.case(ts.SPARSE_CASE), ts.sparse_reference()
    bad = ~ts.finite_rows(ref["frames"])
    assert bad.sum() >= 8
    ctx = _ctx(nn_radius_taubin=ts.SPARSE_RADIUS)
    ctx.set_cloud(c.xyz, c.cam)
    for _ in range(2):
        hyps = ctx.find_hands(c.samples, calculates_antipodal=True)
        _assert_reached(ctx, ref, c.classes)
        assert ctx.neighbor_counts()[0].max() < 16
        _assert_frames_equal_where_finite(ctx.frames(), ref["frames"])
        assert_hyps_equal(hyps, ref["hyps"])
        got = ctx.normals()  # (every point is a sample and both passes use r = 0.01: the sample frames' normals)
        assert np.array_equal(got, ref["frames"]["normal"], equal_nan=True)
        assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()


@pytest.mark.parametrize("name", ts.ALLPOINTS_CASES)
def test_all_points_pass_on_exact_planes(name):
    """calculates_antipodal on plane lattices whose r = 0.01 balls hold about 20 points (a column per lane), 89 (more than 64
    normals in the 128 class) and 333 (the 1152 class): every point's normal and the labels against the oracle."""
    c = ts.case(name)
    ref = ts.reference(name, antipodal=True)
    fr = ts.all_points_frames(name)
    lo, hi = ts.ALLPOINTS_RANGE[name.split("-")[1]]
    assert fr["n_nb"].max() <= hi and (fr["n_nb"][c.samples] >= lo).all()
    ctx = _ctx()
    ctx.set_cloud(c.xyz, c.cam)
    for _ in range(2):
        hyps = ctx.find_hands(c.samples, calculates_antipodal=True)
        _assert_reached(ctx, ref, c.classes)
        _assert_result(ctx, hyps, ref)
        exp = np.where(fr["valid"][:, None] != 0, fr["normal"], 0.0)
        exp[c.samples] = np.where(ref["frames"]["valid"][:, None] != 0, ref["frames"]["normal"], exp[c.samples])  # (hand_search.cpp:102)
        got = ctx.normals()
        assert np.array_equal(got, exp)
        assert (np.abs(got).sum(1) > 0).all()


def test_underdetermined_neighbourhoods():
    """Clusters of 3 .. 8 points, four coplanar points, three collinear points and a cluster with an exact duplicate: rank
    deficient in more than one coordinate."""
    c, ref = ts.case(ts.CLUSTER_CASE), ts.reference(ts.CLUSTER_CASE)
    ctx = _ctx()
    ctx.set_cloud(c.xyz, c.cam)
    for _ in range(2):
        hyps = ctx.find_hands(c.samples)
        assert ctx.neighbor_counts()[0].tolist() == list(ts.CLUSTER_SIZES)
        _assert_reached(ctx, ref, c.classes)
        _assert_result(ctx, hyps, ref)
    assert len(hyps) > 0


@pytest.mark.parametrize("name", ts.FAR_CASES)
def test_surfaces_far_from_the_origin(name):
    """The 1152-class z disc and the cylinder at (6, -3, 2) m: the un-centred fit at its worst conditioning."""
    c, ref = ts.case(name), ts.reference(name)
    ctx = _ctx()
    ctx.set_cloud(c.xyz, c.cam)
    for _ in range(2):
        hyps = ctx.find_hands(c.samples)
        _assert_reached(ctx, ref, c.classes)
        _assert_result(ctx, hyps, ref)
    assert len(hyps) > 0


def test_scene_in_another_unit():
    """The tilted `tiny` scene with every coordinate, both camera origins, both radii and the hand geometry times 8 (the hand's
    depth as far as the context takes it: taubin_surface_cases.scaled_lengths)."""
    from agile_grasp_amd import binding

    xyz, cam, cams, s = ts.scaled_scene()
    ref = ts.scaled_reference()
    ctx = binding.Context(cams, **ts.scaled_lengths())
    ctx.set_cloud(xyz, cam)
    hyps = ctx.find_hands(s)
    nt, nh = ctx.neighbor_counts()
    assert np.array_equal(nt, ref["frames"]["n_nb"]) and np.array_equal(nh, ref["nh"]) and nt.max() <= 1152
    assert len(hyps) > 10
    _assert_result(ctx, hyps, ref)
