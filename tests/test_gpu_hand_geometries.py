"""k_hand_sweep, k_learning_points and the stages behind them off the default hand geometry, against the oracle bit for bit.

The geometries and clouds are those of tests/hand_geometries.py (tests/test_hand_geometries.py pins on the CPU what each one
exercises): one, two, three and four thresholds per look-up cell, bite-depth tables of 1, 2, 7, 11 and 16 entries that the
hands walk to the end, in the plain search, the antipodal pass and the training-image mode.  Every instantiation of
k_hand_sweep<MODE, PX, PY, NT, WG4> runs here:
  <0, 2, 1, 256, 0>  plain, the `few` geometries (default, one_per_cell, one_depth, two_depths, sixteen_depths)
  <0, 4, 4, 256, 0>  plain, three_a / three_b / four; three_a at 4100 samples too, where it must not become ...
  <0, 2, 1, 256, 1>  ... the four-per-CU form of the default hand (tests/test_gpu_capacity_edges.py runs that one)
  <1, 2, 1, 256, 0>  antipodal, the `few` geometries
  <1, 4, 4, 256, 0>  antipodal, three_a / three_b / four
  <2, 4, 4, 256, 0>  training images, every geometry
On the `sheets` cloud three_a's hands hang on the third compare of a look-up cell: a sweep that compares twice per cell
returns other hands there (and the oracle's everywhere else), in all three modes and in the 4100-sample call.
"""
import os

import numpy as np
import pytest

from tests import hand_geometries as hg
from tests.test_gpu_parity import assert_frames_equal, assert_hyps_equal

pytestmark = pytest.mark.gpu

MODES = ("plain", "antipodal", "training")


def _ctx(name, **kw):
    from agile_grasp_amd import binding

    return binding.Context(hg.cam_origins(), **hg.geom(name), **kw)


def _oracle_params(name):
    from oracle import oracle_py as O

    return O.default_params(hg.cam_origins(), num_threads=min(os.cpu_count() or 1, 16), **hg.geom(name))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", hg.ACCEPTED)
def test_every_geometry_in_every_mode(name, mode):
    """Frames, hypotheses and images of each accepted geometry on its clouds; in training mode the three instance images of
    every hypothesis and their descriptors too."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    ctx = _ctx(name)
    if mode == "training":
        ctx.set_training_images(True)
    for cl in hg.CLOUDS[name]:
        xyz, cam, s = hg.cloud(cl)
        ref = hg.reference(name, cl, mode)
        ctx.set_cloud(xyz, cam)
        hyps = ctx.find_hands(s, calculates_antipodal=mode != "plain")
        assert_frames_equal(ctx.frames(), ref["frames"])
        print(name, mode, cl, len(hyps), "of", len(ref["hyps"]))
        assert_hyps_equal(hyps, ref["hyps"])
        if name in hg.EMPTY:
            assert len(hyps) == 0
            continue
        assert len(hyps) >= 20
        if mode == "training":
            packed = ctx.training_images()
            assert np.array_equal(binding.unpack_images(packed.reshape(-1, 250)).reshape(-1, 3, 8000), ref["images"]), cl
            assert np.array_equal(ctx.hog_images(packed.reshape(-1, 250)), O.hog_many(ref["images"].reshape(-1, 8000))), cl
        else:
            assert np.array_equal(ctx.images(), ref["images"]), cl


@pytest.mark.parametrize("name", ["three_a", "one_per_cell", "sixteen_depths"])
def test_learning_points(name):
    """k_learning_points reads the geometry's finger slots, the last bite's box, the hand angles and the hand height: every
    hypothesis' points and camera ids on the rod, whose hands reach the last depth."""
    from oracle import oracle_py as O

    xyz, cam, s = hg.cloud("rod")
    ref = O.find_hands_points(_oracle_params(name), xyz, cam, s)
    ctx = _ctx(name)
    ctx.set_cloud(xyz, cam)
    hyps = ctx.find_hands(s)
    assert_hyps_equal(hyps, ref["hyps"])
    assert len(hyps) >= 20 and hyps["depth_index"].max() == hg.derive(hg.geom(name))["n_depths"] - 1
    for k in range(len(hyps)):
        pts, pcam = ctx.learning_points(k)
        assert pts.shape == (3, hyps["n_in_box"][k]), k
        assert np.array_equal(pts, ref["points"][k]) and np.array_equal(pcam, ref["cams"][k]), k


def test_refused_geometries():
    """More than 15 deepening steps, and five thresholds in one look-up cell: agh_create refuses each with its reason, and a
    context created afterwards works."""
    from agile_grasp_amd import binding

    for name, word in (("refused_depths", "deepening steps"), ("refused_cell", "look-up cell")):
        assert hg.derive(hg.geom(name))["refused"] is not None
        with pytest.raises(binding.AghError) as e:
            _ctx(name)
        assert e.value.code == -1 and word in str(e.value), str(e.value)  # AGH_ERR_INVALID_ARGUMENT
    xyz, cam, s = hg.cloud("tiny")
    ctx = _ctx("default")
    ctx.set_cloud(xyz, cam)
    assert_hyps_equal(ctx.find_hands(s), hg.reference("default", "tiny", "plain")["hyps"])


# ---- beyond find_hands ----------------------------------------------------------------------------------------------
N_SAMPLES = 400
SEED = 7
CHAIN = dict(n_samples=N_SAMPLES, sample_seed=SEED, classify=True, min_inliers=2, filters_boundaries=True)


@pytest.fixture(scope="module")
def raw():
    from agile_grasp_amd import synthetic

    return synthetic.make_raw_cloud(40_000, seed=5)


def _chain_ctx(raw, svm_model):
    from agile_grasp_amd import binding

    ctx = binding.Context(raw.cam_origins, **hg.geom("three_a"))
    ctx.load_svm(*svm_model)
    return ctx


@pytest.fixture(scope="module")
def one_call(raw, svm_model):
    return _chain_ctx(raw, svm_model).localize(raw.xyz, raw.size_left, raw.workspace, **CHAIN)


def _same_result(got, want):
    from tests.test_gpu_boundary_chain import FIELDS, HANDLE_FIELDS

    assert np.array_equal(got["samples"], want["samples"]) and np.array_equal(got["inlier_idx"], want["inlier_idx"])
    assert (got["n_voxels"], got["n_hypotheses"]) == (want["n_voxels"], want["n_hypotheses"])
    assert len(got["hands"]) == len(want["hands"]) and len(got["handles"]) == len(want["handles"])
    for f in FIELDS:
        assert np.array_equal(got["hands"][f], want["hands"][f]), f
    for f in HANDLE_FIELDS:
        assert np.array_equal(got["handles"][f], want["handles"][f]), f


def test_localize_with_a_general_probe_hand_equals_its_stages(raw, svm_model, one_call):
    """agh_localize with three_a: the classifier, the boundary filter and the handle search on the hypotheses of
    <0, kLutProbe, kLutProbe>, against preprocess, find_hands on the chain's samples, classify, the filter restated in numpy
    and find_handles on a second context -- and the search itself against the oracle."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O
    from tests.test_gpu_boundary_chain import _assert_same, _near

    got = one_call
    ctx = _chain_ctx(raw, svm_model)
    n_vox = ctx.preprocess(raw.xyz, raw.size_left, raw.workspace)
    assert got["n_voxels"] == n_vox and np.array_equal(got["samples"], binding.draw_samples(n_vox, N_SAMPLES, SEED))
    hyps = ctx.find_hands(got["samples"])
    vox, vcam = ctx.cloud()
    p = O.default_params(raw.cam_origins, num_threads=min(os.cpu_count() or 1, 16), **hg.geom("three_a"))
    assert_hyps_equal(hyps, O.find_hands(p, vox, vcam, got["samples"])["hyps"])
    keep = ctx.classify().astype(bool)
    near = _near(hyps, raw.workspace)
    hyps["svm_keep"] = keep
    h = hyps[keep & ~near]
    hd, idx = ctx.find_handles(h, 2, 0.005)
    print("hypotheses", len(hyps), "kept", int(keep.sum()), "near a face", int(near.sum()), "hands", len(h), "handles", len(hd))
    assert got["n_hypotheses"] == len(hyps) and len(h) > 0 and len(hd) > 0
    assert 0 < keep.sum() < len(keep) and (keep & near).any() and (keep & ~near).any()  # both filters bite
    _assert_same(got, h, hd, idx)
    assert np.all(got["hands"]["svm_keep"] == 1)


def test_localize_batch_with_a_general_probe_hand(raw, svm_model, one_call):
    """The same capture twice through agh_localize_batch: each equals the single call."""
    ctx = _chain_ctx(raw, svm_model)
    kw = {k: v for k, v in CHAIN.items() if k != "sample_seed"}
    res = ctx.localize_batch([raw.xyz, raw.xyz], [raw.size_left] * 2, raw.workspace, sample_seeds=[SEED, SEED], **kw)
    assert len(res) == 2 and len(one_call["hands"]) > 0
    for r in res:
        _same_result(r, one_call)


@pytest.mark.parametrize("cl", ["tiny", "sheets"])
def test_sharded_search_with_a_general_probe_hand(cl):
    """Two in-process ranks with three_a: every rank holds the single-context list, which is the oracle's."""
    from agile_grasp_amd import binding
    from tests.test_gpu_sharding import _run_ranks, _same

    xyz, cam, s = hg.cloud(cl)
    ref = hg.reference("three_a", cl, "antipodal")["hyps"]
    one = _ctx("three_a")
    one.set_cloud(xyz, cam)
    single = one.find_hands(s, calculates_antipodal=True)
    assert_hyps_equal(single, ref)
    ctxs = [_ctx("three_a") for _ in range(2)]
    for c in ctxs:
        c.set_cloud(xyz, cam)
    binding.comm_init_local(ctxs)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(s, calculates_antipodal=True)):
        _same(hyps, single)
    assert len(single) >= 20 and single["half_antipodal"].any()


def test_a_general_probe_hand_stays_off_the_four_per_cu_form():
    """4100 samples with three_a: beyond kSweepWg4MinSamples the default hand takes <0, 2, 1, 256, 1>, whose two probes
    misrank the points that decide the sheets' hands (tests/test_hand_geometries.py).  tiny's samples and the sheets' give
    the oracle's hands; samples are independent, so every sample's hypotheses are also those of a 64-sample call that holds
    it."""
    from oracle import oracle_py as O

    xyz, cam, s, n_tiny, n_own = hg.padded_tiny()
    assert len(s) > 4096
    ctx = _ctx("three_a")
    ctx.set_cloud(xyz, cam)
    big = ctx.find_hands(s)
    ref = O.find_hands(_oracle_params("three_a"), xyz, cam, s[:n_own])["hyps"]
    assert_hyps_equal(big[big["sample"] < n_own], ref)
    assert ((ref["sample"] >= n_tiny) & (ref["finger_index"] == 2)).sum() >= 20
    parts = []
    for lo in range(0, len(s), 64):
        part = ctx.find_hands(s[lo:lo + 64])
        part["sample"] += lo
        parts.append(part)
    small = np.concatenate(parts)
    assert (big["sample"] >= n_own).any()  # the padding's samples find hands too
    assert_hyps_equal(big, small)
