"""agh_set_hand_filter (include/agh.h; DESIGN.md, "Hand filter"): the approach cone, the aperture and the observed-space test as
a stage of every localize chain.  Every result is held, bit for bit (epoch aside), against the stage-wise route on the samples
the call reports -- agh_find_hands -> the numpy model of tests/hand_filter_cases.py -> [filterHands] -> agh_classify's kept ->
agh_find_handles on a second context that never has a filter -- and the per-list counts against the model's.  The regimes are
those tests/test_hand_filter_cases.py proves on the CPU; a test that finds one empty fails."""
import numpy as np
import pytest

from tests import depth_captures as D
from tests import hand_filter_cases as HF
from tests.test_gpu_boundary_chain import _assert_same, _contexts, _near
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)


@pytest.fixture(scope="module")
def pair(svm_model):
    """(the context under test, the reference context of the stage-wise route), the two-view scene's camera origins"""
    one, ref = _contexts(HF.box_scene(2)["origins"], svm_model)
    yield one, ref
    one.close()
    ref.close()


@pytest.fixture
def ctxs(pair):
    pair[0].clear_hand_filter()
    yield pair
    pair[0].clear_hand_filter()


def _set(ctx, fp):
    ctx.set_hand_filter(**fp)


def _route(ref, images, ws, fp, samples, classify=True, boundaries=False, min_inliers=2, points=None, size_left=None):
    """the hands, handles and inlier lists the chain must return for `samples`, and the model's reason per hypothesis"""
    pts = D.deproject_ref(images) if points is None else points
    ref.preprocess(pts, images[0]["data"].size if size_left is None else size_left, ws, dense=True)
    vox, _ = ref.cloud()
    samples = np.asarray(samples, np.int32)
    hyps = ref.find_hands(samples).copy()
    keep = ref.classify().astype(bool) if classify and len(hyps) else np.ones(len(hyps), bool)
    reason = HF.drop_reasons(hyps, vox[samples[hyps["sample"]]], fp, images)
    ok = reason == 0
    if boundaries:
        ok &= ~_near(hyps, ws)
    if classify:
        hyps["svm_keep"] = keep
    h = hyps[keep & ok]
    hd, idx = ref.find_handles(h, min_inliers, 0.005)
    return h, hd, idx, reason, hyps


def _check(got, ref, images, ws, fp, what, **kw):
    h, hd, idx, reason, hyps = _route(ref, images, ws, fp, got["samples"], **kw)
    print(what, "hypotheses", len(hyps), "model counts", HF.counts(reason), "hands", len(h), "handles", len(hd))
    assert got["n_hypotheses"] == len(hyps), what  # the search's unfiltered count
    _assert_same(got, h, hd, idx)
    return reason, h


# ---- each criterion alone and all three together ----

@pytest.mark.parametrize("name", ["cone", "aperture", "view", "all"])
@pytest.mark.parametrize("n_views", [1, 2])
def test_depth_chain_equals_the_stagewise_route(ctxs, n_views, name):
    one, ref = ctxs
    sc = HF.box_scene(n_views)
    fp = HF.scene_filters(sc)[name]
    _set(one, fp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    reason, h = _check(got, ref, sc["images"], sc["ws"], fp, f"{n_views} views, {name}")
    c = HF.counts(reason)
    assert one.hand_filter_counts().tolist() == [c]
    if name == "all":
        assert min(c[1:4]) >= 1 and c[4] >= 5
    else:
        k = {"cone": 1, "aperture": 2, "view": 3}[name]
        assert c[k] >= 5 and c[4] >= 5 and c[0] == c[k] + c[4]
    assert len(h) >= 1


@pytest.mark.parametrize("classify", [True, False])
def test_points_chain_with_cone_and_aperture(ctxs, classify):
    one, ref = ctxs
    sc = HF.box_scene(2)
    f = HF.scene_filters(sc)
    fp = HF.params(**{k: v for k, v in f["all"].items() if k not in ("view_on",)})
    _set(one, fp)
    pts = D.deproject_ref(sc["images"])
    left = sc["images"][0]["data"].size
    got = one.localize(pts, left, sc["ws"], samples=sc["samples"], dense=True, classify=classify, min_inliers=2)
    reason, h = _check(got, ref, sc["images"], sc["ws"], fp, f"points, classify {classify}", classify=classify)
    c = HF.counts(reason)
    assert c[1] >= 5 and c[2] >= 5 and c[3] == 0 and c[4] >= 5 and one.hand_filter_counts().tolist() == [c]
    if not classify:
        assert len(h) == c[4]


def test_general_svm_model_skips_the_dropped_hands(svm_model):
    """the descriptor + kernel-row path (k_hog_svm without a model, k_svm_decide) honours the drop bytes too"""
    sc = HF.box_scene(2)
    one, ref = _contexts(sc["origins"], svm_model, general=True)
    fp = HF.scene_filters(sc)["all"]
    _set(one, fp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    reason, h = _check(got, ref, sc["images"], sc["ws"], fp, "general model")
    assert one.hand_filter_counts().tolist() == [HF.counts(reason)] and len(h) >= 1
    one.close()
    ref.close()


# ---- exact boundaries ----

def test_thresholds_exactly_on_a_hand_keep_it(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    base = HF.scene_filters(sc)["cone"]
    _, _, _, _, hyps = _route(ref, sc["images"], sc["ws"], HF.params(), sc["samples"])
    d = np.asarray(base["approach_dir"])
    a = hyps["approach"]
    dots = (a[:, 0] * d[0] + a[:, 1] * d[1]) + a[:, 2] * d[2]
    i = int(np.argsort(dots)[len(dots) // 2])
    for cos, kept in ((dots[i], True), (np.nextafter(dots[i], 2.0), False)):
        fp = dict(base, min_approach_cos=float(cos))
        _set(one, fp)
        got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], classify=False, min_inliers=2)
        reason, _ = _check(got, ref, sc["images"], sc["ws"], fp, f"cos on hand {i}, kept {kept}", classify=False)
        assert (reason[i] == 0) == kept and one.hand_filter_counts().tolist() == [HF.counts(reason)]
    w = np.sort(hyps["width"])
    lo, hi = float(w[len(w) // 4]), float(w[3 * len(w) // 4])
    assert lo < hi
    for mn, mx, n_kept in ((lo, hi, int(((hyps["width"] >= lo) & (hyps["width"] <= hi)).sum())),
                           (float(np.nextafter(lo, 1.0)), float(np.nextafter(hi, 0.0)),
                            int(((hyps["width"] > lo) & (hyps["width"] < hi)).sum()))):
        fp = HF.params(width_on=1, min_width=mn, max_width=mx)
        _set(one, fp)
        got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], classify=False, min_inliers=2)
        reason, h = _check(got, ref, sc["images"], sc["ws"], fp, f"widths {mn} .. {mx}", classify=False)
        assert len(h) == n_kept == HF.counts(reason)[4]
    assert (hyps["width"] == lo).any() and (hyps["width"] == hi).any()


# ---- probe edges: an extra view constructed for one unobserved probe of one hand ----

EDGES = {
    # name: (format, row padding, edge_view's keywords, is the probe seen in the extra view?)
    "last_pixel_f32": (D.F32, 0, {}, True),
    "last_pixel_u16_padded": (D.U16, 3, {}, True),
    "last_pixel_f32_padded": (D.F32, 1, {}, True),
    "behind_the_camera": (D.F32, 0, dict(behind=True), False),
    "invalid_f32": (D.F32, 0, dict(valid=False), False),
    "invalid_u16": (D.U16, 0, dict(valid=False), False),
    "surface_far_in_front": (D.F32, 0, dict(z_pix=0.97), False),
}


@pytest.fixture(scope="module")
def edge_probe(pair):
    """one view of the box under the tight workspace, and a hand of it with an unobserved probe outside that workspace"""
    _, ref = pair
    sc = HF.box_scene(1)
    images, ws = sc["images"], sc["ws_tight"]
    ref.preprocess(D.deproject_ref(images), images[0]["data"].size, ws, dense=True)
    vox, _ = ref.cloud()
    samples = np.sort(np.random.default_rng(3).permutation(len(vox))[:200]).astype(np.int32)
    hyps = ref.find_hands(samples).copy()
    fp = HF.params(view_on=1)
    pick = HF.pick_edge_probe(hyps, vox[samples[hyps["sample"]]], fp, images, ws)
    assert pick is not None, "no unobserved probe outside the workspace: the scene lost its regime"
    return dict(images=images, ws=ws, samples=samples, pick=pick, n_hyp=len(hyps))


@pytest.mark.parametrize("name", sorted(EDGES))
def test_probe_edges(ctxs, edge_probe, name):
    one, ref = ctxs
    fmt, pad, kw, is_seen = EDGES[name]
    i, j, w, dirn, n_unobserved = edge_probe["pick"]
    extra = HF.edge_view(w, dirn, fmt=fmt, pad=pad, **kw)
    images = [edge_probe["images"][0], extra]
    fp = HF.params(view_on=1, max_unobserved=n_unobserved - 1)  # (the hand is dropped unless the extra view sees the probe)
    assert bool(HF.seen(w, extra, fp["depth_margin"])) == is_seen
    if is_seen:  # it is the image's last pixel that shows it
        blind = dict(extra, data=np.array(extra["data"]))
        blind["data"][-1, -1] = 0
        assert not HF.seen(w, blind, fp["depth_margin"])
    _set(one, fp)
    got = one.localize_depth(images, edge_probe["ws"], samples=edge_probe["samples"], classify=False, min_inliers=2)
    reason, _ = _check(got, ref, images, edge_probe["ws"], fp, name, classify=False)
    assert got["n_hypotheses"] == edge_probe["n_hyp"]  # (the extra view added no point to the cloud)
    assert (reason[i] == 0) == is_seen and one.hand_filter_counts().tolist() == [HF.counts(reason)]


def test_probe_at_exactly_the_margin(ctxs, edge_probe):
    one, ref = ctxs
    i, j, w, dirn, n_unobserved = edge_probe["pick"]
    extra = HF.edge_view(w, dirn, fmt=D.F32)
    pose = extra["pose"]
    e = w - pose[:, 3]
    qz = (pose[0, 2] * e[0] + pose[1, 2] * e[1]) + pose[2, 2] * e[2]
    z = float(extra["data"][-1, -1])
    margin = qz - z
    assert z + margin == qz and 0.004 < margin < 0.006
    images = [edge_probe["images"][0], extra]
    below = float(np.nextafter(qz, 0.0) - z)  # the largest margin whose sum with z_pix stays below q.z
    assert z + below < qz and below < margin
    for m, is_seen in ((margin, True), (below, False)):
        fp = HF.params(view_on=1, depth_margin=m, max_unobserved=n_unobserved - 1)
        assert bool(HF.seen(w, extra, m)) == is_seen
        _set(one, fp)
        got = one.localize_depth(images, edge_probe["ws"], samples=edge_probe["samples"], classify=False, min_inliers=2)
        reason, _ = _check(got, ref, images, edge_probe["ws"], fp, f"margin {m!r}", classify=False)
        assert (reason[i] == 0) == is_seen and one.hand_filter_counts().tolist() == [HF.counts(reason)]


# ---- launch shape ----

def _samples_for_count(hyps, samples, target):
    """a sub-list of `samples` (in order) whose hypotheses number exactly `target`"""
    per = np.bincount(hyps["sample"], minlength=len(samples))
    take, total = [], 0
    for k in np.argsort(-per, kind="stable"):
        if per[k] > 0 and total + per[k] <= target:
            take.append(k)
            total += per[k]
    assert total == target, (total, target)
    return samples[np.sort(take)]


@pytest.mark.parametrize("probes", [1, 4, 16])
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 130])
def test_launch_shapes(ctxs, count, probes):
    """hypothesis counts around a wave and around the work-group's four waves (63, 65 and 130 are no multiples of four), with
    the view criterion (a wave per hypothesis) and without (a lane per hypothesis)"""
    one, ref = ctxs
    sc = HF.box_scene(2)
    _, _, _, _, hyps = _route(ref, sc["images"], sc["ws"], HF.params(), sc["samples"])
    if count == 0:
        per = np.bincount(hyps["sample"], minlength=len(sc["samples"]))
        samples = sc["samples"][per == 0][:3]
        assert len(samples) >= 1
    else:
        samples = _samples_for_count(hyps, sc["samples"], count)
    f = HF.scene_filters(sc)
    for fp in (dict(f["all"], probes_per_finger=probes, max_unobserved=9 * probes // 4), dict(f["all"], view_on=0)):
        if probes != 4 and not fp["view_on"]:
            continue
        _set(one, fp)
        got = one.localize_depth(sc["images"], sc["ws"], samples=samples, classify=False, min_inliers=2)
        reason, _ = _check(got, ref, sc["images"], sc["ws"], fp, f"{count} hypotheses, {probes} probes", classify=False)
        assert got["n_hypotheses"] == count and one.hand_filter_counts().tolist() == [HF.counts(reason)]


def test_no_samples_at_all(ctxs):
    one, _ = ctxs
    sc = HF.box_scene(1)
    _set(one, HF.scene_filters(sc)["all"])
    got = one.localize_depth(sc["images"], sc["ws"], n_samples=0, classify=False)
    assert got["n_hypotheses"] == 0 and one.hand_filter_counts().tolist() == [[0, 0, 0, 0, 0]]


def test_the_hand_limit_counts_survivors(ctxs):
    """more than 8192 hands reach the handle search unfiltered (AGH_ERR_CAPACITY); an aperture that leaves fewer succeeds"""
    from agile_grasp_amd import binding

    one, ref = ctxs
    sc = HF.box_scene(2)
    samples = np.tile(sc["samples"], 60)
    with pytest.raises(binding.AghError) as e:
        one.localize_depth(sc["images"], sc["ws"], samples=samples, classify=False, min_inliers=2)
    assert e.value.code == binding.AGH_ERR_CAPACITY and "8192" in str(e.value)
    fp = HF.scene_filters(sc)["aperture"]
    _set(one, fp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=samples, classify=False, min_inliers=2)
    reason, h = _check(got, ref, sc["images"], sc["ws"], fp, "8192", classify=False)
    c = HF.counts(reason)
    print("hypotheses", c[0], "survivors", c[4])
    assert c[0] > 8192 > c[4] == len(h) and one.hand_filter_counts().tolist() == [c]


# ---- chain forms ----

def _batch_captures():
    """three depth captures with unequal image sizes, counts, formats and poses"""
    return [HF.box_scene(2), HF.box_scene(1, fmt=D.F32, pad=2, w=128, h=96, f=160.0), HF.box_scene(2, w=144, h=100, f=180.0)]


@pytest.mark.parametrize("name", ["all", "aperture"])
def test_depth_batch_equals_single_calls(ctxs, svm_model, name):
    one, ref = ctxs
    caps = _batch_captures()
    fp = HF.scene_filters(caps[0])[name]
    _set(one, fp)
    (single,) = _contexts(caps[0]["origins"], svm_model, n=1)
    _set(single, fp)
    images, ws = [c["images"] for c in caps], [c["ws"] for c in caps]
    got = one.localize_depth_batch(images, ws, n_samples=[150, 120, 90], sample_seeds=[3, 4, 5], **KW)
    counts = one.hand_filter_counts()
    assert counts.shape == (3, 5)
    for k, c in enumerate(caps):
        want = single.localize_depth(c["images"], c["ws"], n_samples=[150, 120, 90][k], sample_seed=[3, 4, 5][k], **KW)
        _same(got[k], want, f"capture {k}")
        assert counts[k].tolist() == single.hand_filter_counts()[0].tolist()
        reason, _ = _check(got[k], ref, c["images"], c["ws"], fp, f"capture {k}")
        assert counts[k].tolist() == HF.counts(reason)
    print(name, counts.tolist())
    total = counts.sum(0)
    if name == "all":
        assert total[4] >= 5 and (total[1:4] >= 1).all()
    else:
        assert total[2] >= 5 and total[4] >= 5
    single.close()


def test_labeled_call_with_two_objects(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    fp = HF.scene_filters(sc)["all"]
    _set(one, fp)
    got = one.localize_depth_labeled(sc["images"], HF.label_images(sc), sc["ws"], 2, n_samples=80, sample_seed=6, **KW)
    counts = one.hand_filter_counts()
    assert len(got) == 2 and counts.shape == (2, 5)
    for j in range(2):
        assert (got[j]["samples"] >= 0).all()
        reason, _ = _check(got[j], ref, sc["images"], sc["ws"], fp, f"object {j}")
        assert counts[j].tolist() == HF.counts(reason)
    assert counts[0, 0] >= 20 and counts[0, 1:4].sum() >= 5 and counts[:, 4].sum() >= 5


def test_clustered_call(ctxs):
    from agile_grasp_amd import binding

    one, ref = ctxs
    sc = HF.box_scene(2)
    fp = HF.scene_filters(sc)["all"]
    _set(one, fp)
    cp = binding.cluster_params(plane=HF.table_plane(), min_voxels=50, max_objects=2)
    got = one.localize_depth_clustered(sc["images"], sc["ws"], cp, n_samples=100, sample_seed=8, **KW)
    counts = one.hand_filter_counts()
    assert len(got) == 2 and counts.shape == (2, 5)
    reason, _ = _check(got[0], ref, sc["images"], sc["ws"], fp, "object 0")
    assert counts[0].tolist() == HF.counts(reason) and counts[0, 0] >= 20 and counts[0, 1:4].sum() >= 5
    assert got[1]["n_hypotheses"] == 0 and counts[1].tolist() == [0, 0, 0, 0, 0]  # (the scene has one object)


def test_staged_stream_and_mid_chain_calls(ctxs):
    from agile_grasp_amd import binding

    one, ref = ctxs
    caps = [HF.box_scene(2), HF.box_scene(2, seed=6, f=190.0)]
    fp = HF.scene_filters(caps[0])["all"]
    _set(one, fp)
    one.localize_depth_begin(caps[0]["images"], caps[0]["ws"], n_samples=150, sample_seed=2, **KW)
    one.localize_depth_stage(caps[1]["images"])
    # mid-chain: the setter and the counts are refused, the getter answers
    for call in (lambda: one.set_hand_filter(**fp), one.clear_hand_filter, one.hand_filter_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    held = one.get_hand_filter()
    assert held is not None and held.view_on == 1 and held.max_unobserved == fp["max_unobserved"]
    got = one.localize_end()
    reason, _ = _check(got, ref, caps[0]["images"], caps[0]["ws"], fp, "capture 0")
    assert one.hand_filter_counts().tolist() == [HF.counts(reason)]
    one.localize_depth_begin(caps[1]["images"], caps[1]["ws"], n_samples=150, sample_seed=2, **KW)  # (adopts the staged set)
    got = one.localize_end()
    reason, _ = _check(got, ref, caps[1]["images"], caps[1]["ws"], fp, "capture 1")
    c = HF.counts(reason)
    assert one.hand_filter_counts().tolist() == [c] and c[3] >= 1 and c[4] >= 1


def test_together_with_the_boundary_filter(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    ws = sc["ws"].copy()
    vox = sc["vox"][sc["samples"]].astype(np.float64)
    ws[1] = float(np.median(vox[:, 0])) + 0.01  # a face through the box: the boundary filter bites too
    fp = HF.scene_filters(sc)["all"]
    _set(one, fp)
    for classify in (True, False):
        got = one.localize_depth(sc["images"], ws, n_samples=200, sample_seed=4, classify=classify, min_inliers=2,
                                 filters_boundaries=True)
        reason, h = _check(got, ref, sc["images"], ws, fp, f"boundaries, classify {classify}", classify=classify, boundaries=True)
        _, _, _, _, hyps = _route(ref, sc["images"], ws, fp, got["samples"], classify=classify)
        near = _near(hyps, ws)
        print("near", int(near.sum()), "near and kept by the hand filter", int((near & (reason == 0)).sum()))
        assert (near & (reason == 0)).sum() >= 1 and (~near & (reason != 0)).sum() >= 1
        assert one.hand_filter_counts().tolist() == [HF.counts(reason)]


# ---- refusals and identity ----

def test_refusals(ctxs):
    from agile_grasp_amd import binding

    one, _ = ctxs
    sc = HF.box_scene(2)
    good = HF.scene_filters(sc)["all"]
    bad = [(dict(approach_on=2), "approach_on"), (dict(width_on=-1), "width_on"), (dict(view_on=3), "view_on"),
           (dict(approach_dir=(0.0, 0.0, 1.001)), "approach_dir"), (dict(approach_dir=(np.nan, 0.0, 1.0)), "approach_dir[0]"),
           (dict(min_approach_cos=1.5), "min_approach_cos"), (dict(min_approach_cos=np.nan), "min_approach_cos"),
           (dict(min_width=-0.01), "min_width"), (dict(min_width=0.05, max_width=0.04), "min_width"),
           (dict(max_width=np.inf), "max_width"), (dict(probes_per_finger=0), "probes_per_finger"),
           (dict(probes_per_finger=17), "probes_per_finger"), (dict(depth_margin=-1e-9), "depth_margin"),
           (dict(depth_margin=np.inf), "depth_margin"), (dict(max_unobserved=-1), "max_unobserved")]
    _set(one, good)
    for b, field in bad:
        with pytest.raises(binding.AghError) as e:
            one.set_hand_filter(**dict(good, **b))
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and field in str(e.value), b
    held = one.get_hand_filter()  # (the filter held before stays in force)
    assert held.max_unobserved == good["max_unobserved"] and held.min_approach_cos == good["min_approach_cos"]
    one.set_hand_filter(**dict(good, approach_dir=(0.0, 0.0, 1.0 + 4e-7)))  # (inside the unit-vector tolerance)
    _set(one, good)
    # view_on with any form that takes points: refused, the text says why
    pts = D.deproject_ref(sc["images"])
    left = sc["images"][0]["data"].size
    calls = [lambda: one.localize(pts, left, sc["ws"], n_samples=10, dense=True, **KW),
             lambda: one.localize_begin(pts, left, sc["ws"], n_samples=10, dense=True, **KW),
             lambda: one.localize_masked(pts, left, sc["ws"], np.ones(len(pts), np.uint8), n_samples=10, dense=True, **KW),
             lambda: one.localize_labeled(pts, left, sc["ws"], np.ones(len(pts), np.uint8), 1, n_samples=10, dense=True, **KW),
             lambda: one.localize_clustered(pts, left, sc["ws"], binding.cluster_params(plane=HF.table_plane()), n_samples=10, dense=True, **KW),
             lambda: one.localize_batch([pts], [left], [sc["ws"]], n_samples=10, dense=True, **KW),
             lambda: one.localize_batch_begin([pts], [left], [sc["ws"]], n_samples=10, dense=True, **KW)]
    for call in calls:
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "needs depth images" in str(e.value)
    # a pose that is no rotation
    skew = [dict(im) for im in sc["images"]]
    skew[1]["pose"] = np.array(skew[1]["pose"])
    skew[1]["pose"][:, 0] *= 1.001
    for call in (lambda: one.localize_depth(skew, sc["ws"], n_samples=10, **KW),
                 lambda: one.localize_depth_batch([sc["images"], skew], [sc["ws"]] * 2, n_samples=10, **KW)):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "orthonormal" in str(e.value) and "image 1" in str(e.value)
    assert "capture 1, image 1" in str(e.value)  # (the batch's text names the capture too)
    # ... which the same context accepts without the view criterion, as it always did
    _set(one, dict(good, view_on=0))
    assert one.localize_depth(skew, sc["ws"], n_samples=10, **KW)["n_voxels"] > 0
    assert one.localize(pts, left, sc["ws"], n_samples=10, dense=True, **KW)["n_voxels"] > 0


def test_set_then_clear_is_never_set(ctxs, svm_model):
    one, _ = ctxs
    sc = HF.box_scene(2)
    (fresh,) = _contexts(sc["origins"], svm_model, n=1)
    kw = dict(KW, n_samples=150, sample_seed=9)
    want = fresh.localize_depth(sc["images"], sc["ws"], **kw)
    assert fresh.hand_filter_counts().shape == (0, 5) and fresh.get_hand_filter() is None
    _set(one, HF.scene_filters(sc)["all"])
    filtered = one.localize_depth(sc["images"], sc["ws"], **kw)
    assert len(filtered["hands"]) < len(want["hands"])
    one.clear_hand_filter()
    assert one.get_hand_filter() is None
    _same(one.localize_depth(sc["images"], sc["ws"], **kw), want, "cleared")
    assert one.hand_filter_counts().shape == (0, 5)
    caps = _batch_captures()
    args = ([c["images"] for c in caps], [c["ws"] for c in caps])
    bkw = dict(KW, n_samples=[100, 80, 60], sample_seeds=[1, 2, 3])
    want_b = fresh.localize_depth_batch(*args, **bkw)
    got_b = one.localize_depth_batch(*args, **bkw)
    for k in range(3):
        _same(got_b[k], want_b[k], f"cleared, capture {k}")
    fresh.close()
