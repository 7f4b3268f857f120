"""agh_set_hand_clearance (include/agh.h; DESIGN.md, "Hand clearance"): the approach-corridor test as a stage of every localize
chain.  Every result is held, bit for bit (epoch aside), against the stage-wise route on the samples the call reports --
agh_find_hands -> [the hand filter's numpy model] -> the numpy model of tests/hand_clearance_cases.py, brute force over the whole
voxelised cloud -> [filterHands] -> agh_classify's kept -> agh_find_handles on a second context that never has a setting -- and
the per-list counts against the model's.  The regimes are those tests/test_hand_clearance_cases.py proves on the CPU; a test that
finds one empty fails."""
import numpy as np
import pytest

from tests import depth_captures as D
from tests import hand_clearance_cases as HC
from tests import hand_filter_cases as HF
from tests.test_gpu_boundary_chain import _assert_same, _contexts, _near
from tests.test_gpu_hand_filter import _samples_for_count
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
    pair[0].clear_hand_clearance()
    pair[0].clear_hand_filter()
    yield pair
    pair[0].clear_hand_clearance()
    pair[0].clear_hand_filter()


def _hyps(ref, images, ws, samples, points=None, size_left=None):
    """the unfiltered chain's hypotheses for `samples`, their sample points and the voxelised cloud (stage-wise, on `ref`)"""
    pts = D.deproject_ref(images) if points is None else points
    ref.preprocess(pts, images[0]["data"].size if size_left is None else size_left, ws, dense=True)
    vox, _ = ref.cloud()
    samples = np.asarray(samples, np.int32)
    hyps = ref.find_hands(samples).copy()
    return hyps, vox[samples[hyps["sample"]]], vox


def _route(ref, images, ws, cp, samples, fp=None, classify=True, boundaries=False, min_inliers=2, points=None, size_left=None):
    """the hands, handles and inlier lists the chain must return for `samples`; the model's drops, the hand filter's reasons (None
    without one) and the hypotheses"""
    hyps, spts, vox = _hyps(ref, images, ws, samples, points, size_left)
    keep = ref.classify().astype(bool) if classify and len(hyps) else np.ones(len(hyps), bool)
    reason = HF.drop_reasons(hyps, spts, fp, images) if fp is not None else None
    dropped = HC.drop(hyps, spts, vox, cp, reason)
    ok = ~dropped
    if reason is not None:
        ok &= reason == 0
    if boundaries:
        ok &= ~_near(hyps, ws)
    if classify:
        hyps["svm_keep"] = keep
    h = hyps[keep & ok]
    hd, idx = ref.find_handles(h, min_inliers, 0.005)
    return h, hd, idx, dropped, reason, hyps


def _check(got, ref, images, ws, cp, what, **kw):
    h, hd, idx, dropped, reason, hyps = _route(ref, images, ws, cp, got["samples"], **kw)
    print(what, "hypotheses", len(hyps), "model counts", HC.counts(dropped, reason), "hands", len(h), "handles", len(hd))
    assert got["n_hypotheses"] == len(hyps), what  # the search's unfiltered count
    _assert_same(got, h, hd, idx)
    return dropped, reason, h


# ---- 1. chain equality and counts ----

@pytest.mark.parametrize("name", ["defaults", "body"])
@pytest.mark.parametrize("classify", [True, False])
@pytest.mark.parametrize("n_views", [1, 2])
def test_depth_chain_equals_the_stagewise_route(ctxs, n_views, classify, name):
    one, ref = ctxs
    sc = HF.box_scene(n_views)
    cp = HC.params(**(HC.BODY if name == "body" else {}))
    one.set_hand_clearance(**cp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], classify=classify, min_inliers=2)
    dropped, _, h = _check(got, ref, sc["images"], sc["ws"], cp, f"{n_views} views, {name}, classify {classify}", classify=classify)
    c = HC.counts(dropped)
    assert one.hand_clearance_counts().tolist() == [c] and c[0] == c[1] + c[2] == got["n_hypotheses"]
    assert HC.bites(dropped) and len(h) >= 1
    assert one.hand_filter_counts().shape == (0, 5)  # (only a clearance is set)
    if not classify:
        assert len(h) == c[2]


@pytest.mark.parametrize("classify", [True, False])
def test_points_chain(ctxs, classify):
    one, ref = ctxs
    sc = HF.box_scene(2)
    cp = HC.params()
    one.set_hand_clearance(**cp)
    pts = D.deproject_ref(sc["images"])
    left = sc["images"][0]["data"].size
    got = one.localize(pts, left, sc["ws"], samples=sc["samples"], dense=True, classify=classify, min_inliers=2)
    dropped, _, h = _check(got, ref, sc["images"], sc["ws"], cp, f"points, classify {classify}", classify=classify)
    assert one.hand_clearance_counts().tolist() == [HC.counts(dropped)] and HC.bites(dropped) and len(h) >= 1


def test_general_svm_model_skips_the_dropped_hands(svm_model):
    """the descriptor + kernel-row path (k_hog_svm without a model, k_svm_decide) honours the clearance's drop bytes too"""
    sc = HF.box_scene(2)
    one, ref = _contexts(sc["origins"], svm_model, general=True)
    cp = HC.params()
    one.set_hand_clearance(**cp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    dropped, _, h = _check(got, ref, sc["images"], sc["ws"], cp, "general model")
    assert one.hand_clearance_counts().tolist() == [HC.counts(dropped)] and len(h) >= 1
    one.close()
    ref.close()


# ---- 2. the count is exact ----

@pytest.mark.parametrize("n_views", [1, 2])
def test_the_count_is_the_threshold(ctxs, n_views):
    one, ref = ctxs
    sc = HF.box_scene(n_views)
    hyps, spts, vox = _hyps(ref, sc["images"], sc["ws"], sc["samples"])
    c = HC.corridor_counts(hyps, spts, vox, HC.DEFAULTS)
    i = HC.pick_small_count(c)
    assert i is not None, "no hand with 1 .. 10 points in its corridor: the scene lost its regime"
    for max_points, kept in ((int(c[i]), True), (int(c[i]) - 1, False)):
        cp = HC.params(max_points=max_points)
        one.set_hand_clearance(**cp)
        got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], classify=False, min_inliers=2)
        dropped, _, _ = _check(got, ref, sc["images"], sc["ws"], cp, f"hand {i}, count {c[i]}, max_points {max_points}", classify=False)
        assert (not dropped[i]) == kept and one.hand_clearance_counts().tolist() == [HC.counts(dropped)]


# ---- 3. faces are closed, the arithmetic is the contract's ----

def _face_cases(xb, yb, zb, inside):
    """per face (field, the value that puts the face exactly on a point, the next value inwards): the point is the corridor's
    outermost one towards that face, so moving the face inwards loses it"""
    j = np.flatnonzero(inside)
    far, near = float(-yb[j].min()), float(-yb[j].max())
    hw, hh = float(np.abs(xb[j]).max()), float(np.abs(zb[j]).max())
    out = [("far_offset", far, float(np.nextafter(far, 0.0))), ("half_width", hw, float(np.nextafter(hw, 0.0))),
           ("half_height", hh, float(np.nextafter(hh, 0.0)))]
    if near > 0.0:  # (near_offset = 0 is the record's bound: no face can lie beyond it)
        out.append(("near_offset", near, float(np.nextafter(near, 1.0))))
    return out


def test_faces_are_closed(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    hyps, spts, vox = _hyps(ref, sc["images"], sc["ws"], sc["samples"])
    c = HC.corridor_counts(hyps, spts, vox, HC.DEFAULTS)
    i = HC.pick_small_count(c)
    assert i is not None
    xb, yb, zb = (v[0] for v in HC.body_coords(hyps[i:i + 1], HC.palm_points(hyps[i:i + 1], spts[i:i + 1]), vox))
    cases = _face_cases(xb, yb, zb, HC.in_corridor(xb, yb, zb, HC.params()))
    assert len(cases) >= 3
    for field, on, inwards in cases:
        assert 0.0 < on <= (0.5 if field.endswith("offset") else 0.25)
        c_in = int(HC.corridor_counts(hyps[i:i + 1], spts[i:i + 1], vox, {field: inwards})[0])
        c_on = int(HC.corridor_counts(hyps[i:i + 1], spts[i:i + 1], vox, {field: on})[0])
        assert c_on > c_in, field  # the point on the face counts
        for value, kept in ((on, False), (inwards, True)):
            cp = HC.params(**{field: value, "max_points": c_in})
            one.set_hand_clearance(**cp)
            got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], classify=False, min_inliers=2)
            dropped, _, _ = _check(got, ref, sc["images"], sc["ws"], cp, f"{field} = {value!r}", classify=False)
            assert (not dropped[i]) == kept, (field, value)
            assert one.hand_clearance_counts().tolist() == [HC.counts(dropped)]


# ---- 4. launch shapes ----

@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 130])
def test_launch_shapes(ctxs, count):
    """hypothesis counts around a wave's worth of work-groups and around the work-group's four waves (63, 65 and 130 are no
    multiples of four), with a hand filter in front (the kernel reads the bytes) and without (it writes every byte)"""
    one, ref = ctxs
    sc = HF.box_scene(2)
    hyps, _, _ = _hyps(ref, sc["images"], sc["ws"], sc["samples"])
    if count == 0:
        per = np.bincount(hyps["sample"], minlength=len(sc["samples"]))
        samples = sc["samples"][per == 0][:3]
        assert len(samples) >= 1
    else:
        samples = _samples_for_count(hyps, sc["samples"], count)
    cp = HC.params()
    fp_all = dict(HF.scene_filters(sc)["all"], view_on=0)
    for fp in (None, fp_all):
        one.set_hand_clearance(**cp)
        if fp is not None:
            one.set_hand_filter(**fp)
        got = one.localize_depth(sc["images"], sc["ws"], samples=samples, classify=False, min_inliers=2)
        dropped, reason, _ = _check(got, ref, sc["images"], sc["ws"], cp, f"{count} hypotheses, filter {fp is not None}", classify=False, fp=fp)
        assert got["n_hypotheses"] == count and one.hand_clearance_counts().tolist() == [HC.counts(dropped, reason)]


def test_no_samples_at_all(ctxs):
    one, _ = ctxs
    sc = HF.box_scene(1)
    one.set_hand_clearance()
    got = one.localize_depth(sc["images"], sc["ws"], n_samples=0, classify=False)
    assert got["n_hypotheses"] == 0 and one.hand_clearance_counts().tolist() == [[0, 0, 0]]


# ---- 5. grid edges ----

def _median_split(ref, sc, ws, base):
    """`base` with max_points at the median of the model's counts: both regimes non-empty however large the corridor"""
    hyps, spts, vox = _hyps(ref, sc["images"], ws, sc["samples"])
    c = np.sort(HC.corridor_counts(hyps, spts, vox, base))
    cp = HC.params(**dict(base, max_points=int(c[len(c) // 2])))
    assert HC.bites(HC.drop(hyps, spts, vox, cp)), "the median splits nothing"
    return cp


def test_largest_corridor_leaves_the_grid_through_every_face(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    cp = _median_split(ref, sc, sc["ws"], HC.LARGEST)
    ext = sc["vox"].max(0) - sc["vox"].min(0)
    assert (ext < 0.5).all()  # (the cloud is smaller than the corridor's reach: its box leaves the grid on every side)
    one.set_hand_clearance(**cp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    dropped, _, _ = _check(got, ref, sc["images"], sc["ws"], cp, f"largest corridor, max_points {cp['max_points']}")
    assert cp["max_points"] > 100 and one.hand_clearance_counts().tolist() == [HC.counts(dropped)]


@pytest.mark.parametrize("name", ["defaults", "largest"])
def test_kept_descriptor_that_no_longer_covers_the_cloud(ctxs, name):
    """a build of the tightly cropped capture leaves its small descriptor; the next chain, on the whole capture, bins into it: the
    points outside sit clamped in border cells (open faces) and must still be counted"""
    one, ref = ctxs
    sc = HF.box_scene(2)
    cp = HC.params() if name == "defaults" else _median_split(ref, sc, sc["ws"], HC.LARGEST)
    one.localize_depth(sc["images"], sc["ws_tight"], n_samples=10, classify=False)
    one.localize_depth(sc["images"], sc["ws_tight"], n_samples=10, classify=False)  # (the descriptor kept is the tight cloud's own)
    before = one.grid_stats()
    one.set_hand_clearance(**cp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    after, desc = one.grid_stats(), one.grid_desc()
    print(before, after, desc)
    assert after["misses"] == before["misses"] + 1 and after["cold"] == before["cold"] and desc["open"] != 0
    dropped, _, _ = _check(got, ref, sc["images"], sc["ws"], cp, f"kept descriptor, {name}")
    assert HC.bites(dropped) and one.hand_clearance_counts().tolist() == [HC.counts(dropped)]


def test_cloud_inside_one_grid_cell(svm_model):
    """a capture cropped to less than a grid cell (2 cm), in a fresh context: the grid is one cell"""
    sc = HF.box_scene(2)
    one, ref = _contexts(sc["origins"], svm_model)
    centre = sc["vox"][sc["samples"][len(sc["samples"]) // 2]].astype(np.float64)
    ws = np.array([centre[0] - 0.009, centre[0] + 0.009, centre[1] - 0.009, centre[1] + 0.009, centre[2] - 0.009, centre[2] + 0.009])
    for cold, cp in ((True, HC.params()), (False, HC.params(**HC.LARGEST))):
        one.set_hand_clearance(**cp)
        got = one.localize_depth(sc["images"], ws, n_samples=12, sample_seed=2, classify=False, min_inliers=2)
        desc = one.grid_desc()
        print(desc, got["n_voxels"], got["n_hypotheses"])
        assert got["n_voxels"] >= 12 and (got["samples"] >= 0).all() and desc["cell"] >= 0.02
        # (the context's first build takes the cloud's own box: one cell; the second one bins into the descriptor the first
        # left, that box padded by two cells on every face)
        assert desc["dim"] == ((1, 1, 1) if cold else (5, 5, 5))
        dropped, _, _ = _check(got, ref, sc["images"], ws, cp, "one cell", classify=False)
        assert one.hand_clearance_counts().tolist() == [HC.counts(dropped)]
    one.close()
    ref.close()


# ---- 6. batches and per-object lists ----

def _lifted(sc, by=0.05):
    """the same capture with its cameras (and so its whole cloud) moved `by` metres along the table's normal: the images are
    identical, the clouds are not -- this capture's table lies where the other captures' hands approach from"""
    a, b, c, _ = HF.table_plane()
    off = by * np.array([a, b, c])
    images = []
    for im in sc["images"]:
        pose = np.array(im["pose"], np.float64)
        pose[:3, 3] += off
        images.append(dict(im, pose=pose))
    ws = sc["ws"] + np.repeat(off, 2)
    return dict(sc, images=images, ws=ws)


def _batch_captures():
    """three depth captures with unequal image sizes, counts and formats, the second one another scene (the table 5 cm higher)"""
    return [HF.box_scene(2), _lifted(HF.box_scene(1, fmt=D.F32, pad=2, w=128, h=96, f=160.0)), HF.box_scene(2, w=144, h=100, f=180.0)]


def test_depth_batch_equals_single_calls_and_sees_its_own_cloud_only(ctxs, svm_model):
    one, ref = ctxs
    caps = _batch_captures()
    cp = HC.params()
    one.set_hand_clearance(**cp)
    (single,) = _contexts(caps[0]["origins"], svm_model, n=1)
    single.set_hand_clearance(**cp)
    images, ws = [c["images"] for c in caps], [c["ws"] for c in caps]
    got = one.localize_depth_batch(images, ws, n_samples=[150, 120, 90], sample_seeds=[3, 4, 5], **KW)
    counts = one.hand_clearance_counts()
    assert counts.shape == (3, 3) and one.hand_filter_counts().shape == (0, 5)
    clouds, mine = [], []
    for k, c in enumerate(caps):
        want = single.localize_depth(c["images"], c["ws"], n_samples=[150, 120, 90][k], sample_seed=[3, 4, 5][k], **KW)
        _same(got[k], want, f"capture {k}")
        assert counts[k].tolist() == single.hand_clearance_counts()[0].tolist()
        dropped, _, _ = _check(got[k], ref, c["images"], c["ws"], cp, f"capture {k}")
        assert counts[k].tolist() == HC.counts(dropped)
        hyps, spts, vox = _hyps(ref, c["images"], c["ws"], got[k]["samples"])
        clouds.append(vox)
        mine.append((hyps, spts, dropped))
    print(counts.tolist())
    assert counts[:, 1].sum() >= 1 and counts[:, 2].sum() >= 5
    # the test bites: a kernel that counted another capture's points too would decide otherwise
    everything = np.concatenate(clouds)
    assert any((HC.drop(h, s, everything, cp) != d).any() for h, s, d in mine)
    single.close()


def test_labeled_call_with_two_objects(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    cp = HC.params()
    one.set_hand_clearance(**cp)
    got = one.localize_depth_labeled(sc["images"], HF.label_images(sc), sc["ws"], 2, n_samples=80, sample_seed=6, **KW)
    counts = one.hand_clearance_counts()
    assert len(got) == 2 and counts.shape == (2, 3)
    for j in range(2):
        assert (got[j]["samples"] >= 0).all()
        dropped, _, _ = _check(got[j], ref, sc["images"], sc["ws"], cp, f"object {j}")  # (the WHOLE cloud of the capture is tested)
        assert counts[j].tolist() == HC.counts(dropped)
    assert counts[0, 0] >= 20 and counts[:, 1].sum() >= 1 and counts[:, 2].sum() >= 5


def test_clustered_call(ctxs):
    from agile_grasp_amd import binding

    one, ref = ctxs
    sc = HF.box_scene(2)
    cp = HC.params()
    one.set_hand_clearance(**cp)
    cl = binding.cluster_params(plane=HF.table_plane(), min_voxels=50, max_objects=2)
    got = one.localize_depth_clustered(sc["images"], sc["ws"], cl, n_samples=100, sample_seed=8, **KW)
    counts = one.hand_clearance_counts()
    assert len(got) == 2 and counts.shape == (2, 3)
    dropped, _, _ = _check(got[0], ref, sc["images"], sc["ws"], cp, "object 0")
    assert counts[0].tolist() == HC.counts(dropped) and counts[0, 0] >= 20 and counts[0, 1] >= 1 and counts[0, 2] >= 5
    assert got[1]["n_hypotheses"] == 0 and counts[1].tolist() == [0, 0, 0]  # (the scene has one object)


def test_labeled_depth_batch_where_a_list_is_not_its_capture(ctxs):
    one, ref = ctxs
    plain = [HF.box_scene(2), HF.box_scene(1, fmt=D.F32, pad=2, w=128, h=96, f=160.0), HF.box_scene(2, w=144, h=100, f=180.0)]
    caps = _batch_captures()
    cp = HC.params()
    one.set_hand_clearance(**cp)
    labels = [HF.label_images(c) for c in plain]  # (the lifted capture's images are the plain one's: so are its labels)
    n_objects = [2, 2, 1]
    got = one.localize_depth_batch_labeled([c["images"] for c in caps], labels, [c["ws"] for c in caps], n_objects,
                                           n_samples=[80, 70, 60], sample_seeds=[3, 4, 5], **KW)
    counts = one.hand_clearance_counts()
    assert [len(g) for g in got] == n_objects and counts.shape == (5, 3)
    got = [obj for g in got for obj in g]  # (list order: capture after capture, object after object)
    for l, k in enumerate([0, 0, 1, 1, 2]):
        assert (got[l]["samples"] >= 0).all()
        dropped, _, _ = _check(got[l], ref, caps[k]["images"], caps[k]["ws"], cp, f"list {l} of capture {k}")
        assert counts[l].tolist() == HC.counts(dropped)
    print(counts.tolist())
    box_lists = counts[[0, 2, 4]]
    assert (box_lists[:, 0] >= 20).all() and box_lists[:, 1].sum() >= 1 and box_lists[:, 2].sum() >= 5


# ---- 7. together with the hand filter and filters_boundaries ----

def test_together_with_the_hand_filter_and_the_boundary_filter(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    fp = HF.scene_filters(sc)["all"]
    cp = HC.params()
    # the reasons come in order: a hand the filter dropped is not the clearance's, whatever its corridor holds
    one.set_hand_filter(**fp)
    one.set_hand_clearance(**cp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    dropped, reason, h = _check(got, ref, sc["images"], sc["ws"], cp, "hand filter, then clearance", fp=fp)
    hyps, spts, vox = _hyps(ref, sc["images"], sc["ws"], sc["samples"])
    alone = HC.drop(hyps, spts, vox, cp)
    assert (alone & (reason != 0)).sum() >= 1 and not (dropped & (reason != 0)).any() and dropped.sum() >= 1 and len(h) >= 1
    assert one.hand_filter_counts().tolist() == [HF.counts(reason)] and one.hand_clearance_counts().tolist() == [HC.counts(dropped, reason)]
    # ... and with filters_boundaries a hand goes if any of the three says so
    ws = sc["ws"].copy()
    at = sc["vox"][sc["samples"]].astype(np.float64)
    ws[1] = float(np.median(at[:, 0])) + 0.01  # a face through the box: the boundary filter bites too
    for classify in (True, False):
        kw = dict(n_samples=200, sample_seed=4, classify=classify, min_inliers=2, filters_boundaries=True)
        one.clear_hand_clearance()
        one.localize_depth(sc["images"], ws, **kw)
        without = one.hand_filter_counts().tolist()
        assert one.hand_clearance_counts().shape == (0, 3)
        one.set_hand_clearance(**cp)
        got = one.localize_depth(sc["images"], ws, **kw)
        dropped, reason, h = _check(got, ref, sc["images"], ws, cp, f"all three, classify {classify}", classify=classify, boundaries=True, fp=fp)
        near = _near(_hyps(ref, sc["images"], ws, got["samples"])[0], ws)
        print("filter", HF.counts(reason), "clearance", HC.counts(dropped, reason), "near", int(near.sum()))
        assert dropped.sum() >= 1 and near.sum() >= 1
        assert one.hand_filter_counts().tolist() == without == [HF.counts(reason)]  # unchanged by the clearance
        c = one.hand_clearance_counts().tolist()
        assert c == [HC.counts(dropped, reason)] and c[0][0] == without[0][4]  # n_tested = the hand filter's n_kept


# ---- 8. streams and mid-chain calls ----

def test_staged_stream_and_mid_chain_calls(ctxs):
    from agile_grasp_amd import binding

    one, ref = ctxs
    caps = [HF.box_scene(2), HC.two_scene()]
    cp = HC.params(far_offset=0.15)
    one.set_hand_clearance(**cp)
    one.localize_depth_begin(caps[0]["images"], caps[0]["ws"], n_samples=150, sample_seed=2, **KW)
    one.localize_depth_stage(caps[1]["images"])
    # mid-chain: the setter and the counts are refused, the getter answers
    for call in (lambda: one.set_hand_clearance(**cp), one.clear_hand_clearance, one.hand_clearance_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    held = one.get_hand_clearance()
    assert held is not None and held.far_offset == 0.15 and held.max_points == 0
    got = one.localize_end()
    dropped, _, _ = _check(got, ref, caps[0]["images"], caps[0]["ws"], cp, "capture 0")
    assert one.hand_clearance_counts().tolist() == [HC.counts(dropped)]
    one.localize_depth_begin(caps[1]["images"], caps[1]["ws"], n_samples=150, sample_seed=2, **KW)  # (adopts the staged set)
    got = one.localize_end()
    dropped, _, _ = _check(got, ref, caps[1]["images"], caps[1]["ws"], cp, "capture 1")
    assert one.hand_clearance_counts().tolist() == [HC.counts(dropped)] and dropped.any() and (~dropped).sum() >= 5
    # a batch chain refuses them too
    one.localize_depth_batch_begin([c["images"] for c in caps], [c["ws"] for c in caps], n_samples=[60, 60], sample_seeds=[1, 2], **KW)
    for call in (lambda: one.set_hand_clearance(**cp), one.hand_clearance_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    assert one.get_hand_clearance().far_offset == 0.15
    got = one.localize_batch_end()
    counts = one.hand_clearance_counts()
    for k, c in enumerate(caps):
        dropped, _, _ = _check(got[k], ref, c["images"], c["ws"], cp, f"batch stream, capture {k}")
        assert counts[k].tolist() == HC.counts(dropped)


# ---- 9. refusals ----

def test_refusals(ctxs):
    from agile_grasp_amd import binding

    one, _ = ctxs
    good = HC.params(far_offset=0.2, max_points=3)
    bad = [(dict(near_offset=-0.01), "near_offset"), (dict(near_offset=np.nan), "near_offset"), (dict(near_offset=np.inf), "near_offset"),
           (dict(near_offset=0.2), "far_offset"), (dict(near_offset=0.3), "far_offset"), (dict(far_offset=0.5000001), "far_offset"),
           (dict(far_offset=np.nan), "far_offset"), (dict(far_offset=np.inf), "far_offset"),
           (dict(half_width=0.0), "half_width"), (dict(half_width=-0.05), "half_width"), (dict(half_width=0.2500001), "half_width"),
           (dict(half_width=np.nan), "half_width"), (dict(half_height=0.0), "half_height"), (dict(half_height=0.26), "half_height"),
           (dict(half_height=-np.inf), "half_height"), (dict(max_points=-1), "max_points")]
    one.set_hand_clearance(**good)
    for b, field in bad:
        with pytest.raises(binding.AghError) as e:
            one.set_hand_clearance(**dict(good, **b))
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and field in str(e.value), b
        held = one.get_hand_clearance()  # (the setting held before stays in force)
        assert (held.near_offset, held.far_offset, held.half_width, held.half_height, held.max_points) == (0.0, 0.2, 0.05, 0.04, 3)
    one.set_hand_clearance(**HC.LARGEST)  # (the bounds themselves are legal)
    assert one.get_hand_clearance().far_offset == 0.5
    # no form is refused: the points forms run with it
    sc = HF.box_scene(2)
    pts = D.deproject_ref(sc["images"])
    left = sc["images"][0]["data"].size
    one.set_hand_clearance(**good)
    assert one.localize(pts, left, sc["ws"], n_samples=10, dense=True, **KW)["n_voxels"] > 0
    assert one.hand_clearance_counts().shape == (1, 3)
    got = one.localize_batch([pts], [left], [sc["ws"]], n_samples=10, dense=True, **KW)
    assert got[0]["n_voxels"] > 0 and one.hand_clearance_counts().shape == (1, 3)


# ---- 10. set, then clear ----

def test_set_then_clear_is_never_set(ctxs, svm_model):
    one, _ = ctxs
    sc = HF.box_scene(2)
    (fresh,) = _contexts(sc["origins"], svm_model, n=1)
    kw = dict(KW, n_samples=150, sample_seed=9)
    want = fresh.localize_depth(sc["images"], sc["ws"], **kw)
    assert fresh.hand_clearance_counts().shape == (0, 3) and fresh.get_hand_clearance() is None
    one.set_hand_clearance()
    assert one.get_hand_filter() is None
    cleared = one.localize_depth(sc["images"], sc["ws"], **kw)
    assert len(cleared["hands"]) <= len(want["hands"]) and one.hand_clearance_counts()[0, 1] >= 1
    assert one.hand_clearance_counts().shape == (1, 3) and one.hand_filter_counts().shape == (0, 5)
    one.clear_hand_clearance()
    assert one.get_hand_clearance() is None
    _same(one.localize_depth(sc["images"], sc["ws"], **kw), want, "cleared")
    assert one.hand_clearance_counts().shape == (0, 3) and one.hand_filter_counts().shape == (0, 5)
    caps = _batch_captures()
    args = ([c["images"] for c in caps], [c["ws"] for c in caps])
    bkw = dict(KW, n_samples=[100, 80, 60], sample_seeds=[1, 2, 3])
    want_b = fresh.localize_depth_batch(*args, **bkw)
    got_b = one.localize_depth_batch(*args, **bkw)
    for k in range(3):
        _same(got_b[k], want_b[k], f"cleared, capture {k}")
    assert one.hand_clearance_counts().shape == (0, 3)
    fresh.close()


# ---- 11. the settings take turns on one context ----

def test_settings_alternate_on_one_context(ctxs, svm_model):
    """what a chain leaves for the two counts getters is that chain's alone: filter only, clearance only, neither, both, a
    two-capture depth batch with both, then a single chain with the clearance only, all on one context, each step held against a
    fresh context that ran nothing but that step with the same settings"""
    one, _ = ctxs
    sc, sc2 = HF.box_scene(2), HF.box_scene(2, w=144, h=100, f=180.0)
    fp, cp = HF.scene_filters(sc)["all"], HC.params()
    single = lambda c: [c.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)]
    batch = lambda c: c.localize_depth_batch([sc["images"], sc2["images"]], [sc["ws"], sc2["ws"]], samples=[sc["samples"], sc2["samples"]], **KW)
    steps = [("filter only", fp, None, single, 1), ("clearance only", None, cp, single, 1), ("neither", None, None, single, 1),
             ("both", fp, cp, single, 1), ("batch with both", fp, cp, batch, 2), ("clearance only, after the batch", None, cp, single, 1)]
    for what, f, cl, run, lists in steps:
        (fresh,) = _contexts(sc["origins"], svm_model, n=1)
        for c in (one, fresh):
            c.clear_hand_filter()
            c.clear_hand_clearance()
            if f is not None:
                c.set_hand_filter(**f)
            if cl is not None:
                c.set_hand_clearance(**cl)
        got, want = run(one), run(fresh)
        fc, cc = one.hand_filter_counts(), one.hand_clearance_counts()
        print(what, "filter", fc.tolist(), "clearance", cc.tolist(), "hands", [len(g["hands"]) for g in got])
        assert len(got) == len(want) == lists, what
        for k in range(lists):
            _same(got[k], want[k], f"{what}, list {k}")
        assert fc.tolist() == fresh.hand_filter_counts().tolist() and cc.tolist() == fresh.hand_clearance_counts().tolist(), what
        # (no records exactly where the test is not set, one per list of THIS chain where it is)
        assert fc.shape == ((lists, 5) if f is not None else (0, 5)) and cc.shape == ((lists, 3) if cl is not None else (0, 3)), what
        if f is not None and cl is not None:  # both tests bite and both keep: every list drops and keeps under each
            assert (fc[:, 1:4].sum(1) >= 1).all() and (fc[:, 4] >= 1).all() and (cc[:, 1] >= 1).all() and (cc[:, 2] >= 1).all(), what
            assert (cc[:, 0] == fc[:, 4]).all() and all(len(g["hands"]) >= 1 for g in got), what
        fresh.close()
