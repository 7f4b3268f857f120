"""agh_set_handle_ranking / agh_rank_handles (include/agh.h; DESIGN.md, "Handle ranking"): every list of a localize chain leaves in
rank order.  Exact equality throughout: the ranked handles, byte for byte, and their score records (score, terms, index,
best_inlier) equal the numpy model of tests/handle_ranking_cases.py on what a context that never heard of the call returns for the
same chain, plus agh_get_hand_margins; and equal agh_rank_handles on the same.  The stage-wise call reaches the shapes no scene
produces.  The regimes are those tests/test_handle_ranking_cases.py proves on the CPU."""
import numpy as np
import pytest

from tests import depth_captures as D
from tests import hand_clearance_cases as HC
from tests import hand_filter_cases as HF
from tests import handle_ranking_cases as R
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
# every term under a weight of its own
ALL = dict(w_support=0.5, w_margin=1.5, w_approach=0.75, w_position=-2.0, w_distance=0.25, w_width=-3.0, w_length=4.0,
           ref_point=(0.1, -0.2, 0.3), preferred_width=0.04, approach_dir=(0.0, 0.6, -0.8), position_dir=(1.0, 2.0, 3.0))
NO_MARGIN = dict(w_support=1.0, w_margin=0.0, w_position=1.0, w_length=2.0)


def _rec(rp):
    from agile_grasp_amd import binding

    return binding.handle_ranking_params(**rp)


@pytest.fixture(scope="module")
def pair(svm_model):
    """(the context under test, a context that never has a ranking), the two-view scene's camera origins"""
    one, ref = _contexts(HF.box_scene(2)["origins"], svm_model)
    yield one, ref
    one.close()
    ref.close()


@pytest.fixture
def ctxs(pair):
    def reset():
        pair[0].clear_handle_ranking()
        for c in pair:
            c.clear_hand_clearance()
            c.clear_hand_filter()

    reset()
    yield pair
    reset()


def _stage(ctx, rp, hands, margins, handles, idx, what=""):
    """agh_rank_handles against the model, byte for byte"""
    got = ctx.rank_handles(_rec(rp), hands, margins, handles, idx)
    want = R.rank(rp, hands, margins, handles, idx)
    assert got[2] == want[2], (what, got[2], want[2])
    assert np.array_equal(got[1]["index"], want[1]["index"]), what
    assert R.same_scores(got[1], want[1]), what
    assert R.same_bytes(got[0], want[0]), what
    return got


def _check(one, ref, got, want, rp, classify=True, what=""):
    """the ranked chain's lists `got` against the unranked chain's `want` (a context that never has a ranking): everything but the
    handles is the unranked call's; the handles and the three getters equal the model and agh_rank_handles"""
    scores, margins, counts = one.handle_scores(), one.hand_margins(), one.handle_ranking_counts()
    assert len(counts) == len(got) == len(want), what
    s0 = m0 = 0
    out = []
    for l, (g, w) in enumerate(zip(got, want)):
        at = f"{what}, list {l}"
        _same(dict(g, handles=w["handles"]), w, at)  # (hands, inlier_idx, samples, counts: untouched)
        m = margins[m0:m0 + len(w["hands"])]
        if classify:
            assert (m >= 0).all(), at  # (kept hands)
        else:
            assert not m.any() and not np.signbit(m).any(), at
        hd, sc, cnt = R.rank(rp, w["hands"], m if classify else None, w["handles"], w["inlier_idx"])
        print(at, "counts", cnt, "order", sc["index"].tolist())
        assert counts[l].tolist() == cnt and len(g["handles"]) == cnt[2], at
        assert R.same_bytes(g["handles"], hd), at
        assert R.same_scores(scores[s0:s0 + cnt[2]], sc), at
        hd2, sc2, cnt2 = ref.rank_handles(_rec(rp), w["hands"], m if classify else None, w["handles"], w["inlier_idx"])
        assert cnt2 == cnt and R.same_bytes(hd2, hd) and R.same_scores(sc2, sc), at
        s0 += cnt[2]
        m0 += len(w["hands"])
        out.append((sc, m))
    assert s0 == len(scores) and m0 == len(margins), what
    return out


# ---- 1. stage-wise shapes ----

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 8192])
def test_handle_counts_around_the_sort_sizes(pair, n):
    """one inlier each; the margins are drawn from n / 2 + 1 values, so that exact ties abound"""
    rng = np.random.default_rng(n)
    values = rng.integers(0, n // 2 + 1, n) / 8.0
    hands, g, handles, idx = R.singles(values)
    got = _stage(pair[0], R.MARGIN_ONLY, hands, g, handles, idx, f"{n} handles")
    assert got[2] == [n, 0, n]
    if n >= 63:
        assert len(np.unique(values)) < n and (np.diff(got[1]["score"]) <= 0).all()
    _stage(pair[0], ALL, hands, g, handles, idx, f"{n} handles, every term")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 2048])
def test_one_handle_of_n_inliers(pair, n):
    hands, g, handles, idx = R.make_list([n], R.cancelling_margins(n), seed=n)
    _stage(pair[0], ALL, hands, g, handles, idx, f"{n} inliers")
    if n > 64:  # (in list order the wave sum of these margins is not their sequential sum: tests/test_handle_ranking_cases.py)
        hands, g, handles, idx = R.make_list([n], R.cancelling_margins(n), seed=n, shuffle=False)
        got = _stage(pair[0], ALL, hands, g, handles, idx, f"{n} inliers, in list order")
        assert got[1]["terms"][0, 1] == R.wave_sum(g) / n != R.sequential_sum(g) / n
    # ... among other handles, the inlier lists interleaved
    hands, g, handles, idx = R.make_list([3, n, 1, 70], R.cancelling_margins(n + 74), seed=n + 1)
    _stage(pair[0], ALL, hands, g, handles, idx, f"{n} inliers, among others")


@pytest.mark.parametrize("n", [128, 2048])
def test_the_wave_sum_ties_where_a_sequential_sum_would_not(pair, n):
    hands, g, handles, idx = R.swapped_pair(n)
    got = _stage(pair[0], R.MARGIN_ONLY, hands, g, handles, idx, "swapped pair")
    assert got[1]["index"].tolist() == [0, 1] and got[1]["score"][0] == got[1]["score"][1]


@pytest.mark.parametrize("name", ["ascending", "descending", "equal"])
def test_presorted_inputs(pair, name):
    values = dict(ascending=np.arange(300.0), descending=np.arange(300.0)[::-1].copy(), equal=np.full(300, 2.5))[name]
    hands, g, handles, idx = R.singles(values)
    got = _stage(pair[0], R.MARGIN_ONLY, hands, g, handles, idx, name)
    assert got[1]["index"].tolist() == (list(range(299, -1, -1)) if name == "ascending" else list(range(300)))


def test_nan_infinite_and_signed_zero_scores(pair):
    hands, g, handles, idx = R.singles(R.SPECIAL_SCORES)
    got = _stage(pair[0], R.MARGIN_ONLY, hands, g, handles, idx, "special scores")
    assert got[1]["index"].tolist() == [4, 9, 12, 0, 6, 3, 5, 10, 13, 7, 2, 11, 1, 8]
    for bound, n_ret in ((-1.0, 10), (float(np.nextafter(-1.0, 0.0)), 9), (0.5, 5), (float(np.nextafter(0.5, 1.0)), 3)):
        got = _stage(pair[0], dict(R.MARGIN_ONLY, min_score=bound), hands, g, handles, idx, f"min_score {bound!r}")
        assert got[2] == [14, 14 - n_ret, n_ret]
    hands, g, handles, idx = R.signed_zero_list([-0.0, 0.0, 0.25, -0.0, 0.0])
    got = _stage(pair[0], R.SIGNED_ZERO, hands, g, handles, idx, "signed zeros")
    assert got[1]["index"].tolist() == [0, 1, 3, 4, 2] and np.signbit(got[1]["score"]).tolist() == [True, False, True, False, True]
    for bound in (0.0, -0.0):
        assert _stage(pair[0], dict(R.SIGNED_ZERO, min_score=bound), hands, g, handles, idx, "zero bound")[2] == [5, 1, 4]
    # a NaN term under weight 0
    hands, g, handles, idx = R.singles([1.0, 2.0, 3.0])
    handles["width"][1] = np.nan
    handles["center"][2] = np.inf
    got = _stage(pair[0], R.DEFAULTS, hands, g, handles, idx, "NaN terms")
    assert np.isnan(got[1]["score"]).tolist() == [False, True, True] and got[1]["index"].tolist() == [0, 1, 2]
    assert _stage(pair[0], dict(R.DEFAULTS, min_score=0.0), hands, g, handles, idx, "NaN terms, bound")[2] == [3, 2, 1]


def test_max_handles_and_margins_null(pair):
    n = 37
    hands, g, handles, idx = R.make_list([2] * n, np.random.default_rng(1).uniform(0, 2, 2 * n), seed=9)
    for k in (0, 1, n, n + 1):
        got = _stage(pair[0], dict(ALL, max_handles=k), hands, g, handles, idx, f"max_handles {k}")
        assert got[2] == [n, 0, n if k == 0 else min(k, n)]
    got = _stage(pair[0], dict(ALL, max_handles=5, min_score=float(np.median(R.scores(ALL, hands, g, handles, idx)["score"]))),
                 hands, g, handles, idx, "max_handles and min_score")
    assert got[2] == [n, n // 2, 5]
    got = _stage(pair[0], ALL, hands, None, handles, idx, "no margins")
    assert not got[1]["terms"][:, 1].any() and not got[1]["best_inlier"].any()


def test_best_inlier_ties(pair):
    g = np.zeros(129 + 4 + 3 + 2)
    g[[70, 5, 128]] = 7.0
    g[129:133] = [1.0, 3.0, 3.0, 2.0]
    g[133:136] = [np.nan, -np.inf, -np.inf]
    g[136:138] = np.nan
    hands, g, handles, idx = R.make_list([129, 4, 3, 2], g, shuffle=False)
    got = pair[0].rank_handles(_rec(R.DEFAULTS), hands, g, handles, idx)
    by_index = got[1][np.argsort(got[1]["index"])]
    assert by_index["best_inlier"].tolist() == [5, 1, 1, 0]
    _stage(pair[0], R.DEFAULTS, hands, g, handles, idx, "best_inlier")


def test_refusals(ctxs):
    from agile_grasp_amd import binding

    one, _ = ctxs
    good = dict(ALL, max_handles=3)
    bad = [(dict(w_support=np.nan), "w_support"), (dict(w_margin=np.inf), "w_margin"), (dict(w_length=-np.inf), "w_length"),
           (dict(approach_dir=(0.0, 0.0, -1.001)), "approach_dir"), (dict(approach_dir=(np.nan, 0.0, -1.0)), "approach_dir"),
           (dict(approach_dir=(0.0, 0.0, 0.0)), "approach_dir"), (dict(position_dir=(0.0, np.inf, 1.0)), "position_dir"),
           (dict(ref_point=(np.nan, 0.0, 0.0)), "ref_point"), (dict(preferred_width=np.nan), "preferred_width"),
           (dict(min_score=np.nan), "min_score"), (dict(min_score=np.inf), "min_score"), (dict(support_cap=0), "support_cap"),
           (dict(support_cap=-3), "support_cap"), (dict(max_handles=-1), "max_handles")]
    hands, g, handles, idx = R.make_list([2, 3], np.arange(5.0))
    one.set_handle_ranking(**good)
    for b, field in bad:
        for call in (lambda: one.set_handle_ranking(**dict(good, **b)),
                     lambda: one.rank_handles(_rec(dict(good, **b)), hands, g, handles, idx)):
            with pytest.raises(binding.AghError) as e:
                call()
            assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and field in str(e.value), b
        held = one.get_handle_ranking()  # (the setting held before stays in force)
        assert (held.w_support, held.max_handles, held.approach_dir[1], held.min_score) == (0.5, 3, 0.6, -np.inf)
    one.set_handle_ranking(position_dir=(0.0, 0.0, 0.0), approach_dir=(0.0, 0.0, 1.0 + 4e-7))  # (legal: |a^2 + b^2 + c^2 - 1| = 8e-7)
    # agh_rank_handles' own
    with pytest.raises(binding.AghError) as e:
        one.rank_handles(None, hands, g, handles, idx)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "rp" in str(e.value)
    for field, value, text in (("n_inliers", 0, "n_inliers"), ("n_inliers", 4, "outside n_idx"), ("first_inlier", -1, "outside n_idx"),
                               ("first_inlier", 3, "outside n_idx")):
        h = handles.copy()
        h[field][1] = value
        with pytest.raises(binding.AghError) as e:
            one.rank_handles(_rec(good), hands, g, h, idx)
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and text in str(e.value), (field, value)
    for value in (5, -1):
        i = idx.copy()
        i[3] = value
        with pytest.raises(binding.AghError) as e:
            one.rank_handles(_rec(good), hands, g, handles, i)
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "outside n_hands" in str(e.value)
    big_hands, big_g, big_handles, big_idx = R.singles(np.zeros(8193))
    for args in ((big_hands, big_g, handles, idx), (hands, g, big_handles, big_idx)):
        with pytest.raises(binding.AghError) as e:
            one.rank_handles(_rec(good), *args)
        assert e.value.code == binding.AGH_ERR_CAPACITY and "8192" in str(e.value)
    with pytest.raises(binding.AghError) as e:
        one.rank_handles(_rec(dict(good, max_handles=0)), hands, g, handles, idx, cap=1)
    assert e.value.code == binding.AGH_ERR_CAPACITY and one.last_rank_counts == [2, 0, 2]
    # the chain call: w_margin needs the classifier
    sc = HF.box_scene(1)
    one.set_handle_ranking()
    for call in (lambda: one.localize_depth(sc["images"], sc["ws"], n_samples=10, classify=False),
                 lambda: one.localize_depth_batch([sc["images"]], [sc["ws"]], n_samples=[10], classify=False),
                 lambda: one.localize(D.deproject_ref(sc["images"]), sc["images"][0]["data"].size, sc["ws"], n_samples=10, dense=True,
                                      classify=False)):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "w_margin" in str(e.value)
    # the getters without a ranked chain behind them
    one.clear_handle_ranking()
    one.localize_depth(sc["images"], sc["ws"], n_samples=10, classify=False)
    for call in (one.handle_scores, one.handle_ranking_counts, one.hand_margins):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE


# ---- 2. chains ----

@pytest.mark.parametrize("name", ["defaults", "all"])
@pytest.mark.parametrize("n_views", [1, 2])
def test_depth_chain(ctxs, n_views, name):
    one, ref = ctxs
    sc = HF.box_scene(n_views)
    rp = R.params(**(ALL if name == "all" else {}))
    one.set_handle_ranking(**rp)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    want = ref.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    ((scores, margins),) = _check(one, ref, [got], [want], rp, what=f"{n_views} views, {name}")
    assert len(want["handles"]) >= 3 and scores["index"].tolist() != list(range(len(scores)))  # (the ranking bites)
    # the margins are minus the decision sums of the stage-wise search, hypothesis by hypothesis
    ref.preprocess(D.deproject_ref(sc["images"]), sc["images"][0]["data"].size, sc["ws"], dense=True)
    hyps = ref.find_hands(np.asarray(sc["samples"], np.int32)).copy()
    keep = ref.classify().astype(bool)
    _, sums = ref.hog()
    assert len(hyps) == got["n_hypotheses"] and keep.sum() == len(got["hands"])
    assert np.array_equal(hyps["sample"][keep], got["hands"]["sample"]) and np.array_equal(hyps["orientation"][keep], got["hands"]["orientation"])
    assert R.same_bytes(margins, -sums[keep])
    # top-k and a bound on the same chain
    bound = float(scores["score"][1])
    for extra, n_ret in ((dict(max_handles=1), 1), (dict(min_score=bound), 2), (dict(min_score=float(np.nextafter(bound, np.inf))), 1)):
        one.set_handle_ranking(**dict(rp, **extra))
        got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
        _check(one, ref, [got], [want], dict(rp, **extra), what=str(extra))
        assert len(got["handles"]) == n_ret and len(got["inlier_idx"]) == len(want["inlier_idx"])


def test_points_chain_and_handle_cap_is_judged_on_the_returned_count(ctxs):
    from agile_grasp_amd import binding

    one, ref = ctxs
    sc = HF.box_scene(2)
    pts, left = D.deproject_ref(sc["images"]), sc["images"][0]["data"].size
    one.set_handle_ranking(**ALL)
    got = one.localize(pts, left, sc["ws"], samples=sc["samples"], dense=True, **KW)
    want = ref.localize(pts, left, sc["ws"], samples=sc["samples"], dense=True, **KW)
    _check(one, ref, [got], [want], R.params(**ALL), what="points")
    n = len(want["handles"])
    assert n >= 3
    # a batch call's caps: (handles, inlier indices, hands)
    caps = (2, len(want["inlier_idx"]), len(want["hands"]))
    with pytest.raises(binding.AghError) as e:
        one.localize_batch([pts], [left], [sc["ws"]], samples=[sc["samples"]], dense=True, caps=caps, **KW)
    assert e.value.code == binding.AGH_ERR_CAPACITY and one.last_batch_counts[0]["n_handles"] == n
    one.set_handle_ranking(**dict(ALL, max_handles=2))
    (got,) = one.localize_batch([pts], [left], [sc["ws"]], samples=[sc["samples"]], dense=True, caps=caps, **KW)
    _check(one, ref, [got], [want], R.params(**dict(ALL, max_handles=2)), what="points batch, two handles' room")
    assert len(got["handles"]) == 2 and one.last_batch_counts[0]["n_handles"] == 2


def test_without_a_classifier(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    one.set_handle_ranking(**NO_MARGIN)
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], classify=False, min_inliers=2)
    want = ref.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], classify=False, min_inliers=2)
    ((scores, _),) = _check(one, ref, [got], [want], R.params(**NO_MARGIN), classify=False, what="classify 0")
    assert len(scores) >= 3 and not scores["terms"][:, 1].any()


def test_general_svm_model(svm_model):
    sc = HF.box_scene(2)
    one, ref = _contexts(sc["origins"], svm_model, general=True)
    one.set_handle_ranking()
    got = one.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    want = ref.localize_depth(sc["images"], sc["ws"], samples=sc["samples"], **KW)
    ((scores, margins),) = _check(one, ref, [got], [want], R.DEFAULTS, what="general model")
    assert len(scores) >= 3 and margins.any()
    one.close()
    ref.close()


# ---- 3. batches and per-object lists ----

def _batch_captures():
    return [HF.box_scene(2), HF.box_scene(1, fmt=D.F32, pad=2, w=128, h=96, f=160.0), HF.box_scene(2, w=144, h=100, f=180.0)]


def test_depth_batch_with_a_capture_without_handles(ctxs):
    one, ref = ctxs
    caps = _batch_captures()
    args = ([c["images"] for c in caps], [c["ws"] for c in caps])
    kw = dict(KW, n_samples=[150, 0, 90], sample_seeds=[3, 4, 5])
    one.set_handle_ranking(**ALL)
    got = one.localize_depth_batch(*args, **kw)
    want = ref.localize_depth_batch(*args, **kw)
    res = _check(one, ref, got, want, R.params(**ALL), what="depth batch")
    assert [len(s) for s, _ in res][1] == 0 and len(res[0][0]) >= 2 and len(res[2][0]) >= 1
    assert one.handle_ranking_counts()[1].tolist() == [0, 0, 0]


def test_labeled_and_clustered_calls(ctxs):
    from agile_grasp_amd import binding

    one, ref = ctxs
    sc = HF.box_scene(2)
    one.set_handle_ranking(**ALL)
    lab = HF.label_images(sc)
    kw = dict(KW, n_samples=80, sample_seed=6)
    got = one.localize_depth_labeled(sc["images"], lab, sc["ws"], 2, **kw)
    want = ref.localize_depth_labeled(sc["images"], lab, sc["ws"], 2, **kw)
    res = _check(one, ref, got, want, R.params(**ALL), what="labelled")
    assert len(res) == 2 and len(res[0][0]) >= 2
    cl = binding.cluster_params(plane=HF.table_plane(), min_voxels=50, max_objects=2)
    kw = dict(KW, n_samples=100, sample_seed=8)
    got = one.localize_depth_clustered(sc["images"], sc["ws"], cl, **kw)
    want = ref.localize_depth_clustered(sc["images"], sc["ws"], cl, **kw)
    res = _check(one, ref, got, want, R.params(**ALL), what="clustered")
    assert len(res) == 2 and len(res[0][0]) >= 2 and len(res[1][0]) == 0  # (the scene has one object)


def test_labeled_depth_batch_where_a_list_is_not_its_capture(ctxs):
    one, ref = ctxs
    caps = _batch_captures()
    labels = [HF.label_images(c) for c in caps]
    args = ([c["images"] for c in caps], labels, [c["ws"] for c in caps], [2, 2, 1])
    kw = dict(KW, n_samples=[80, 70, 60], sample_seeds=[3, 4, 5])
    one.set_handle_ranking(**dict(ALL, max_handles=2))
    got = one.localize_depth_batch_labeled(*args, **kw)
    want = ref.localize_depth_batch_labeled(*args, **kw)
    assert [len(g) for g in got] == [2, 2, 1]
    res = _check(one, ref, [o for g in got for o in g], [o for g in want for o in g], R.params(**dict(ALL, max_handles=2)),
                 what="labelled depth batch")
    counts = one.handle_ranking_counts()
    assert counts.shape == (5, 3) and (counts[:, 2] <= 2).all() and (counts[[0, 2, 4], 0] >= 2).all() and len(res) == 5


# ---- 4. with the other settings ----

def test_together_with_the_hand_filter_the_clearance_and_the_boundary_filter(ctxs):
    one, ref = ctxs
    sc = HF.box_scene(2)
    fp = dict(HF.scene_filters(sc)["all"])
    ws = sc["ws"].copy()
    ws[1] = float(np.median(sc["vox"][sc["samples"]].astype(np.float64)[:, 0])) + 0.01  # (a face through the box)
    for c in (one, ref):
        c.set_hand_filter(**fp)
        c.set_hand_clearance(**HC.params(max_points=40))
    for classify, rp in ((True, ALL), (False, NO_MARGIN)):
        kw = dict(n_samples=250, sample_seed=4, classify=classify, min_inliers=2, filters_boundaries=True)
        one.set_handle_ranking(**rp)
        got = one.localize_depth(sc["images"], ws, **kw)
        want = ref.localize_depth(sc["images"], ws, **kw)
        _check(one, ref, [got], [want], R.params(**rp), classify=classify, what=f"all settings, classify {classify}")
        fc, cc = one.hand_filter_counts(), one.hand_clearance_counts()
        print(fc.tolist(), cc.tolist(), len(want["handles"]))
        assert fc.tolist() == ref.hand_filter_counts().tolist() and cc.tolist() == ref.hand_clearance_counts().tolist()
        assert fc[0, 1:4].sum() >= 1 and len(want["hands"]) < fc[0, 0] and len(want["handles"]) >= 1


# ---- 5. streams and mid-chain calls ----

def test_staged_stream_and_mid_chain_calls(ctxs):
    from agile_grasp_amd import binding

    one, ref = ctxs
    caps = [HF.box_scene(2), HC.two_scene()]
    rp = R.params(**ALL)
    one.set_handle_ranking(**rp)
    hands, g, handles, idx = R.make_list([2, 3], np.arange(5.0))
    kw = dict(KW, n_samples=150, sample_seed=2)
    one.localize_depth_begin(caps[0]["images"], caps[0]["ws"], **kw)
    one.localize_depth_stage(caps[1]["images"])
    refused = (lambda: one.set_handle_ranking(**rp), one.clear_handle_ranking, one.handle_scores, one.handle_ranking_counts,
               one.hand_margins, lambda: one.rank_handles(_rec(rp), hands, g, handles, idx))
    for call in refused:
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    held = one.get_handle_ranking()
    assert held is not None and held.w_length == 4.0 and held.support_cap == 10
    got = one.localize_end()
    _check(one, ref, [got], [ref.localize_depth(caps[0]["images"], caps[0]["ws"], **kw)], rp, what="capture 0")
    one.localize_depth_begin(caps[1]["images"], caps[1]["ws"], **kw)  # (adopts the staged set)
    got = one.localize_end()
    _check(one, ref, [got], [ref.localize_depth(caps[1]["images"], caps[1]["ws"], **kw)], rp, what="capture 1")
    # a batch chain refuses them too
    args = ([c["images"] for c in caps], [c["ws"] for c in caps])
    bkw = dict(KW, n_samples=[60, 60], sample_seeds=[1, 2])
    one.localize_depth_batch_begin(*args, **bkw)
    for call in refused:
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    assert one.get_handle_ranking().w_width == -3.0
    got = one.localize_batch_end()
    _check(one, ref, got, ref.localize_depth_batch(*args, **bkw), rp, what="batch stream")


# ---- 6. state ----

def test_set_then_clear_is_never_set_and_settings_take_turns(ctxs, svm_model):
    from agile_grasp_amd import binding

    one, ref = ctxs
    sc = HF.box_scene(2)
    (fresh,) = _contexts(sc["origins"], svm_model, n=1)
    kw = dict(KW, n_samples=150, sample_seed=9)
    want = fresh.localize_depth(sc["images"], sc["ws"], **kw)
    assert fresh.get_handle_ranking() is None
    caps = _batch_captures()
    args = ([c["images"] for c in caps], [c["ws"] for c in caps])
    bkw = dict(KW, n_samples=[100, 80, 60], sample_seeds=[1, 2, 3])
    want_b = fresh.localize_depth_batch(*args, **bkw)
    # two settings take turns on one context, each chain's getters its own
    first, second = R.params(**ALL), R.params(max_handles=2, w_position=1.0)
    for rp in (first, second, first):
        one.set_handle_ranking(**rp)
        _check(one, ref, [one.localize_depth(sc["images"], sc["ws"], **kw)], [want], rp, what="single")
        _check(one, ref, one.localize_depth_batch(*args, **bkw), want_b, rp, what="batch")
    one.clear_handle_ranking()
    assert one.get_handle_ranking() is None
    _same(one.localize_depth(sc["images"], sc["ws"], **kw), want, "cleared")
    with pytest.raises(binding.AghError) as e:
        one.handle_scores()
    assert e.value.code == binding.AGH_ERR_STATE
    for k, g in enumerate(one.localize_depth_batch(*args, **bkw)):
        _same(g, want_b[k], f"cleared, capture {k}")
    fresh.close()
