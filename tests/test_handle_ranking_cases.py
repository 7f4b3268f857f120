"""The regimes of tests/handle_ranking_cases.py, proven on the CPU: the wave sum is not the sequential sum, the constructed lists
hold exact ties, signed zeros, NaN and infinite scores, a score exactly at min_score and best_inlier ties, and on the
box-on-a-table scene, with the oracle's hands, the default ranking's order is not the discovery order -- so a GPU test that finds a
regime empty has found a fault."""
import numpy as np
import pytest

from tests import handle_ranking_cases as R
from tests import hand_filter_cases as HF


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("n", [65, 128, 129, 2048])
def test_the_wave_sum_is_not_the_sequential_sum(n):
    g = R.cancelling_margins(n)
    w, s = R.wave_sum(g), R.sequential_sum(g)
    print(n, repr(w), repr(s))
    assert _bits(w) != _bits(s) and abs(w - s) <= 1e-6 * abs(s)
    hands, marg, handles, idx = R.make_list([n], g, seed=2)
    sc = R.scores(R.MARGIN_ONLY, hands, marg, handles, idx)
    assert _bits(sc["terms"][0, 1]) == _bits(np.float64(R.wave_sum(marg[idx])) / np.float64(n))


@pytest.mark.parametrize("n", [128, 2048])
def test_a_swap_of_lane_halves_ties_the_wave_sum_only(n):
    """the butterfly's first step adds lane l and lane l ^ 32: with those lanes' values swapped W is bit for bit the same, the
    sequential sum is not -- two such handles tie exactly, and a kernel with another order would rank them by rounding noise"""
    hands, marg, handles, idx = R.swapped_pair(n)
    a, b = marg[idx[:n]], marg[idx[n:]]
    assert _bits(R.wave_sum(a)) == _bits(R.wave_sum(b)) and _bits(R.sequential_sum(a)) != _bits(R.sequential_sum(b))
    assert R.sequential_sum(a) < R.sequential_sum(b)  # (a sequential kernel would put handle 1 first)
    sc = R.scores(R.MARGIN_ONLY, hands, marg, handles, idx)
    assert _bits(sc["score"][0]) == _bits(sc["score"][1]) and R.order(sc, R.MARGIN_ONLY)[0].tolist() == [0, 1]


def test_wave_sum_edges():
    assert R.wave_sum([]) == 0.0 and not np.signbit(R.wave_sum([]))
    assert R.wave_sum([-0.0]) == 0.0 and not np.signbit(R.wave_sum([-0.0]))  # (from +0.0: -0 never survives)
    assert R.wave_sum([1.5]) == 1.5
    v = np.arange(1.0, 131.0)
    assert R.wave_sum(v) == v.sum()  # (small integers: every order is exact)
    assert np.isnan(R.wave_sum([1.0, np.nan])) and R.wave_sum([np.inf, 1.0]) == np.inf and np.isnan(R.wave_sum([np.inf, -np.inf]))
    # lane l holds v[l] + v[l + 64]: a pair that cancels inside its lane leaves the small values intact
    v = np.zeros(128)
    v[0], v[64], v[1] = 1e300, -1e300, 1.0
    assert R.wave_sum(v) == 1.0 and R.sequential_sum(v) == 0.0  # (in sequence 1e300 absorbs the 1.0 before its partner arrives)
    v[64], v[65] = 0.0, -1e300  # (now lane 1 holds 1.0 - 1e300: the 1.0 is absorbed there, and the butterfly cancels the rest)
    assert R.wave_sum(v) == 0.0


def test_special_scores_order():
    hands, g, handles, idx = R.singles(R.SPECIAL_SCORES)
    sc = R.scores(R.MARGIN_ONLY, hands, g, handles, idx)
    assert R.same_bytes(np.where(sc["score"] == 0.0, 0.0, sc["score"]), np.where(R.SPECIAL_SCORES == 0.0, 0.0, R.SPECIAL_SCORES))
    keep, below = R.order(sc, R.MARGIN_ONLY)
    # +inf (4, 9), 3.0 (12), 0.5 (0, 6), the zeros of either sign by index (3, 5, 10, 13), -1 (7), -inf (2, 11), NaN (1, 8)
    assert keep.tolist() == [4, 9, 12, 0, 6, 3, 5, 10, 13, 7, 2, 11, 1, 8] and below == 0
    keep, below = R.order(sc, dict(R.MARGIN_ONLY, min_score=-1.0))  # (a finite bound leaves NaN and what lies below out)
    assert keep.tolist() == [4, 9, 12, 0, 6, 3, 5, 10, 13, 7] and below == 4
    keep, below = R.order(sc, dict(R.MARGIN_ONLY, min_score=float(np.nextafter(-1.0, 0.0))))
    assert keep.tolist() == [4, 9, 12, 0, 6, 3, 5, 10, 13] and below == 5
    keep, below = R.order(sc, dict(R.MARGIN_ONLY, max_handles=3))
    assert keep.tolist() == [4, 9, 12] and below == 0
    keep, below = R.order(sc, dict(R.MARGIN_ONLY, min_score=0.5, max_handles=100))
    assert keep.tolist() == [4, 9, 12, 0, 6] and below == 9


def test_signed_zeros_tie():
    values = np.array([-0.0, 0.0, 0.25, -0.0, 0.0])
    hands, g, handles, idx = R.signed_zero_list(values)
    sc = R.scores(R.SIGNED_ZERO, hands, g, handles, idx)
    assert np.signbit(sc["score"]).tolist() == [True, False, True, True, False] and (sc["score"][[0, 1, 3, 4]] == 0.0).all()
    assert sc["score"][2] < -0.2 and sc["terms"][:, 2].tolist() == [1.0, -1.0, 1.0, 1.0, -1.0] and (sc["terms"][:, 3] > 0.0).all()
    keep, _ = R.order(sc, R.SIGNED_ZERO)
    assert keep.tolist() == [0, 1, 3, 4, 2]  # (the zeros of either sign tie: by index)
    for bound in (0.0, -0.0):  # (-0 >= +0 and +0 >= -0)
        keep, below = R.order(sc, dict(R.SIGNED_ZERO, min_score=bound))
        assert keep.tolist() == [0, 1, 3, 4] and below == 1


def test_a_nan_term_poisons_the_score_under_weight_zero():
    hands, g, handles, idx = R.singles([1.0, 2.0, 3.0])
    handles["width"][1] = np.nan
    handles["center"][2] = np.inf  # (0 x inf is NaN too)
    sc = R.scores(R.DEFAULTS, hands, g, handles, idx)
    assert np.isnan(sc["score"]).tolist() == [False, True, True] and R.order(sc, R.DEFAULTS)[0].tolist() == [0, 1, 2]


def test_best_inlier():
    assert R.best_inlier([1.0, 3.0, 3.0, 2.0]) == 1
    assert R.best_inlier([np.nan, np.nan]) == 0
    assert R.best_inlier([np.nan, -np.inf, -np.inf]) == 1
    assert R.best_inlier([0.0, -0.0, 0.0]) == 0
    g = np.zeros(129)
    g[[70, 5, 128]] = 7.0
    assert R.best_inlier(g) == 5
    hands, marg, handles, idx = R.make_list([129], g, shuffle=False)
    assert R.scores(R.DEFAULTS, hands, marg, handles, idx)["best_inlier"].tolist() == [5]


def test_terms_against_their_definitions():
    hands, g, handles, idx = R.make_list([3, 12, 1], np.linspace(0.1, 1.6, 16), seed=4)
    rp = R.params(w_approach=0.5, w_position=-2.0, w_distance=0.25, w_width=-3.0, w_length=4.0, ref_point=(0.1, -0.2, 0.3),
                  preferred_width=0.04, approach_dir=(0.0, 0.6, -0.8), position_dir=(1.0, 2.0, 3.0))
    sc = R.scores(rp, hands, g, handles, idx)
    assert sc["terms"][:, 0].tolist() == [0.3, 1.0, 0.1] and sc["index"].tolist() == [0, 1, 2]
    for h in range(3):
        m = idx[handles[h]["first_inlier"]:][:handles[h]["n_inliers"]]
        t = sc["terms"][h]
        assert abs(t[1] - g[m].mean()) < 1e-12 and abs(t[2] - handles[h]["approach"] @ np.array(rp["approach_dir"])) < 1e-12
        assert abs(t[3] - handles[h]["center"] @ np.array(rp["position_dir"])) < 1e-12
        assert abs(t[4] - np.linalg.norm(handles[h]["center"] - np.array(rp["ref_point"]))) < 1e-12
        assert abs(t[5] - abs(handles[h]["width"] - 0.04)) < 1e-15
        x = hands["bottom"][m] @ handles[h]["axis"]
        assert abs(t[6] - (x.max() - x.min())) < 1e-12
        w = [rp[k] for k in R.WEIGHTS]
        assert abs(sc["score"][h] - float(np.dot(w, t))) < 1e-12
    assert sc["terms"][2, 6] == 0.0  # (one inlier: no length)


def test_default_ranking_reorders_the_box_scene(svm_model):
    """the oracle's hands on the box-on-a-table scene, its classifier's decision sums as margins, its handle search: the default
    ranking returns the handles in another order than they were found in"""
    from oracle import oracle_py as O

    w, rho = svm_model
    for n_views in (1, 2):
        sc = HF.box_scene(n_views)
        found = O.find_hands(O.default_params(sc["origins"]), sc["vox"], sc["cam"], sc["samples"], want_images=True)
        keep, sums = O.classify(found["images"], w, rho)
        keep = keep.astype(bool)
        assert (sums[keep] <= 0).all() and (sums[~keep] > 0).all()  # (the kept hands' margins are >= 0)
        hands, margins = found["hyps"][keep], -sums[keep]
        handles, idx = O.find_handles(hands, 2, 0.005)
        handles = np.ascontiguousarray(handles).view(R.HANDLE_DTYPE) if handles.dtype != R.HANDLE_DTYPE else handles
        ranked, scores, counts = R.rank(R.DEFAULTS, hands, margins, handles, idx)
        print(n_views, "views:", len(hands), "hands,", counts, "order", scores["index"].tolist())
        assert counts == [len(handles), 0, len(handles)] and len(handles) >= 3
        assert scores["index"].tolist() != list(range(len(handles)))
        assert sorted(scores["index"].tolist()) == list(range(len(handles)))
        assert (np.diff(scores["score"]) <= 0).all() and (scores["terms"][:, 1] >= 0).all()
        top = R.rank(dict(R.DEFAULTS, max_handles=1), hands, margins, handles, idx)
        assert R.same_bytes(top[0], ranked[:1]) and top[2] == [len(handles), 0, 1]
