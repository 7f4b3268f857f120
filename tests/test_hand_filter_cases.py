"""The regimes of tests/hand_filter_cases.py, proven on the CPU with the oracle's hypotheses: on each scene every criterion alone
drops at least five hands and keeps at least five, and the combined filter drops hands under each of the three reasons -- so a
GPU test that finds a regime empty has found a fault.  And the model's own edges: the order of the reasons, a NaN record, the
bite table."""
import numpy as np
import pytest

from tests import hand_filter_cases as HF


@pytest.fixture(scope="module")
def oracle_hands():
    from oracle import oracle_py as O

    out = {}
    for n_views in (1, 2):
        sc = HF.box_scene(n_views)
        hyps = O.find_hands(O.default_params(sc["origins"]), sc["vox"], sc["cam"], sc["samples"])["hyps"]
        out[n_views] = (sc, hyps, sc["vox"][sc["samples"][hyps["sample"]]])
    return out


@pytest.mark.parametrize("n_views", [1, 2])
def test_every_regime_bites_and_leaves_hands(oracle_hands, n_views):
    sc, hyps, pts = oracle_hands[n_views]
    assert 64 <= len(sc["samples"]) <= 300 and all(im["data"].shape == (HF.H, HF.W) for im in sc["images"])
    filters = HF.scene_filters(sc)
    for name, reason_id in (("cone", 1), ("aperture", 2), ("view", 3)):
        c = HF.counts(HF.drop_reasons(hyps, pts, filters[name], sc["images"]))
        print(n_views, name, c)
        assert c[reason_id] >= 5 and c[4] >= 5 and c[0] == c[reason_id] + c[4]
    c = HF.counts(HF.drop_reasons(hyps, pts, filters["all"], sc["images"]))
    print(n_views, "all", c)
    assert min(c[1:4]) >= 1 and c[4] >= 5 and c[0] == sum(c[1:])


def test_a_hand_counts_under_the_first_criterion_that_drops_it(oracle_hands):
    sc, hyps, pts = oracle_hands[1]
    f = HF.scene_filters(sc)
    alone = {k: HF.drop_reasons(hyps, pts, f[k], sc["images"]) != 0 for k in ("cone", "aperture", "view")}
    both = HF.drop_reasons(hyps, pts, dict(f["cone"], width_on=1, min_width=f["aperture"]["min_width"],
                                           max_width=f["aperture"]["max_width"]), sc["images"])
    assert (alone["cone"] & alone["aperture"]).sum() >= 1
    assert np.array_equal(both == 1, alone["cone"]) and np.array_equal(both == 2, alone["aperture"] & ~alone["cone"])


def test_a_second_view_observes_more(oracle_hands):
    """the same probes are unobserved less often with two cameras: what the criterion is for"""
    sc1, hyps, pts = oracle_hands[1]
    sc2 = HF.box_scene(2)
    fp = HF.scene_filters(sc1)["view"]
    w = HF.probes(hyps, pts, fp)
    one = HF.seen(w, sc1["images"][0], fp["depth_margin"])
    two = one | HF.seen(w, sc2["images"][1], fp["depth_margin"])
    assert np.array_equal(sc1["images"][0]["data"], sc2["images"][0]["data"])
    assert two.sum() > one.sum() and not (one & ~two).any()


def test_nan_records_are_kept(oracle_hands):
    sc, hyps, pts = oracle_hands[2]
    f = HF.scene_filters(sc)["all"]
    r = HF.drop_reasons(hyps, pts, f, sc["images"])
    h = hyps.copy()
    h["approach"][:] = np.nan
    h["width"][:] = np.nan
    assert (r != 0).sum() >= 5 and not HF.drop_reasons(h, pts, f, sc["images"]).any()


def test_bite_table_is_the_sweeps():
    t = HF.bite_table(HF.GEOMETRY)
    assert len(t) == 11 and t[0] == 0.01 and t[1] == 0.01 + 0.005 and t[-1] <= 0.06
    d = 0.01
    for k in range(1, 11):
        d += 0.005
        assert t[k] == d
