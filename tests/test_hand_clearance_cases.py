"""The regimes of tests/hand_clearance_cases.py, proven on the CPU with the oracle's hypotheses: on each scene the default corridor
and a larger gripper body drop at least five hands and keep at least five, the fingers' own cross-section is clear for at least 95 %
of the hands (what the sweep guarantees), and a hand with 1 .. 10 points in its corridor exists for the threshold tests -- so a
GPU test that finds a regime empty has found a fault.  And the model's own edges: closed faces, a NaN record, the order behind the
hand filter."""
import numpy as np
import pytest

from tests import hand_clearance_cases as HC
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
    assert 64 <= len(sc["samples"]) <= 300 and len(sc["vox"]) <= 13000
    for name, cp in (("defaults", HC.DEFAULTS), ("body", HC.BODY)):
        d = HC.drop(hyps, pts, sc["vox"], cp)
        print(n_views, name, HC.counts(d))
        assert HC.bites(d), name
    c = HC.corridor_counts(hyps, pts, sc["vox"], HC.FINGERS)
    print(n_views, "fingers", int((c == 0).sum()), "of", len(c), "clear")
    assert HC.mostly_clear(c)
    c = HC.corridor_counts(hyps, pts, sc["vox"], HC.DEFAULTS)
    i = HC.pick_small_count(c)
    assert i is not None
    print(n_views, "hand", i, "has", int(c[i]), "points in its corridor")
    # the count is the threshold: max_points = c keeps the hand, c - 1 drops it
    assert not HC.drop(hyps, pts, sc["vox"], dict(max_points=int(c[i])))[i]
    assert HC.drop(hyps, pts, sc["vox"], dict(max_points=int(c[i]) - 1))[i]


def test_a_larger_body_drops_no_fewer_hands(oracle_hands):
    sc, hyps, pts = oracle_hands[2]
    small = HC.corridor_counts(hyps, pts, sc["vox"], HC.DEFAULTS)
    large = HC.corridor_counts(hyps, pts, sc["vox"], HC.BODY)
    largest = HC.corridor_counts(hyps, pts, sc["vox"], HC.LARGEST)
    assert (large >= small).all() and (largest >= large).all() and (large > small).any()


def test_faces_are_closed(oracle_hands):
    """a corridor whose face passes exactly through a point counts it; one ulp inwards does not"""
    sc, hyps, pts = oracle_hands[1]
    c = HC.corridor_counts(hyps, pts, sc["vox"], HC.DEFAULTS)
    i = HC.pick_small_count(c)
    one = hyps[i:i + 1]
    palm = HC.palm_points(one, pts[i:i + 1])
    xb, yb, zb = (v[0] for v in HC.body_coords(one, palm, sc["vox"]))
    j = int(np.flatnonzero(HC.in_corridor(xb, yb, zb, HC.params()))[0])
    assert yb[j] < 0.0 and xb[j] != 0.0 and zb[j] != 0.0
    wide = dict(near_offset=0.0, far_offset=0.5, half_width=0.25, half_height=0.25)
    for field, on, inwards in (("far_offset", -yb[j], np.nextafter(-yb[j], 0.0)), ("half_width", abs(xb[j]), np.nextafter(abs(xb[j]), 0.0)),
                               ("half_height", abs(zb[j]), np.nextafter(abs(zb[j]), 0.0)), ("near_offset", -yb[j], np.nextafter(-yb[j], 1.0))):
        assert HC.in_corridor(xb[j], yb[j], zb[j], dict(wide, **{field: float(on)})), field
        assert not HC.in_corridor(xb[j], yb[j], zb[j], dict(wide, **{field: float(inwards)})), field


def test_a_nan_record_counts_nothing(oracle_hands):
    sc, hyps, pts = oracle_hands[2]
    assert HC.drop(hyps, pts, sc["vox"], HC.BODY).sum() >= 5
    for field in ("approach", "binormal", "axis", "bottom"):
        h = hyps.copy()
        h[field][:] = np.nan
        assert not HC.corridor_counts(h, pts, sc["vox"], HC.LARGEST).any(), field


def test_hands_the_hand_filter_dropped_are_not_counted(oracle_hands):
    sc, hyps, pts = oracle_hands[2]
    fp = HF.scene_filters(sc)["all"]
    reason = HF.drop_reasons(hyps, pts, fp, sc["images"])
    alone = HC.drop(hyps, pts, sc["vox"], HC.DEFAULTS)
    behind = HC.drop(hyps, pts, sc["vox"], HC.DEFAULTS, reason)
    assert (alone & (reason != 0)).sum() >= 1  # (some hands fail both: they count under the hand filter only)
    assert np.array_equal(behind, alone & (reason == 0)) and behind.sum() >= 1
    c = HC.counts(behind, reason)
    assert c[0] == HF.counts(reason)[4] and c[0] == c[1] + c[2] and c[2] >= 1
    assert HC.counts(alone) == [len(hyps), int(alone.sum()), int((~alone).sum())]
