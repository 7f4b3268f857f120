"""The hand geometries of tests/hand_geometries.py are what their names say, and the clouds chosen for them make the oracle
use the tables they shape from end to end.

CPU only.  `derive` (a restatement of build_geometry) must reproduce every property of the table, the formulas it restates
are read out of the sources, and the oracle must give each accepted geometry enough hypotheses, at the first and the last
bite depth, with antipodal labels -- so that a geometry or a cloud that stops exercising its instantiation of k_hand_sweep
fails here before any GPU time is spent.
"""
import os
import re

import numpy as np
import pytest

from tests import hand_geometries as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "agile_grasp_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(hg.TABLE))
def test_the_restatement_reproduces_the_table(name):
    g, want = hg.TABLE[name]
    got = hg.derive(g)
    print(name, got)
    for k, v in want.items():
        assert got[k] == v, (name, k, got[k], v)


def test_the_table_covers_every_probe_count_and_both_ends_of_the_depth_table():
    d = {k: hg.derive(g) for k, (g, _) in hg.TABLE.items()}
    assert {d[k]["x_probes"] for k in hg.ACCEPTED} == {1, 2, 3, 4}
    assert {1, 2, hg.MAX_DEPTHS} <= {d[k]["n_depths"] for k in hg.ACCEPTED}
    assert d["one_depth"]["ylut_scale"] == 0.0  # a one-entry table: every depth falls into cell 0
    assert {d[k]["refused"] for k in hg.REFUSED} == {"depths", "cell"}
    # the instantiations: <.., 2, 1> for the `few` geometries, <.., kLutProbe, kLutProbe> for the others
    assert set(hg.GENERAL) == {"three_a", "three_b", "four"}
    assert all(d[k]["few"] for k in ("default", "one_per_cell", "one_depth", "two_depths", "sixteen_depths"))
    # bite depths lie 5 mm apart and at most 16 are accepted: no depth table ever puts two into one of its 64 cells, so
    # the second to fourth depth compares of the kLutProbe instantiations cannot decide anything for an accepted geometry
    assert all(hg.derive(dict(init_bite=0.005, hand_depth=0.005 + 0.005 * k))["y_probes"] == 1 for k in range(16))
    # one step less, or a finger a hair narrower, and the refused geometries are accepted
    assert hg.derive(dict(init_bite=0.005, hand_depth=0.08))["refused"] is None
    assert hg.derive(dict(finger_width=0.09975, hand_outer_diameter=0.1))["x_probes"] == 4
    assert hg.derive(dict(finger_width=0.0899, hand_outer_diameter=0.09))["refused"] == "cell"
    # capacity_clouds.PROBE4 is three_a: three thresholds in its fullest cell, not four
    from tests import capacity_clouds as cc

    assert cc.PROBE4 == hg.geom("three_a") and d["three_a"]["x_probes"] == 3


def test_the_restatement_is_tied_to_the_sources():
    api, hdr, sweep = _src("api.hip"), _src("agh_internal.h"), _src("hand_sweep.hip")
    assert int(re.search(r"constexpr int kLutProbe = (\d+);", hdr).group(1)) == hg.LUT_PROBE
    assert re.search(r"cell\[k\] = \(int\) std::fmin\(std::fmax\(\(tab\[k\] - lo\) \* scale, 0\.0\), \(double\) \(ncell - 1\)\);", api)
    assert re.search(r"const double scale = \(hi > lo\) \? \(double\) ncell / \(hi - lo\) : 0\.0;", api)
    assert re.search(r"if \(inside > kLutProbe\)\s*return false;", api)
    m = re.search(r"build_lut\(g->thr, g->n_thr, (\d+),.*\n.*build_lut\(g->depths, g->n_depths, (\d+),", api)
    assert (int(m.group(1)), int(m.group(2))) == (hg.X_CELLS, hg.Y_CELLS)
    assert re.search(r"for \(double d = p\.init_bite \+ 0\.005; d <= p\.hand_depth; d \+= 0\.005\)", api)
    assert int(re.search(r"if \(k >= (\d+)\)\s*\{\s*\*err = \"more than 15 deepening steps", api).group(1)) == hg.MAX_DEPTHS
    assert re.search(r"const double fstep = \(high - low\) / 9\.0;", api)
    assert re.search(r"g->fs\[i\] = \(h - p\.hand_outer_diameter\) \+ p\.finger_width;", api)
    assert re.search(r"t\.push_back\(g->fs\[i\] \+ p\.finger_width\);", api)
    assert re.search(r"const bool few = c->geom\.x_probes <= 2 && c->geom\.y_probes <= 1;", sweep)
    assert re.search(r"double depths\[(\d+)\]", hdr).group(1) == str(hg.MAX_DEPTHS)


def test_the_clouds_are_what_the_table_says():
    for name, lo, hi in (("rod", 1300, 1500), ("plate", 4200, 4400), ("sheets", 6400, 6600)):
        xyz, cam, s = hg.cloud(name)
        print(name, len(xyz), len(s))
        assert lo < len(xyz) < hi and xyz.dtype == np.float32
        assert len(s) == hg.N_SAMPLES == len(set(s.tolist())) and (np.diff(s) > 0).all() and s.max() < len(xyz)
        assert cam.tolist() == [k % 2 for k in range(len(xyz))]
        again = hg.cloud(name)
        assert all(np.array_equal(a, b) for a, b in zip(again, (xyz, cam, s)))
    assert set(hg.CLOUDS) == set(hg.ACCEPTED) and all("rod" in c for c in hg.CLOUDS.values())


@pytest.mark.parametrize("name", [k for k in hg.ACCEPTED if k not in hg.EMPTY])
def test_the_oracle_uses_the_whole_depth_table_and_labels_hands(name):
    """Per cloud at least 20 hypotheses and half-antipodal hands; over the geometry's clouds depth_index takes both 0 and
    n_depths - 1 (the deepening's exit by exhaustion of the table); fully antipodal hands on the rod."""
    n_depths = hg.derive(hg.geom(name))["n_depths"]
    seen = set()
    for cl in hg.CLOUDS[name]:
        plain = hg.reference(name, cl, "plain")["hyps"]
        anti = hg.reference(name, cl, "antipodal")["hyps"]
        print(name, cl, len(plain), "depth_index", np.bincount(plain["depth_index"], minlength=n_depths).tolist(), "finger_index",
              sorted(set(plain["finger_index"].tolist())), "half", int(anti["half_antipodal"].sum()), "full",
              int(anti["full_antipodal"].sum()))
        assert len(plain) >= 20 and len(anti) == len(plain)
        assert anti["half_antipodal"].any()
        if cl == "rod":
            assert anti["full_antipodal"].any()
        assert plain["depth_index"].max() < n_depths
        seen |= set(plain["depth_index"].tolist())
    assert 0 in seen and n_depths - 1 in seen, sorted(seen)


def test_the_sheets_leave_a_finger_to_the_third_compare_of_a_cell():
    """What hg.sheets promises, from the oracle's frames: at orientations 0 and 4 the oracle picks hand 2, and every point in
    the slot of finger 9 (there is one at least) falls into the look-up cell that holds three_a's three thresholds next to
    zero, above all three -- ranked right only by a sweep that makes the third compare -- while a point beyond the slot
    exists, so that the slot alone decides the finger.  (On tiny, the rod and the plate a sweep that compares twice per cell
    returns the oracle's hands all the same: other points of the slot cover for the misranked ones.)"""
    from tests.capacity_clouds import flann_d2

    g = hg.params(hg.geom("three_a"))
    fs, t = hg.thresholds(g["finger_width"], g["hand_outer_diameter"])
    cell_of, scale = hg.cells(t, hg.X_CELLS)
    full = int(np.bincount(cell_of).argmax())
    assert np.bincount(cell_of)[full] == 3 and fs[9] == t[cell_of == full].max() and 0.0 in t[cell_of == full]
    xyz, cam, s = hg.cloud("sheets")
    ref = hg.reference("three_a", "sheets", "plain")
    hyps, fr = ref["hyps"], ref["frames"]
    along = hyps[(hyps["orientation"] == 0) | (hyps["orientation"] == 4)]
    print("hypotheses along the sheets", len(along), "finger_index", sorted(set(along["finger_index"].tolist())))
    assert len(along) >= 20 and (along["finger_index"] == 2).all()
    for h in along:
        k, ang = h["sample"], -np.pi + h["orientation"] * (2 * np.pi / 8)
        q = xyz[s[k]]
        d = (xyz - q).astype(np.float64)
        nxa = np.cross(fr["normal"][k], fr["axis"][k])
        tx, ty, tz = d @ fr["normal"][k], d @ nxa, d @ fr["axis"][k]
        crop = (flann_d2(xyz, q) < np.float32(0.08 * 0.08)) & (np.abs(tz) < g["hand_height"])
        xr, yr = np.cos(ang) * tx - np.sin(ang) * ty, np.sin(ang) * tx + np.cos(ang) * ty
        crop &= yr < g["init_bite"]
        slot = crop & (xr > fs[9]) & (xr < fs[9] + g["finger_width"])
        cells = np.minimum(np.maximum((xr[slot] - t[0]) * scale, 0.0), hg.X_CELLS - 1).astype(int)
        assert slot.sum() >= 1 and (cells == full).all(), (k, slot.sum(), xr[slot].max())
        assert (crop & (xr > fs[9] + g["finger_width"])).any()


def test_only_the_four_per_cell_geometry_gives_the_oracle_no_hands():
    """finger_width 0.0898 of hand_outer_diameter 0.09: the two fingers of a hand overlap, and every slot spans 9 cm next to
    the sample, which lies at x = 0 of its own hand frame.  Only hand 9 has slots that spare x = 0, and its left finger
    then needs a point beyond x = 0.0898 + 0.0002 -- farther than nn_radius_hands = 0.08 reaches.  So the oracle finds no
    hand with it on any cloud, tiny, the rod and the plate included, and the compare of the fourth probe stays unobserved
    by results: the GPU runs the geometry all the same and must return nothing too.  It is the only such geometry."""
    assert hg.EMPTY == ("four",)
    for cl in hg.CLOUDS["four"]:
        for mode in ("plain", "antipodal"):
            assert len(hg.reference("four", cl, mode)["hyps"]) == 0
    assert hg.derive(hg.geom("four"))["x_probes"] == hg.LUT_PROBE


def test_the_training_reference_labels_like_the_antipodal_one():
    """find_hands_training is find_hands(calculates_antipodal) plus the instance images: three per hypothesis."""
    for name, cl in (("three_a", "rod"), ("one_depth", "rod")):
        tr, anti = hg.reference(name, cl, "training"), hg.reference(name, cl, "antipodal")
        assert tr["hyps"].tobytes() == anti["hyps"].tobytes()
        assert tr["images"].shape == (len(anti["hyps"]), 3, 8000) and np.array_equal(tr["images"][:, 0], anti["images"])


def test_the_padded_sample_list_keeps_tinys_hands_and_the_sheets_decisive_ones():
    xyz, cam, s, n_tiny, n_own = hg.padded_tiny()
    from agile_grasp_amd import synthetic

    sc = synthetic.config("tiny")
    assert len(s) == hg.PADDED_SAMPLES > 4096 and np.array_equal(s[:n_tiny], sc.samples) and np.array_equal(xyz[:sc.n], sc.xyz)
    assert n_own == n_tiny + hg.N_SAMPLES and len(set(s.tolist())) == len(s)
    own = xyz[s[:n_own]].astype(np.float64)
    d = xyz[s[n_own]:, None, :].astype(np.float64) - own[None]
    assert np.sqrt((d * d).sum(2)).min() > 0.08 + 0.03 + 0.1  # the padding lies beyond every ball of the other samples
    d = own[:n_tiny, None, :] - own[None, n_tiny:]
    assert np.sqrt((d * d).sum(2)).min() > 2 * 0.08 + 0.2  # (tiny and the sheets: no ball of one reaches a point of the other)
    from oracle import oracle_py as O

    p = O.default_params(hg.cam_origins(), num_threads=min(os.cpu_count() or 1, 16), **hg.geom("three_a"))
    ref = O.find_hands(p, xyz, cam, s[:n_own + 64])["hyps"]
    a = ref[ref["sample"] < n_tiny]
    assert a.tobytes() == hg.reference("three_a", "tiny", "plain")["hyps"].tobytes()
    b = ref[(ref["sample"] >= n_tiny) & (ref["sample"] < n_own)]
    along = b[(b["orientation"] == 0) | (b["orientation"] == 4)]
    print("sheets beside tiny: hypotheses", len(b), "along the sheets", len(along), "padding's first 64 samples",
          int((ref["sample"] >= n_own).sum()))
    assert len(along) >= 20 and (along["finger_index"] == 2).all()  # (as where test_the_sheets_... examines them)
    assert (ref["sample"] >= n_own).any()  # the padding is searchable surface, not idle samples
