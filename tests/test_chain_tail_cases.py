"""The sample lists of tests/chain_tail_cases.py sit on the edges they name.

CPU only.  The table's promise -- the hands of a multiset of samples are the table's, repeated -- is checked against the oracle's
search of one such list; then every case's K, S and longest row are counted on the hands themselves (capacity_clouds.seed_inliers,
not the table's shortcut), and the thresholds they straddle are read out of the sources.
"""
import os
import re

import numpy as np
import pytest

from tests import capacity_clouds as cc
from tests import chain_tail_cases as tc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "agile_grasp_amd", "csrc")


@pytest.fixture(scope="module")
def table():
    return tc.build_table()


@pytest.fixture(scope="module")
def cases(table):
    return tc.single_cases(table)


def _longest_row(h):
    return max(cc.seed_inliers(h, i) for i in range(len(h)))


def test_the_edges_are_where_the_sources_put_them():
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    assert re.search(r"constexpr int kHandleLdsHands = 640;", src("handles.hip"))
    assert re.search(r"constexpr int kHandleMaxHands = 8192;", src("handles.hip"))
    assert re.search(r"constexpr int kHandleListCap = 2048;", src("handles.hip"))
    assert re.search(r"constexpr int kMaxRow = 128,", src("handles.hip"))
    assert re.search(r"dim3\(d_H \? std::min\(Hi, 1024\) : Hi, L\)", src("handles.hip"))  # k_handle_build's bounded grid
    assert re.search(r"for \(int64_t b0 = r0; b0 < r1; b0 \+= 1024\)", src("agh_internal.h"))  # compact_kept_records' blocks
    assert re.search(r"hand_bound = std::min<int64_t>\(8 \* L\.S, 8192\)", src("localize.hip"))


def test_a_multiset_of_samples_makes_the_tables_hands(table):
    """Repeated and distinct samples through the oracle's search: the hypotheses are the table's, entry by entry."""
    from oracle import oracle_py as O

    t = table
    lst = np.sort(np.concatenate([tc.exact_list(t, 150), np.full(5, tc.lone_sample(t)[0])]))
    p = O.default_params(t.rc.cam_origins, num_threads=min(os.cpu_count() or 1, 16))
    v, cam = O.preprocess(t.rc.xyz, t.rc.size_left, t.rc.workspace)
    assert len(v) == t.n_voxels
    got = O.find_hands(p, v, cam, t.s[lst])["hyps"]
    want = tc.hands_of(t, lst)
    assert len(got) == len(want) == 155
    for f in ("sample", "orientation", "axis", "approach", "binormal", "bottom", "surface", "width"):
        assert np.array_equal(got[f], want[f]), f


def test_single_cases_hit_their_counts(table, cases):
    t = table
    print("table: samples", len(t.s), "hypotheses", len(t.hyps), "per sample", np.bincount(t.y).tolist())
    for name, c in cases.items():
        lst = c["lst"]
        h = tc.hands_of(t, lst)
        S = len(lst)
        assert (np.diff(lst) >= 0).all() and len(h) == c["K"] <= 8 * S, name
        shortcut = int(tc.rows_of(t, lst).max())
        row = _longest_row(h) if len(h) <= 3000 else shortcut  # (the large lists: from the table's matrix)
        print(name, "S", S, "K", len(h), "longest row", row)
        assert row == shortcut, name
        if c["row"] == "<=128":
            assert row <= 128, name
        elif c["row"] is not None:
            assert row == c["row"], name
        else:
            assert row <= 2048, name
    K = {n: c["K"] for n, c in cases.items()}
    S = {n: len(c["lst"]) for n, c in cases.items()}
    assert K["K640"] == 640 and K["K641"] == 641 and 8 * S["K640"] > 640 and 8 * S["K641"] > 640  # both variants queued
    assert 8 * S["S80"] == 640 and K["S80"] == S["S80"] * t.y.max() and t.y.max() < 8  # only the small variant queued
    assert [K[f"N{n}"] for n in (1023, 1024, 1025)] == [1023, 1024, 1025]  # compact_kept_records' first block edge
    assert K["K8192"] == 8192 and K["K8193"] == 8193 and 8 * S["K8193"] > 8192
    assert K["R129small"] <= 640 < K["R129general"] and 8 * S["R129small"] > 640
    assert K["R128"] <= 640


def test_repeated_sample_is_a_row_of_its_own(table):
    """The hand of the repeated sample is an inlier of itself and of nothing else in its lists: r copies are a row of r."""
    t = table
    lst, j = tc.repeated_list(t, 129, 400)
    h = tc.hands_of(t, lst)
    mine = np.flatnonzero(lst == j)
    assert len(mine) == 129 and t.y[j] == 1
    idx = np.flatnonzero(np.isin(h["sample"], mine))
    assert len(idx) == 129 and all(cc.seed_inliers(h, i) == 129 for i in idx[[0, 64, 128]])
    others = np.setdiff1d(np.arange(len(h)), idx)
    assert max(cc.seed_inliers(h, i) for i in others) <= 64


def test_classify_list_is_more_than_two_scan_blocks(table):
    lst = tc.classify_list(table)
    assert len(tc.hands_of(table, lst)) > 2048


def test_batch_lists_hit_their_counts(table):
    t = table
    b = tc.batch_lists(t)
    for kind in ("mixed", "last", "plain"):
        rows = []
        for lst, K in zip(b[kind], b["K"][kind]):
            h = tc.hands_of(t, lst)
            assert len(h) == K and (np.diff(lst) >= 0).all()
            rows.append(_longest_row(h))
        print(kind, "K", b["K"][kind], "longest rows", rows)
        want_declined = [K == 329 for K in b["K"][kind]]
        assert [r > 128 for r in rows] == want_declined and all(r == 129 for r, d in zip(rows, want_declined) if d)
