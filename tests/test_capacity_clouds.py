"""The capacity-edge inputs (tests/capacity_clouds.py) hit their targets, and the targets sit on the kernels' thresholds.

CPU only.  Every generated case is checked against the oracle (n_nb, handle inlier counts) or the numpy crop count, so a
mistargeted case fails here before any GPU time is spent.  The threshold table reads each boundary out of the .hip / .h
text: if a threshold moves, the test names the case that must move with it.
"""
import os
import re

import numpy as np
import pytest

from tests import capacity_clouds as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "agile_grasp_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _straddles(cases, b):
    return b in cases and b + 1 in cases


# (boundary name, file, regex, expected groups, the cases that must straddle each value (b and b + 1 both present))
THRESHOLDS = [
    ("K1a first class (n > CAP hands on)", "taubin.hip", r"k_taubin_moments<(\d+)>, dim3\(Si\)", ("256",), cc.TAUBIN_DET),
    ("K1a hand-on test", "taubin.hip", r"const int n = count;\s*if \(n (>) CAP\)", (">",), None),
    ("K1a/K1c 1152 class", "taubin.hip", r"AGH_LAUNCH_FRAME\((\d+), 256, 0\);\s*if \(c->big_classes && c->d_ovf\)", ("1152",),
     cc.TAUBIN_DET),
    ("K1c 4096 class (list walk)", "taubin.hip", r"AGH_LAUNCH_FRAME_L\((\d+), 256, (\d+),", ("4096", "1152"), cc.TAUBIN_DET),
    ("K1c 6144 class", "agh_internal.h", r"constexpr int kHugeCap = (\d+);", ("6144",), cc.TAUBIN_DET),
    ("K1c huge class launch", "taubin.hip", r"AGH_LAUNCH_FRAME\(kHugeCap, 256, (\d+)\)", ("4096",), cc.TAUBIN_DET),
    ("K1c ownership nmin < n <= CAP", "taubin.hip", r"ks_class (<=) nmin \|\| ks_class (>) CAP", ("<=", ">"), None),
    ("K1c all-points class", "taubin.hip", r"AGH_LAUNCH_FRAME\((\d+), 64, 0\)", ("128",), cc.ALLPOINTS),
    ("K1c all-points second class", "taubin.hip", r"AGH_LAUNCH_FRAME\((\d+), 256, (\d+)\);\s*else", ("1152", "128"),
     cc.ALLPOINTS),
    ("K1a all-points first class", "taubin.hip", r"k_taubin_moments<(\d+)>, dim3\(Si\)", ("256",), cc.ALLPOINTS),
    ("K1c RAND50 class", "taubin.hip", r"AGH_LAUNCH_FRAME\((\d+), 256, 0\);\s*\}", ("64",), cc.RAND50_EDGE[:2] + (64, 65)),
    ("RAND50 draws only for n > 50", "taubin.hip", r"nt\[i0 \+ u\] > (\d+)\) \? (\d+) : 0", ("50", "50"), cc.RAND50_EDGE),
    ("RAND50 normals room", "taubin.hip", r"ks_class = \(rand_mode && n > (\d+)\) \? (\d+) : n", ("50", "50"),
     cc.RAND50_EDGE),
    ("eigen lanes per sample", "taubin.hip", r"#define AGH_LPS8_MAX (\d+)", ("4096",), cc.SAMPLE_COUNTS),
    ("scheduling orders", "taubin.hip", r"constexpr int kOrderMaxSamples = (\d+);", ("4096",), cc.SAMPLE_COUNTS),
    ("sweep block order needs S >= 4 * kSweepBlock", "taubin.hip", r"constexpr int kSweepBlock = (\d+),", ("32",),
     None),  # (S = 127 / 128: see test_derived_boundaries_are_straddled)
    ("sweep WG4 beyond", "agh_internal.h", r"constexpr int kSweepWg4MinSamples = (\d+);", ("4096",), cc.SAMPLE_COUNTS),
    ("sweep tiles", "hand_sweep.hip",
     r"kTile = TRAIN \? (\d+) : \(NORMALS \? (\d+) : \(NT == 512 \? \d+ : \(WG4 \? (\d+) : AGH_SWEEP_TILE\)\)\);",
     (str(cc.TILES["train"]), str(cc.TILES["normals"]), str(cc.TILES["wg4"])), None),
    ("sweep default tile", "hand_sweep.hip", r"#define AGH_SWEEP_TILE (\d+)", (str(cc.TILES["default"]),), None),
    ("sweep tile overflow test", "hand_sweep.hip", r"if \(base \+ cnt (>) kTile\)", (">",), None),
    ("compaction: fused", "hand_sweep.hip", r"if \(S <= (\d+)\)\s*hipLaunchKernelGGL\(k_compact_fused", ("4096",),
     cc.SAMPLE_COUNTS),
    ("compaction: offsets + copy", "hand_sweep.hip", r"else if \(S <= (\d+)\)\s*\{\s*hipLaunchKernelGGL\(k_compact_offsets",
     ("65536",), cc.SAMPLE_COUNTS),
    ("compaction: k_compact_top chunks", "hand_sweep.hip", r"for \(int b0 = 0; b0 < nb; b0 \+= (\d+)\)", ("256",), None),
    ("pinned mirror", "api.hip", r"constexpr int64_t kMirrorMaxRecords = 1 << (\d+);", ("16",), None),
    ("all-points chunk", "agh_internal.h", r"constexpr int64_t kNormalsChunk = (\d+);", ("16384",), None),
    ("handle search: LDS variant", "handles.hip", r"constexpr int kHandleLdsHands = (\d+);", ("640",), cc.HANDLE_COUNTS),
    ("handle search: inliers of a seed", "handles.hip", r"constexpr int kHandleListCap = (\d+);", ("2048",), None),
    ("handle search: at most hands", "handles.hip", r"constexpr int kHandleMaxHands = (\d+);", ("8192",), None),
    ("handle search: one-word-per-lane scan", "handles.hip", r"if \(W <= (\d+)\)", ("16",), None),
    ("handle search: two-half walk", "handles.hip", r"half < \(W > (\d+) \? 2 : 1\)", ("64",), None),
    ("handle search: longest row of the batched walk", "handles.hip", r"constexpr int kMaxRow = (\d+)", ("128",),
     tuple(k for _, k in cc.HANDLE_ROWS)),
    ("handle search: one slot per lane", "handles.hip", r"if \(s_maxrow <= (\d+)\)", ("64",),
     tuple(k for _, k in cc.HANDLE_SEEDS)),
    ("handle search: the batched walk declines", "handles.hip", r"if \(s_maxrow (>) kMaxRow\)", (">",), None),
]


@pytest.mark.parametrize("row", THRESHOLDS, ids=[t[0] for t in THRESHOLDS])
def test_threshold_table_matches_the_sources(row):
    name, fname, pat, want, cases = row
    m = re.search(pat, _src(fname))
    assert m, f"{name}: pattern not found in {fname} -- the code moved; re-derive the cases of tests/capacity_clouds.py"
    assert m.groups() == want, f"{name}: {fname} now says {m.groups()}, the cases were built for {want}"
    if cases is not None:
        b = int(want[0])
        assert _straddles(cases, b), f"{name}: the cases {cases} no longer straddle {b}"


def test_derived_boundaries_are_straddled():
    """The boundaries that are expressions of the constants above."""
    assert _straddles(cc.SAMPLE_COUNTS, 4 * 32 - 1)  # S >= 4 * kSweepBlock: 127 / 128
    assert _straddles(cc.SAMPLE_COUNTS, 65536) and _straddles(cc.MIRROR_COUNTS, 1 << 16)
    assert 8 * 65537 // 1024 + 1 > 256  # the largest S makes k_compact_top carry across 256-entry chunks
    assert _straddles(cc.ALLPOINTS_SIZES, 16384)
    for H in (640, 1024, 4096):  # W <= 16 (H <= 1024), W > 64 (H > 4096)
        assert _straddles(cc.HANDLE_COUNTS, H)
    assert max(cc.HANDLE_COUNTS) == 8192
    seeds = [k for _, k in cc.HANDLE_SEEDS]
    # one wave's row (beyond it k_handle_batch takes two members per lane), kHandleListCap, and kMaxRow = two waves' worth
    # (k_handle_batch declines beyond) in both LDS variants
    assert _straddles(seeds, 64) and _straddles(seeds, 2048)
    for H in (600, 1500):
        assert _straddles([k for h, k in cc.HANDLE_ROWS if h == H], 128) and _straddles([k for h, k in cc.HANDLE_SEEDS if h == H], 64)
    assert max(h for h, _ in cc.HANDLE_ROWS if h <= 640) <= 640 < min(h for h, _ in cc.HANDLE_ROWS if h > 640)
    for T in cc.TILES.values():
        assert cc.tile_targets(T) == (T - 1, T, T + 1, 2 * T, 2 * T + 1)


def _n_nb(xyz, cam, s, r):
    from oracle import oracle_py as O

    return O.fit_frames(cc._params({}), xyz, cam, s, r)["n_nb"]


def test_taubin_class_cloud_hits_its_counts():
    xyz, cam, s = cc.ball_cloud(cc.TAUBIN_DET, 0.03, seed=1, filler=500)
    n = _n_nb(xyz, cam, s, 0.03)
    print("n_nb", n.tolist())
    assert n.tolist() == list(cc.TAUBIN_DET)


def test_rand50_cloud_hits_its_counts():
    xyz, cam, s = cc.rand50_cloud()
    n = _n_nb(xyz, cam, s, 0.03)
    print("n_nb", n.tolist())
    assert n[:len(cc.RAND50_EDGE)].tolist() == list(cc.RAND50_EDGE)
    assert (n[len(cc.RAND50_EDGE):] > 50).all()


@pytest.mark.parametrize("total", cc.ALLPOINTS_SIZES)
def test_all_points_cloud_hits_its_counts(total):
    xyz, cam, s = cc.ball_cloud(cc.ALLPOINTS, 0.01, seed=2, total=total)
    n = _n_nb(xyz, cam, s, 0.01)
    print(len(xyz), "n_nb(r = 0.01)", n.tolist())
    assert len(xyz) == total and n.tolist() == list(cc.ALLPOINTS)


@pytest.mark.parametrize("kind", sorted(cc.TILES))
def test_tile_cloud_hits_its_crop_counts(kind):
    from oracle import oracle_py as O

    xyz, cam, s, geom, fr = cc.tile_cloud(kind)
    k = len(cc.tile_targets(cc.TILES[kind]))
    g = {**cc.HAND_DEFAULTS, **geom}
    ref = O.find_hands(cc._params(geom), xyz, cam, s[:k])
    rf = ref["frames"]
    assert np.array_equal(rf["axis"], fr["axis"]) and np.array_equal(rf["normal"], fr["normal"])  # the added points left the frame alone
    crop = [cc.crop_count(xyz, xyz[s[j]], rf["axis"][j], g["nn_radius_hands"], g["hand_height"]) for j in range(k)]
    print(kind, "crop", crop, "hypotheses", len(ref["hyps"]))
    assert crop == list(cc.tile_targets(cc.TILES[kind]))
    # the crop matters: some hypothesis of every sample has more points in its closing region than the patch holds
    for j in range(k):
        assert (ref["hyps"]["n_in_box"][ref["hyps"]["sample"] == j] > 400).any(), j
    if kind == "wg4":
        assert len(s) > 4096


def test_handle_cases_hit_their_counts():
    from oracle import oracle_py as O

    for H in cc.HANDLE_COUNTS:
        hands = cc.handle_hands(H, 0, seed=H)
        hd, _ = O.find_handles(hands, 3, 0.005)
        assert len(hands) == H and len(hd) > H // 40, H
        assert max(cc.seed_inliers(hands, i) for i in range(0, H, max(H // 200, 1))) <= 64
    for H, big in cc.HANDLE_SEEDS:
        hands = cc.handle_hands(H, big, seed=H + big)
        hd, _ = O.find_handles(hands, 3, 0.005)
        print(H, big, "largest handle", int(hd["n_inliers"].max()))
        assert len(hands) == H and int(hd["n_inliers"].max()) == big
        members = np.flatnonzero(cc.big_members(hands))
        assert len(members) == big and cc.seed_inliers(hands, members[0]) == big


def _rows(hands):
    return [cc.seed_inliers(hands, i) for i in range(len(hands))]


@pytest.mark.parametrize("H,big", cc.HANDLE_ROWS)
def test_handle_rows_hit_kmaxrow(H, big):
    """127 / 128 / 129 hands in the longest row of the pair matrix, with at most 640 hands and with more: no other row is
    longer, and the oracle finds the whole row as one handle."""
    from oracle import oracle_py as O

    hands = cc.handle_hands(H, big, seed=H + big)
    rows = _rows(hands)
    hd, _ = O.find_handles(hands, 3, 0.005)
    print(H, big, "longest rows", sorted(rows)[-3:], "largest handle", int(hd["n_inliers"].max()))
    assert len(hands) == H and max(rows) == big <= 2048
    assert rows[np.flatnonzero(cc.big_members(hands))[0]] == big and int(hd["n_inliers"].max()) == big


def test_handle_row_options_leave_the_defaults_alone():
    for H, big in cc.HANDLE_SEEDS[:4] + cc.HANDLE_ROWS:
        assert cc.handle_row_hands(H, big, seed=H + big).tobytes() == cc.handle_hands(H, big, seed=H + big).tobytes()


@pytest.mark.parametrize("case", cc.HANDLE_ROW_SHAPES, ids=cc.row_shape_id)
def test_handle_row_shapes_sit_on_their_edges(case):
    """Every shaped row: the longest row of the pair matrix is the big one (so the search takes k_handle_batch's two-slot
    evaluation and does not decline); a gap case is cut by its gap; a tie case has equal distances at sorted positions
    (63, 64), and a tied pair whose members sit in different slots of the UNSORTED member list (bit order: by index); a dead
    case has more than 64 potential members and fewer than 64 live ones."""
    from oracle import oracle_py as O

    H, big, opt = case
    hands = cc.row_shape_hands(case)
    rows = _rows(hands)
    first, members, dist = cc.big_row_sorted(hands)
    hd, idx = O.find_handles(hands, 3, 0.005)
    print(cc.row_shape_id(case), "longest rows", sorted(rows)[-3:], "handles", sorted(hd["n_inliers"].tolist())[-3:])
    assert len(hands) == H and len(members) == big and 64 < max(rows) == rows[first] == big <= 128
    if "gap_after" in opt:
        k = opt["gap_after"]
        assert dist[k + 1] - dist[k] > 0.02 + 1e-3 and (np.diff(dist)[:k] < 0.02 - 1e-3).all()
        lists = [idx[h["first_inlier"]:h["first_inlier"] + h["n_inliers"]] for h in hd]
        # the handle the row's first seed makes: the k hands before the gap, in order (the seed itself may lie beyond it)
        assert sum(len(l) == k and np.array_equal(l, members[:k]) for l in lists) == 1
    if "ties" in opt:
        assert dist[63] == dist[64] and members[63] < members[64]
        tied = np.flatnonzero(dist[1:] == dist[:-1])
        assert len(tied) == opt["ties"]
        slot = np.argsort(np.argsort(members)) // 64  # a member's slot in the unsorted list
        assert any(slot[p] != slot[p + 1] for p in tied)
        other = members[-1]  # equal along any other seed's axis too
        assert np.ptp(cc.along_seed(hands, other, members[63:65])) == 0.0
        assert int(hd["n_inliers"].max()) == big
    if "dead" in opt:
        live = int((hands["width"][members] != -1.0).sum())
        assert live == big - opt["dead"] and 3 <= live < 64 and hands["width"][first] != -1.0
        assert int(hd["n_inliers"].max()) == live
