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
    assert _straddles(seeds, 64) and _straddles(seeds, 2048)  # one wave's row (k_handle_batch declines beyond)
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
