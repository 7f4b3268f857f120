"""Sample lists that put the tail of the localize chains -- kept-hand compaction, handle search under a device-side count, the
handles-only requeue -- on its edges (tests/test_chain_tail_cases.py checks every list on the CPU, tests/test_gpu_chain_tail.py
runs them on the GPU).

Plain numpy and the oracle, no GPU.  One raw cloud; its voxels' hypotheses are tabulated once for a few thousand distinct
samples.  An explicit sample list may repeat an index (include/agh.h puts no uniqueness rule on sample_idx) and samples are
independent work items, so the table fixes the hands of ANY multiset of its samples: a sample with y hypotheses that is listed r
times yields r y hands, the r copies of each identical and inliers of each other.  With classify off every hypothesis is a kept
hand, so a list's K (kept hands, the handle search's H) and n_hypotheses are sums over the table, and the rows of its pair
matrix are sums over the table's pair matrix.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

RAW = dict(n_points=60_000, seed=7, n_objects=4)
N_TABLE = 6000  # distinct samples in the table (about 1700 hypotheses)


def raw_cloud():
    from agile_grasp_amd import synthetic

    return synthetic.make_raw_cloud(RAW["n_points"], RAW["seed"], n_objects=RAW["n_objects"])


def pair_matrix(h):
    """P[i, j]: hand j is a potential inlier of seed i (handle_search.cpp:19-28; tests/capacity_clouds.seed_inliers, all seeds
    at once)."""
    ax, bt, ap = h["axis"], h["bottom"], h["approach"]
    d = bt[None, :, :] - bt[:, None, :]  # [i, j] = bottom j - bottom i
    along = np.einsum("ijk,ik->ij", d, ax)
    v = d - along[:, :, None] * ax[:, None, :]
    dist = np.sqrt((v * v).sum(2))
    ang = np.arccos(np.clip(ax @ ax.T, -1, 1))
    nn = np.arccos(np.clip(ap @ ap.T, -1, 1))
    return (dist < 0.01) & (np.minimum(ang, np.pi - ang) < 0.34) & (nn < 0.34)


@dataclass
class Table:
    rc: object            # the raw capture
    n_voxels: int
    s: np.ndarray         # the table's samples: sorted distinct voxel indices
    hyps: np.ndarray      # the oracle's hypotheses of s (`sample`: position in s)
    y: np.ndarray         # hypotheses per sample
    first: np.ndarray     # offset of each sample's hypotheses in hyps
    P: np.ndarray         # pair_matrix(hyps)


def build_table():
    from oracle import oracle_py as O

    rc = raw_cloud()
    v, cam = O.preprocess(rc.xyz, rc.size_left, rc.workspace)
    s = np.sort(np.random.default_rng(1).permutation(len(v))[:N_TABLE]).astype(np.int32)
    p = O.default_params(rc.cam_origins, num_threads=min(os.cpu_count() or 1, 16))
    h = O.find_hands(p, v, cam, s)["hyps"]
    assert (np.diff(h["sample"]) >= 0).all()
    y = np.bincount(h["sample"], minlength=len(s))
    first = np.concatenate([[0], np.cumsum(y)[:-1]])
    return Table(rc, len(v), s, h, y, first, pair_matrix(h))


def hands_of(t, lst):
    """The hands the chain's search makes of the list `lst` (positions in t.s, sorted): every entry's hypotheses in list order,
    `sample` = the position in the list."""
    lst = np.asarray(lst)
    rows = np.concatenate([np.arange(t.first[j], t.first[j] + t.y[j]) for j in lst] + [np.zeros(0, np.int64)]).astype(np.int64)
    h = t.hyps[rows].copy()
    h["sample"] = np.repeat(np.arange(len(lst)), t.y[lst])
    return h


def rows_of(t, lst):
    """Length of every row of the pair matrix of hands_of(t, lst): from the table's matrix and the multiplicities."""
    lst = np.asarray(lst)
    mult = np.bincount(lst, minlength=len(t.s))
    per_hand = np.repeat(mult, t.y)  # multiplicity of each table hand
    full = t.P @ per_hand
    rows = np.concatenate([np.arange(t.first[j], t.first[j] + t.y[j]) for j in lst] + [np.zeros(0, np.int64)]).astype(np.int64)
    return full[rows]


def exact_list(t, K, reps=1, max_row=None, avoid=None, start=0, pad_to=0):
    """A sorted list of positions in t.s whose hypotheses number exactly K: the samples with hypotheses from `start` on, up to
    `reps` times each, none whose hands would make a row longer than max_row, none of `avoid`; then samples without hypotheses
    until the list has pad_to entries."""
    mult = np.zeros(len(t.s), np.int64)
    rowlen = np.zeros(len(t.hyps), np.int64)  # rows of the table hands, under mult
    used = np.zeros(len(t.hyps), bool)
    left = K
    banned = np.zeros(len(t.s), bool)
    if avoid is not None:
        banned[np.asarray(avoid)] = True
    for j in range(start, len(t.s)):
        if left == 0:
            break
        yj = int(t.y[j])
        if yj == 0 or banned[j]:
            continue
        m = min(reps, left // yj)
        if m == 0:
            continue
        hs = np.arange(t.first[j], t.first[j] + yj)
        if max_row is not None:
            new = rowlen + m * t.P[:, hs].sum(1)
            u = used.copy()
            u[hs] = True
            if new[u].max() > max_row:
                continue
            rowlen = new
            used = u
        mult[j] = m
        left -= m * yj
    assert left == 0, (K, left)
    lst = np.repeat(np.arange(len(t.s)), mult)
    if len(lst) < pad_to:
        empty = np.flatnonzero((t.y == 0) & ~banned)[:pad_to - len(lst)]
        assert len(lst) + len(empty) == pad_to
        lst = np.sort(np.concatenate([lst, empty]))
    return lst


def lone_sample(t):
    """A sample with one hypothesis whose hand is an inlier of itself (unit axis and approach pass the alignment test) and has few
    neighbours in the table: (position, positions of the samples whose hands share a row with it either way)."""
    best = None
    for j in np.flatnonzero(t.y == 1):
        a = t.first[j]
        if not t.P[a, a]:
            continue
        near = np.flatnonzero(t.P[a] | t.P[:, a])
        if best is None or len(near) < best[1]:
            best = (int(j), len(near), np.unique(t.hyps["sample"][near]))
    assert best is not None
    return best[0], best[2]


def repeated_list(t, r, K_others, max_row=64):
    """One sample r times -- r identical hands, a row of exactly r -- among samples that make K_others further hands, none of
    them in a row with the repeated one and no row of their own longer than max_row."""
    j, near = lone_sample(t)
    others = exact_list(t, K_others, max_row=max_row, avoid=near)
    return np.sort(np.concatenate([others, np.full(r, j)])), j


# ---- the cases: name -> (list builder, what it must be on the CPU) ---------------------------------------------------------------
# K: kept hands = n_hypotheses (classify off); S: entries of the list; row: the longest row of the pair matrix (None: any, "<=128":
# not declined, ">128": declined)
def single_cases(t):
    c = {}
    c["K640"] = dict(lst=exact_list(t, 640, max_row=128, pad_to=700), K=640, row="<=128")
    c["K641"] = dict(lst=exact_list(t, 641, max_row=128, pad_to=700), K=641, row="<=128")
    # only the small variant queued: 8 S <= 640.  No sample of this cloud has eight hypotheses (the most is three), so K = 640
    # cannot meet S = 80; the exact fit is S = 80 entries of three hands each
    three = np.flatnonzero(t.y == t.y.max())[:4]
    c["S80"] = dict(lst=np.sort(np.repeat(three, 20)), K=80 * int(t.y.max()), row="<=128")
    for n in (1023, 1024, 1025):
        c[f"N{n}"] = dict(lst=exact_list(t, n, max_row=128), K=n, row="<=128")
    c["K8192"] = dict(lst=exact_list(t, 8192, reps=6), K=8192, row=None)
    c["K8193"] = dict(lst=exact_list(t, 8193, reps=6), K=8193, row=None)
    c["R129small"] = dict(lst=repeated_list(t, 129, 400)[0], K=529, row=129)
    c["R129general"] = dict(lst=repeated_list(t, 129, 600)[0], K=729, row=129)
    c["R128"] = dict(lst=repeated_list(t, 128, 400)[0], K=528, row=128)
    c["R2049"] = dict(lst=repeated_list(t, 2049, 200)[0], K=2249, row=2049)
    return c


def classify_list(t):
    """Every sample with hypotheses twice: more than 2048 hypotheses, of which the classifier keeps some."""
    return np.repeat(np.flatnonzero(t.y > 0), 2)


def batch_lists(t):
    """[K = 300 plain, one sample x 129 plus 200 other hands, K = 700 plain] and three plain lists."""
    plain300 = exact_list(t, 300, max_row=128)
    declining = repeated_list(t, 129, 200)[0]
    plain700 = exact_list(t, 700, max_row=128, start=len(t.s) // 4)
    plain500 = exact_list(t, 500, max_row=128, start=len(t.s) // 8)
    return dict(mixed=[plain300, declining, plain700], last=[plain700, plain300, declining],
                plain=[plain300, plain500, plain700], K=dict(mixed=[300, 329, 700], last=[700, 300, 329], plain=[300, 500, 700]))
