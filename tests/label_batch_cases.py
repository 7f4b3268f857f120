"""Batches of captures with label arrays for the agh_localize_batch_labeled* tests (numpy only), built from the single-capture
cases of tests/label_cases.py.

A batch is a list of (name, case) pairs, a case as tests/label_cases.py makes it; cell_size must be equal across a batch, so
the 1 cm cases and the 3 mm cases go into batches of their own, and every batch holds at most 64 lists (a list per object of a
capture).  Each batch is named after the regime tests/test_label_batch_cases.py proves it is in.

  point_batches    name -> batch; SEQUENCES names the batches that run one after the other on ONE context
  first_lists      capture k's first list among the batch's (the exclusive prefix sum of n_objects)
  point_model      ([E_{k,0} ..], voxel model) of one capture alone: what the batch must give for it
  n_samples / seed S_k and seed_k the GPU test draws with
"""
import numpy as np

from tests import label_cases as L
from tests import mask_batch_cases as MB

CM, MM = 0.01, 0.003
MAX_LISTS = 64

# the batches that run one after the other on one context: the first one's lattices size the kept bitmap slots
SEQUENCES = {"dense_after_small": ("cm_small", "cm")}

# the 1 cm batch: a one-object capture first, all_dropped in the middle, the row, word-edge and block-edge cases behind captures
# that have voxels and lists; the reversed batch starts with dup_voxel
CM_ORDER = ("k1", "row_63", "word_edge", "row_1025", "block_edge", "dense_block", "two_cameras_same_lattice", "all_dropped",
            "dropped", "rank_cameras", "row_64", "row_1024", "row_65", "dup_voxel")
LARGE_LATTICES = ("dense_block", "block_edge", "two_cameras_same_lattice")


def _named_cases() -> dict:
    cases = dict(L.point_cases())
    # k64's capture with 60 objects: the labels 61 .. 64 are above n_objects and belong to none
    cases["k64_as_60"] = dict(cases["k64"], n_objects=60)
    return cases


def point_batches() -> dict:
    cases = _named_cases()
    orders = {
        "cm": list(CM_ORDER),
        "cm_small": [n for n in CM_ORDER if n not in LARGE_LATTICES],
        "k64": ["k64"],  # 64 lists from one capture
        "full64": ["k1", "k64_as_60", "dropped"],  # exactly 64 lists over several captures, a 1-object one beside a 60-object one
        "mm": ["stride32", "values"],
    }
    for name in ("cm", "cm_small", "full64", "mm"):  # (k64 has one capture: its reverse is itself)
        orders[name + "_reversed"] = orders[name][::-1]
    batches = {name: [(n, cases[n]) for n in order] for name, order in orders.items()}
    for name, batch in batches.items():
        assert len({c["cell"] for _, c in batch}) == 1 and sum(c["n_objects"] for _, c in batch) <= MAX_LISTS, name
    return batches


def first_lists(batch) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([c["n_objects"] for _, c in batch])]).astype(np.int64)


def point_counts(batch) -> list:
    return [len(c["points"]) for _, c in batch]


def point_model(c):
    cams = L.cams_of(c)
    return L.eligible_lists(c, cams), MB.voxels_or_none(c["points"], cams, c["workspace"], c["cell"])


def n_samples(name: str, ms) -> int:
    """S of a capture whose lists hold ms voxels: around the counts (the largest list + 2: every list is shorter than S, some
    by 1 or 2; at most 24: the long lists hold 2 S and more)"""
    return 200 if name == "dense_block" else min(max(ms) + 2, 24)


def seed(k: int) -> int:
    return 11 + k
