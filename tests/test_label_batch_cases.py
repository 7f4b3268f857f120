"""The labelled batches (tests/label_batch_cases.py) reach the regimes the batched label stage can go wrong in, on the numpy
model alone.

CPU only.  tests/test_gpu_localize_batch_labeled.py holds the GPU to the model on these batches by exact equality; what is
asserted here is which lists are empty, where the seam cases lie in a batch (a non-zero first list and a non-zero offset in the
common voxel array), how many lists a batch holds, and that the sequence takes the kept-slot path.
"""
import functools

import numpy as np
import pytest

from tests import label_batch_cases as LB
from tests import label_cases as L
from tests.test_mask_batch_cases import WORDS_PER_BLOCK, _lattice_words


@functools.lru_cache(maxsize=None)
def _points():
    return LB.point_batches()


@functools.lru_cache(maxsize=None)
def _ms(name):
    """per capture of the batch: (name, [M_{k,0} ..], voxels)"""
    return [(n, [len(e) for e in LB.point_model(c)[0]], len(LB.point_model(c)[1][0])) for n, c in _points()[name]]


def _names(batch):
    return [n for n, _ in batch]


def test_the_batches_are_the_ones_the_gpu_test_names():
    b = _points()
    assert set(b) == {"cm", "cm_reversed", "cm_small", "cm_small_reversed", "k64", "full64", "full64_reversed", "mm", "mm_reversed"}
    assert set(LB.SEQUENCES) == {"dense_after_small"}
    assert len(b["k64"]) == 1  # (the only batch without a reversed twin: one capture)
    for name in ("cm", "cm_small", "full64", "mm"):
        assert _names(b[name + "_reversed"]) == _names(b[name])[::-1] and len(b[name]) > 1
    every = {n for n, c in L.point_cases().items()}
    used = {n for batch in b.values() for n, _ in batch}
    assert every <= used  # every single-capture case runs in some batch
    for name, batch in b.items():
        assert len({c["cell"] for _, c in batch}) == 1, name  # cell_size must be equal across a batch
        assert LB.first_lists(batch)[-1] <= LB.MAX_LISTS, name


@pytest.mark.parametrize("name", sorted(LB.point_batches()))
def test_each_capture_of_the_batch_gives_its_own_model(name):
    batch = _points()[name]
    first = LB.first_lists(batch)
    for k, (n, c) in enumerate(batch):
        E, vox = LB.point_model(c)
        assert len(E) == c["n_objects"] == first[k + 1] - first[k]
        want = L.eligible_lists(c)
        assert all(np.array_equal(a, b) for a, b in zip(E, want))
        for e in E:
            assert (np.diff(e) > 0).all() and (e < max(len(vox[0]), 1)).all()  # ascending capture-local voxel indices
        assert sum(len(e) for e in E) <= len(c["points"])  # a raw point adds at most one (voxel, object) pair


def test_the_numbers_of_lists():
    b = _points()
    assert len(b["k64"]) == 1 and LB.first_lists(b["k64"])[-1] == 64  # 64 lists from one capture
    for name in ("full64", "full64_reversed"):
        objects = [c["n_objects"] for _, c in b[name]]
        assert sum(objects) == 64 and len(objects) == 3 and 1 in objects and 60 in objects  # ... and over several, 1 beside 60
    # labels above n_objects belong to no object: the 60-object capture is k64's with its bytes 61 .. 64 ignored
    c = dict(b["full64"])["k64_as_60"]
    assert c["labels"].max() == 64 and [len(e) for e in LB.point_model(c)[0]] == [1] * 60
    assert LB.first_lists(b["cm"])[-1] == 31 and LB.first_lists(b["mm"])[-1] == 6
    objects = [c["n_objects"] for _, c in b["cm"]]
    assert objects[0] == 1 and max(objects) == 3


def test_the_empty_lists():
    for name in ("cm", "cm_reversed"):
        ms = _ms(name)
        names = [n for n, _, _ in ms]
        k = names.index("all_dropped")
        assert 0 < k < len(names) - 1 and ms[k][1] == [0, 0, 0]  # every M = 0, between captures that have samples
        assert any(m for m in ms[k - 1][1]) and any(m for m in ms[k + 1][1])
        assert ms[names.index("dropped")][1] == [1, 0, 1]  # an empty list between non-empty ones of ONE capture
    for name in ("full64", "full64_reversed"):
        assert dict((n, m) for n, m, _ in _ms(name))["dropped"] == [1, 0, 1]


def test_the_seams_lie_behind_other_captures():
    """the wave and work-group seams of count / emit (63, 64, 65, 1024, 1025 voxels in a row) and the word and block edges of
    the bitmap, each at a capture index >= 1 with voxels and lists in front: cloud_off and first_list are non-zero there"""
    for name in ("cm", "cm_reversed"):
        batch = _points()[name]
        ms = _ms(name)
        first = LB.first_lists(batch)
        voff = np.concatenate([[0], np.cumsum([v for _, _, v in ms])])
        names = _names(batch)
        for n in ["row_%d" % r for r in L.ROWS] + ["block_edge", "word_edge", "dense_block"]:
            k = names.index(n)
            assert k >= 1 and first[k] > 0 and voff[k] > 0, (name, n)
        for r in L.ROWS:
            k = names.index("row_%d" % r)
            assert ms[k][2] == r and ms[k][1] == [(r + 1) // 2, r // 2]
        assert {"two_cameras_same_lattice", "rank_cameras"} <= set(names)
        # offsets in the common voxel array that are no multiple of the 256-voxel work-group or the 64-lane wave
        assert any(voff[k] % 64 for k in range(1, len(names))) and any(voff[k] % 256 for k in range(1, len(names)))


def test_the_sample_counts_lie_around_the_list_lengths():
    """M = 0, M < S by 1 or 2, M a little above S and M >= 2 S all occur in the 1 cm batch"""
    ms = dict((n, m) for n, m, _ in _ms("cm"))
    assert LB.n_samples("all_dropped", ms["all_dropped"]) == 2 and LB.n_samples("dense_block", ms["dense_block"]) == 200
    assert min(ms["dense_block"]) >= 400 and all(m >= 48 for m in ms["row_1024"])  # M >= 2 S
    assert ms["two_cameras_same_lattice"] == [14, 12] and LB.n_samples("", [14, 12]) == 16  # M a little below S
    assert ms["row_63"] == [32, 31] and LB.n_samples("row_63", ms["row_63"]) == 24  # M a little above S
    mm = dict((n, m) for n, m, _ in _ms("mm"))
    assert LB.n_samples("", mm["stride32"]) == 24 and sorted(mm["stride32"]) == [14, 20, 20, 22] and min(mm["values"]) >= 48


def test_the_sequence_takes_the_kept_slot_path():
    """cm_small sizes the slots a context keeps (the largest lattice + 25 %, in whole blocks, + one); the batch that follows holds
    dense_block, block_edge and two_cameras_same_lattice, whose two blocks fit the kept slots of three: it takes the kept-slot
    path on slots sized by OTHER lattices (tests/test_mask_batch_cases.py has the reasoning).  The repeat of a batch whose
    lattices outgrew the kept slots is run by the GPU test on the main depth batch, small workspace first."""
    first, then = (_points()[n] for n in LB.SEQUENCES["dense_after_small"])
    words = max(_lattice_words(c) for _, c in first)
    slot = ((words + words // 4) // WORDS_PER_BLOCK + 1) * WORDS_PER_BLOCK
    need = {n: _lattice_words(c) for n, c in then}
    assert words == 2 * WORDS_PER_BLOCK and slot == 3 * WORDS_PER_BLOCK
    assert need["dense_block"] == need["block_edge"] == need["two_cameras_same_lattice"] == 2 * WORDS_PER_BLOCK == max(need.values())
    assert not set(LB.LARGE_LATTICES) & set(_names(first))
