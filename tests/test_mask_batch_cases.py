"""The masked batches (tests/mask_batch_cases.py) reach the regimes the batched mask stage can go wrong in, on the numpy model
alone.

CPU only.  tests/test_gpu_localize_batch_masked.py holds the GPU to the model on these batches by exact equality; what is
asserted here is where the captures' masks lie in the packed buffer (k_mask_mark_batch's aligned-word trick is per capture), which
slots the block-edge cases sit in, and which of M_k = 0, M_k < S_k and M_k >= 2 S_k each batch holds.
"""
import functools

import numpy as np
import pytest

from tests import depth_captures as D
from tests import mask_batch_cases as MB
from tests import mask_cases as M
from tests import vox_edge_clouds as V

WORDS_PER_BLOCK = 4096


@functools.lru_cache(maxsize=None)
def _points():
    return MB.point_batches()


def _names(batch):
    return [n for n, _ in batch]


def test_the_batches_are_the_ones_the_gpu_test_names():
    b = _points()
    assert set(b) == {"cm", "cm_reversed", "mm", "mm_rotated", "cm_small"} and set(MB.SEQUENCES) == {"dense_after_small"}
    assert set(_names(b["cm"])) == {n for n, c in M.point_cases().items() if c["cell"] == 0.01} and len(b["cm"]) == 10
    assert _names(b["cm_reversed"]) == _names(b["cm"])[::-1]
    assert sorted(_names(b["mm"])) == sorted(_names(b["mm_rotated"])) == ["stride32", "values", "values_other_mask"]
    assert _names(b["mm"]) != _names(b["mm_rotated"])
    for name, batch in b.items():
        assert len({c["cell"] for _, c in batch}) == 1, name  # cell_size must be equal across a batch
    v, o = dict(b["mm"])["values"], dict(b["mm"])["values_other_mask"]
    assert np.array_equal(v["points"], o["points"]) and not np.array_equal(v["mask"] != 0, o["mask"] != 0) and o["mask"].any()


@pytest.mark.parametrize("name", sorted(MB.point_batches()))
def test_each_capture_of_the_packed_buffer_gives_its_own_model(name):
    batch = _points()[name]
    off = MB.raw_offsets(MB.point_counts(batch))
    packed = np.concatenate([c["mask"] for _, c in batch])
    assert len(packed) == off[-1]
    for k, (n, c) in enumerate(batch):
        own = packed[off[k]:off[k + 1]]
        assert np.array_equal(own, c["mask"])
        cams = M.camera_ids(c["points"], c["size_left"], c["dense"])
        E, vox = MB.point_model(c)
        assert np.array_equal(E, M.eligible_model(c["points"], cams, own, c["workspace"], c["cell"]))
        assert len(vox[0]) == sum(M.voxel_counts(c["points"], cams, c["workspace"], c["cell"])) and (E < max(len(vox[0]), 1)).all()


def test_where_the_masks_lie_in_the_packed_buffer():
    starts, ends, neighbours = set(), set(), 0
    for name, batch in _points().items():
        off = MB.raw_offsets(MB.point_counts(batch))
        starts |= {int(o) % 4 for o in off[:-1]}
        ends |= {int(o) % 4 for o in off[1:]}
        packed = np.concatenate([c["mask"] for _, c in batch])
        for k in range(1, len(batch)):
            # the aligned word that straddles the boundary between captures k - 1 and k holds non-zero bytes of one of them
            w0 = int(off[k]) // 4 * 4
            if off[k] % 4 and packed[w0:w0 + 4].any():
                neighbours += 1
    assert starts == {0, 1, 2, 3}  # every residue of a capture's first byte
    assert {3, 0} <= ends  # one capture ends a byte before a word boundary, one on it
    assert neighbours >= 5
    for name in ("cm", "cm_reversed"):
        off = MB.raw_offsets(MB.point_counts(_points()[name]))
        assert {int(o) % 4 for o in off[:-1]} == {0, 1, 2, 3}, name


def test_the_regimes_of_m_and_the_slots():
    for name in ("cm", "cm_reversed"):
        batch = _points()[name]
        names = _names(batch)
        assert names.index("block_edge") != 0 and names.index("dense_block") != 0
        assert names.index("all_dropped") not in (0, len(names) - 1)  # M = 0 between captures that have samples
        ms = {n: len(MB.point_model(c)[0]) for n, c in batch}
        ss = {n: MB.n_samples(n, m) for n, m in ms.items()}
        assert ms["all_dropped"] == 0 and ss["all_dropped"] == 2
        assert any(0 < ms[n] < ss[n] for n in names) and any(ms[n] >= 2 * ss[n] for n in names)
        assert ms["dense_block"] >= 2 * ss["dense_block"] == 400
    ms = [len(MB.point_model(c)[0]) for _, c in _points()["mm"]]
    assert all(m >= 2 * MB.n_samples("", m) for m in ms) and len(set(ms)) == 3


def _lattice_words(c):
    """the words of the capture's voxel bitmap: per camera the lattice's bits in words, rounded up to whole blocks"""
    return V.lattice_words(c["points"], c["size_left"], c["workspace"], c["cell"], c["dense"])


def test_the_sequence_takes_the_kept_slot_path():
    """cm_small sizes the slots a context keeps (the largest lattice + 25 %, in whole blocks, + one).  Every 1 cm case needs one
    block per camera, or two for dense_block and block_edge, so with rank_cameras' two camera blocks among the small ones the kept
    slots (12288 words) hold the batch that follows: it takes the kept-slot path, on slots sized by OTHER lattices, with
    dense_block and block_edge reaching into a block the first batch never marked.  No 1 cm case can outgrow such a slot; the
    repeat of a batch whose lattices outgrew the kept slots is run by the GPU test on the main depth batch, small workspace first."""
    first, then = (_points()[n] for n in MB.SEQUENCES["dense_after_small"])
    words = max(_lattice_words(c) for _, c in first)
    slot = ((words + words // 4) // WORDS_PER_BLOCK + 1) * WORDS_PER_BLOCK
    need = {n: _lattice_words(c) for n, c in then}
    assert words == 2 * WORDS_PER_BLOCK and slot == 3 * WORDS_PER_BLOCK
    assert need["dense_block"] == need["block_edge"] == need["two_cameras_same_lattice"] == 2 * WORDS_PER_BLOCK == max(need.values())
    assert not {"dense_block", "block_edge", "two_cameras_same_lattice"} & set(_names(first))
    one_camera = [c for n, c in first if n != "rank_cameras"]
    assert max(_lattice_words(c) for c in one_camera) == WORDS_PER_BLOCK  # (only camera blocks of one 4096-word block there)


def test_depth_batches():
    b = MB.depth_batches()
    edge, main = b["edge"], b["main"]
    kinds = {"padded": 0, "second_null": 0, "invalid": 0}
    ms = []
    for k, (images, masks, ws) in enumerate(zip(edge["captures"], edge["masks"], edge["workspaces"])):
        assert len(masks) == len(images) and any(m is not None for m in masks)
        for im, m in zip(images, masks):
            assert m is None or (m.shape == im["data"].shape and m.dtype == np.uint8)
        E, vox, packed, pts = MB.depth_model(images, masks, ws)
        ms.append(len(E))
        if k % 3 == 0:
            kinds["padded"] += all(m.strides[0] > m.shape[1] and (m.base[:, m.shape[1]:] != 0).all() for m in masks)
        if k % 3 == 1 and len(images) == 2:
            kinds["second_null"] += masks[1] is None
        if k % 3 == 2:
            bad = ~np.isfinite(pts).all(1)
            kinds["invalid"] += bool(bad.any() and (packed[bad] != 0).all())
            assert np.array_equal(E, M.eligible_model(pts, D.image_index(images), np.where(bad, 0, packed), ws))
    assert kinds["padded"] >= 3 and kinds["second_null"] >= 1 and kinds["invalid"] >= 2, kinds
    assert min(ms) == 0 and max(ms) >= 48 and any(0 < m < 22 for m in ms), ms  # M = 0, M < S and M >= 2 S with S = min(M + 2, 24)
    off = MB.raw_offsets(MB.depth_counts(edge))
    assert {int(o) % 4 for o in off[:-1]} == {0, 1, 2, 3} and {0, 3} <= {int(o) % 4 for o in off[1:]}
    assert len(main["captures"]) == 6 and [len(c) for c in main["captures"]].count(1) == 1
    for images, masks in zip(main["captures"], main["masks"]):
        assert masks[0][MB.RECT].all() and masks[0].sum() == 80 * 80 and (len(masks) == 1 or masks[1] is None)
