"""The sample-mask inputs (tests/mask_cases.py) reach the regime each one names, on the numpy model alone.

CPU only.  tests/test_gpu_localize_masked.py holds the GPU to the model on these cases by exact equality; what is asserted here
is that the model, and so a GPU that agrees with it, is then on the bit, the word, the block or the camera rule that the case is
there for -- with bit positions computed from the model.  A case that stops meeting its condition fails here.
"""
import functools
import os
import re

import numpy as np
import pytest

from tests import depth_captures as D
from tests import mask_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS_PER_BLOCK = 4096


@functools.lru_cache(maxsize=None)
def _points():
    return M.point_cases()


@functools.lru_cache(maxsize=None)
def _depth():
    return M.depth_cases()


def _model(name):
    c = _points()[name]
    cams = M.camera_ids(c["points"], c["size_left"], c["dense"])
    return c, cams, M.eligible_model(c["points"], cams, c["mask"], c["workspace"], c["cell"])


def _masked_bits(c, cams):
    """per camera: (bit positions of the kept masked points, of the kept unmasked points, dims)"""
    out = {}
    for sel, cam, pos, dim in M.bit_positions(c["points"], cams, c["workspace"], c["cell"]):
        on = c["mask"][sel] != 0
        out[cam] = (np.unique(pos[on]), np.unique(pos[~on]), dim)
    return out


def test_the_block_size_is_the_voxelisers():
    with open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "voxelize.hip")) as f:
        vox = f.read()
    with open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_mask.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int kWordsPerBlock = (\d+);", vox).group(1)) == WORDS_PER_BLOCK
    assert int(re.search(r"constexpr int kMaskWordsPerBlock = (\d+);", src).group(1)) == WORDS_PER_BLOCK
    assert {"tiny", "dup_voxel", "neighbour_unmasked", "dropped", "all_dropped", "two_cameras_same_lattice", "word_edge", "block_edge",
            "dense_block", "rank_cameras", "stride32", "values"} == set(_points())


def test_tiny_dup_and_neighbour():
    c, cams, E = _model("tiny")
    assert len(c["points"]) == 3 and c["mask"].sum() == 1 and E.tolist() == [1]
    c, cams, E = _model("dup_voxel")
    on, off, _ = _masked_bits(c, cams)[0]
    assert (c["mask"] != 0).sum() == 3 and len(on) == 1 and on[0] in off and len(E) == 1  # masked and unmasked in ONE voxel
    c, cams, E = _model("neighbour_unmasked")
    on, off, dim = _masked_bits(c, cams)[0]
    assert dim.tolist() == [6, 1, 1] and on.tolist() == [1, 3, 4] and 2 in off and 2 not in on and E.tolist() == [1, 3, 4]


def test_dropped_points_make_nothing_eligible():
    c, cams, E = _model("dropped")
    p, m, ws = c["points"], c["mask"], c["workspace"]
    kept = M._kept(p, ws) & (cams >= 0)
    lost = (m != 0) & ~kept
    assert np.isnan(p[lost]).any() and (p[lost] == np.inf).any() and (p[lost] == -np.inf).any()
    for a in range(3):  # one float beyond each face, and the other two coordinates inside
        assert (p[lost][:, a] == np.nextafter(np.float32(ws[2 * a]), np.float32(0))).any()
        assert (p[lost][:, a] == np.nextafter(np.float32(ws[2 * a + 1]), np.float32(1))).any()
    assert lost.sum() == 10 and (kept & (m != 0)).sum() == 1 and len(E) == 1 and M.voxel_counts(p, cams, ws, c["cell"]) == [4, 0]
    c2, cams2, E2 = _model("all_dropped")
    assert np.array_equal(c2["points"], p, equal_nan=True) and (c2["mask"] != 0).sum() == 10 and len(E2) == 0
    assert not (M._kept(p, ws) & (c2["mask"] != 0)).any()


def test_two_cameras_same_lattice():
    c, cams, E = _model("two_cameras_same_lattice")
    n = c["size_left"]
    assert np.array_equal(c["points"][:n], c["points"][n:]) and not c["mask"][:n].any() and c["mask"][n:].sum() > 5
    nv = M.voxel_counts(c["points"], cams, c["workspace"], c["cell"])
    assert nv[0] == nv[1] > 20 and len(E) > 5 and (E >= nv[0]).all()
    bits = _masked_bits(c, cams)
    assert len(bits[0][0]) == 0 and np.isin(bits[1][0], np.union1d(bits[0][0], bits[0][1])).all()  # the same bits, the other camera


def test_word_and_block_edges():
    c, cams, E = _model("word_edge")
    on, off, dim = _masked_bits(c, cams)[0]
    assert dim.tolist() == [1, 1, 40] and on.tolist() == [31, 32] and E.tolist() == [31, 32]
    assert on[0] // 32 + 1 == on[1] // 32 and {30, 33} <= set(off.tolist())
    c, cams, E = _model("block_edge")
    on, off, dim = _masked_bits(c, cams)[0]
    edge = 32 * WORDS_PER_BLOCK
    assert dim.tolist() == [34, 64, 64] and {edge - 1, edge} <= set(on.tolist()) and {edge - 2, edge + 1} <= set(off.tolist())
    assert (edge - 1) // edge == 0 and edge // edge == 1 and E.tolist() == [1, 3, 4]


def test_dense_block():
    c, cams, E = _model("dense_block")
    on, off, dim = _masked_bits(c, cams)[0]
    bits = 32 * WORDS_PER_BLOCK
    assert dim.tolist() == [33, 64, 64] and len(on) + len(off) == 33 * 64 * 64 and not np.intersect1d(on, off).size
    first = np.concatenate([on[on < bits], off[off < bits]])
    assert len(first) == bits > 4096  # every bit of the first block is set: more voxels in it than k_vox_emit's list takes
    assert (on < bits).sum() == bits // 2 and np.array_equal(E, np.sort(on))  # (a full lattice: rank = bit position)
    pos = np.arange(33 * 64 * 64)
    assert np.array_equal(on, pos[(pos // 4096 + pos // 64 % 64 + pos % 64) % 2 == 1])  # the checkerboard: ranks inside full words


def test_rank_cameras():
    c, cams, E = _model("rank_cameras")
    p, m = c["points"], c["mask"]
    raw = M.camera_ids(p, c["size_left"], True)
    fin = np.isfinite(p).all(1)
    assert not c["dense"] and not fin[:c["size_left"]].all()
    differ = fin & (raw != cams)
    assert (differ & (m != 0)).sum() == 2 and (m[~fin] != 0).any()
    wrong = M.eligible_model(np.where(fin[:, None], p, np.float32(1e6)), raw, m, c["workspace"], c["cell"])
    assert not np.array_equal(E, wrong) and E.tolist() == [2, 3, 5]


def test_stride32_and_values():
    c, cams, E = _model("stride32")
    assert c["points"].shape == (300, 8) and c["points"].strides == (32, 4) and (c["points"][:, 3:] == 7.0).all()
    assert c["mask"].shape == (300,) and c["mask"].strides == (1,) and 20 < len(E) < sum(M.voxel_counts(c["points"], cams, c["workspace"], c["cell"]))
    c, cams, E = _model("values")
    assert set(np.unique(c["mask"]).tolist()) == {0, 1, 2, 255}
    for v in (1, 2, 255):  # each non-zero value makes a voxel eligible that no other value does
        only = M.eligible_model(c["points"], cams, c["mask"] == v, c["workspace"], c["cell"])
        others = M.eligible_model(c["points"], cams, (c["mask"] != 0) & (c["mask"] != v), c["workspace"], c["cell"])
        assert len(np.setdiff1d(only, others)) > 0 and np.isin(only, E).all()


@pytest.mark.parametrize("name", sorted(M.depth_cases()))
def test_depth_cases(name):
    images, masks, ws = _depth()[name]
    assert any(name.startswith(base + "_") for base in M.DEPTH_NAMES)
    pts = D.deproject_ref(images)
    packed = M.packed_masks(images, masks)
    assert packed.shape == (len(pts),)
    E = M.eligible_model(pts, D.image_index(images), packed, ws)
    nv = len(D.voxel_model(pts, D.image_index(images), ws)[0])
    assert 0 < len(E) < nv
    for im, m in zip(images, masks):
        assert m is None or m.shape == im["data"].shape
    if name.endswith("_random_padded"):
        for m in masks:
            assert m.strides[0] > m.shape[1] and m.base is not None and (m.base[:, m.shape[1]:] != 0).all()
    if name.endswith("_second_null"):
        assert masks[1] is None and (E < len(D.voxel_model(pts[:images[0]["data"].size], np.zeros(images[0]["data"].size, np.int32), ws)[0])).all()
    if name.endswith("_first_null"):
        n0 = images[0]["data"].size
        assert masks[0] is None and (E >= nv - len(D.voxel_model(pts[n0:], np.ones(len(pts) - n0, np.int32), ws)[0])).all()
    if name.endswith("_invalid_pixels"):
        bad = ~np.isfinite(pts).all(1)
        assert bad.any() and (packed[bad] != 0).all() and (packed[~bad] != 0).any()
        # the masked invalid pixels make nothing eligible
        assert np.array_equal(E, M.eligible_model(pts, D.image_index(images), np.where(bad, 0, packed), ws))


def test_masked_samples_follow_the_drawn_strata():
    from agile_grasp_amd.binding import draw_samples, masked_samples

    E = np.array([3, 4, 9, 17, 30, 31, 40], np.int32)
    for S in (6, 7, 8, 13, 17, 3, 1, 0):
        got = masked_samples(E, S, 5)
        pos = draw_samples(len(E), S, 5)
        assert got.dtype == np.int32 and got.shape == (S,)
        if S <= len(E):
            assert np.array_equal(got, E[pos]) and (np.diff(got) > 0).all()
        else:
            assert np.array_equal(got[:len(E)], E) and (got[len(E):] == -(1 << 31)).all()
    assert (masked_samples(np.zeros(0, np.int32), 4, 1) == -(1 << 31)).all()
