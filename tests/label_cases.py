"""Captures with label arrays for the agh_localize_labeled* tests (numpy only), built on tests/mask_cases.py.

A case is a mask case's dict with `labels` ((N,) uint8: 0 no object, j + 1 object j) and `n_objects` in the place of `mask`.
The model of object j's eligible voxels is mask_cases.eligible_model with the mask labels == j + 1 (eligible_lists).  Each case
is named after the regime tests/test_label_cases.py proves it is in.
"""
import numpy as np

from tests import mask_cases as M

F32 = np.float32
ROWS = (63, 64, 65, 1024, 1025)  # voxels in a row: the wave (64) and work-group (256) seams of the count / emit kernels


def _labeled(case, labels, n_objects):
    c = {k: v for k, v in case.items() if k != "mask"}
    c["labels"] = np.ascontiguousarray(labels, np.uint8)
    assert c["labels"].shape == (len(c["points"]),)
    c["n_objects"] = n_objects
    return c


def row_case(n):
    """n voxels in voxel order (rows of 32 along z, the fastest axis: voxel k is (0, k // 32, k % 32)), labels alternating
    1, 2 by voxel index; the corner is voxel 0"""
    k = np.arange(1, n)
    col = np.stack([np.zeros(n - 1), k // 32, k % 32], axis=1)
    pts = np.concatenate([M.corner(), M.lattice(col)])
    return _labeled(M._case(pts, np.zeros(n, np.uint8)), 1 + np.arange(n) % 2, 2)


def point_cases() -> dict:
    P = M.point_cases()
    rng = np.random.default_rng(77)
    cases = {}
    cases["k1"] = _labeled(P["tiny"], P["tiny"]["mask"], 1)
    # voxel (3, 0, 0) holds points of object 0 and of object 1, and unlabelled ones
    cases["dup_voxel"] = _labeled(P["dup_voxel"], [0, 1, 0, 2, 0, 1, 0], 2)
    # two objects: the bytes 255 belong to none
    cases["values"] = _labeled(P["values"], P["values"]["mask"], 2)
    lab = np.zeros(41, np.uint8)
    lab[1 + 31], lab[1 + 32] = 1, 2  # bit 31, the last of a word, and bit 32, the first of the next
    cases["word_edge"] = _labeled(P["word_edge"], lab, 2)
    # bits 131071 (31, 63, 63) and 131072 (32, 0, 0), either side of a 4096-word block, and their neighbours
    cases["block_edge"] = _labeled(P["block_edge"], [0, 0, 1, 2, 1, 2, 3], 3)
    g = np.stack(np.meshgrid(np.arange(33), np.arange(64), np.arange(64), indexing="ij"), axis=-1).reshape(-1, 3)
    cases["dense_block"] = _labeled(P["dense_block"], 1 + g.sum(1) % 3, 3)
    c = P["two_cameras_same_lattice"]
    cases["two_cameras_same_lattice"] = _labeled(c, c["mask"] * (1 + np.arange(len(c["mask"])) % 2), 2)
    cases["rank_cameras"] = _labeled(P["rank_cameras"], [1, 0, 0, 0, 2, 1, 0, 2, 0, 0], 2)
    # raw points 0, 1 and 6.. are dropped by the preprocessing (NaN, inf, outside the workspace); 3 and 5 are kept
    lab = np.full(len(P["dropped"]["points"]), 2, np.uint8)
    lab[2:6] = [0, 1, 0, 3]
    cases["dropped"] = _labeled(P["dropped"], lab, 3)  # object 1 holds dropped points only: M = (1, 0, 1)
    lab = 1 + np.arange(len(lab), dtype=np.uint8) % 3
    lab[2:6] = 0
    cases["all_dropped"] = _labeled(P["all_dropped"], lab, 3)
    c = P["stride32"]
    cases["stride32"] = _labeled(c, c["mask"] * (1 + rng.integers(0, 4, len(c["mask"]))), 4)
    # 64 objects, one voxel each
    pts = np.concatenate([M.corner(), M.lattice([[i + 1, i % 3, 0] for i in range(64)])])
    cases["k64"] = _labeled(M._case(pts, np.zeros(65, np.uint8)), np.arange(65), 64)
    for n in ROWS:
        cases["row_%d" % n] = row_case(n)
    return cases


def cams_of(c):
    return M.camera_ids(c["points"], c["size_left"], c["dense"])


def eligible_lists(c, cams=None):
    """[E_0 .. E_{K-1}] of include/agh.h (agh_localize_labeled)"""
    cams = cams_of(c) if cams is None else cams
    return [M.eligible_model(c["points"], cams, c["labels"] == j + 1, c["workspace"], c["cell"]) for j in range(c["n_objects"])]


def tiled_labels(shape, rows=3, cols=4) -> np.ndarray:
    """an image tiled rows x cols into objects 0 .. rows * cols - 1 (labels 1 ..), row-major"""
    v, u = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return (1 + (v * rows // shape[0]) * cols + u * cols // shape[1]).astype(np.uint8)
