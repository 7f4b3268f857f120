"""Batches of depth-image captures for the agh_localize_depth_batch* tests (numpy only): lists of the image lists of
tests/depth_captures.py, as agile_grasp_amd.binding.Context.localize_depth_batch takes them.

  edge_batch   the sizes, formats and layouts at which k_deproject_batch takes another path, in one batch
  max_views    64 captures x 2 images: the view table's capacity
  main_batch   the captures the chain tests run: (captures, workspace, camera origins)
"""
import numpy as np

from tests import depth_captures as D
from tests.test_gpu_localize_depth import _shifted

SAMPLES = 160  # explicit samples per capture of main_batch

# edge_batch, in this order: names of D.edge_cases().  The starts (in points) follow from the totals: "main" starts at 0 (wide
# stores), "total_1025" and "total_1023" are each followed by a capture whose first point is no multiple of four.
EDGE_ORDER = ("main", "u16_1x1", "total_1025", "f32_padded", "total_1023", "u16_odd_stride", "one_image", "f32_1x1",
              "f32_special_unaligned", "u16_257x1", "f32_special_values", "u16_extremes", "f32_65x2")


def points_of(images) -> int:
    return sum(im["data"].size for im in images)


def starts_of(captures) -> np.ndarray:
    """capture k's first point among the batch's (len + 1 entries)"""
    return np.concatenate([[0], np.cumsum([points_of(c) for c in captures])]).astype(np.int64)


def deproject_ref(captures) -> np.ndarray:
    """what agh_deproject_batch writes: the captures' model points end to end"""
    return np.concatenate([D.deproject_ref(c) for c in captures])


def edge_batch():
    cases = D.edge_cases()
    return [cases[name] for name in EDGE_ORDER]


def max_views():
    rng = np.random.default_rng(123)
    out = []
    for k in range(64):
        sizes = [(int(rng.integers(1, 10)), int(rng.integers(1, 4))) for _ in range(2)]
        out.append([D._random_image(rng, w, h, (D.U16, D.F32)[(k + j) % 2], cam=j, pad=(k + j) % 3) for j, (w, h) in enumerate(sizes)])
    return out


def to_metres(images):
    """the same capture as float32 metres, rows padded as they were"""
    out = []
    for im in images:
        d = im["data"]
        wide = np.zeros((d.shape[0], d.strides[0] // d.itemsize), D.F32)
        wide[:, :d.shape[1]] = d.astype(D.F32) * D.F32(im["depth_scale"])
        out.append(dict(im, data=wide[:, :d.shape[1]]))
    return out


_MAIN = []


def main_batch():
    """Four shifted captures of the main case, one with image 0 only, one in float32 metres: (captures, workspace, origins).
    Cached, read-only."""
    if not _MAIN:
        images, ws, origins = D.main_case()
        caps = [_shifted(images, k) for k in range(4)] + [_shifted(images, 5)[:1], to_metres(_shifted(images, 2))]
        for c in caps:
            for im in c:
                im["data"].setflags(write=False)
        _MAIN.append((caps, ws, origins))
    return _MAIN[0]


def samples_for(k: int, n_voxels: int) -> np.ndarray:
    """capture k's explicit sample list"""
    return np.sort(np.random.default_rng(50 + k).permutation(n_voxels)[:SAMPLES]).astype(np.int32)


def voxels_of(images, ws):
    return D.voxel_model(D.deproject_ref(images), D.image_index(images), ws)
