"""Batches of captures with sample masks for the agh_localize_batch_masked* tests (numpy only), built from the single-capture
cases of tests/mask_cases.py and the depth batches of tests/depth_batch_captures.py.

A points batch is a list of (name, case) pairs, a case as tests/mask_cases.py makes it; cell_size must be equal across a batch,
so the 1 cm cases and the 3 mm cases go into batches of their own.  A depth batch is a dict: `captures` (a list of image lists),
`masks` (per capture a list with one (H, W) uint8 array or None per image) and `workspaces` (one per capture).

  point_batches    name -> batch; SEQUENCES names the batches that run one after the other on ONE context
  depth_batches    "edge" and "main"
  raw_offsets      capture k's first byte in the packed mask buffer (= its first point among the batch's)
  point_model / depth_model   E_k and the voxel model of one capture alone: what the batch must give for it
  n_samples / seed            S_k and seed_k the GPU test draws with
"""
import numpy as np

from tests import depth_batch_captures as DB
from tests import depth_captures as D
from tests import mask_cases as M

RECT = (slice(80, 160), slice(120, 200))  # tests/test_gpu_localize_masked.py's rectangle: rows, columns of image 0 of the main case
CM, MM = 0.01, M.CELL

# the batches that run one after the other on one context: the first one's lattices size the kept bitmap slots
SEQUENCES = {"dense_after_small": ("cm_small", "cm")}


def _named_cases() -> dict:
    cases = dict(M.point_cases())
    rng = np.random.default_rng(7)
    v = cases["values"]
    cases["values_other_mask"] = dict(v, mask=(rng.random(len(v["mask"])) < 0.35).astype(np.uint8) * np.uint8(200))
    return cases


def point_batches() -> dict:
    cases = _named_cases()
    cm = [n for n in M.point_cases() if cases[n]["cell"] == CM]  # (in the order tests/mask_cases.py builds them)
    assert len(cm) == 10 and cm.index("all_dropped") not in (0, len(cm) - 1)
    mm = ["stride32", "values", "values_other_mask"]
    assert all(cases[n]["cell"] == MM for n in mm)
    small = [n for n in cm if n not in ("dense_block", "block_edge", "two_cameras_same_lattice")]
    orders = {"cm": cm, "cm_reversed": cm[::-1], "mm": mm, "mm_rotated": mm[1:] + mm[:1], "cm_small": small}
    return {name: [(n, cases[n]) for n in order] for name, order in orders.items()}


def raw_offsets(counts) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def point_counts(batch) -> list:
    return [len(c["points"]) for _, c in batch]


def n_samples(name: str, m: int) -> int:
    return 200 if name == "dense_block" else min(m + 2, 24)


def seed(k: int) -> int:
    return 11 + k


def voxels_or_none(points, cams, workspace, cell):
    """D.voxel_model, or empty arrays for a capture that keeps no point"""
    keep = np.asarray(cams) >= 0
    p, c = np.asarray(points, np.float32)[keep, :3], np.asarray(cams)[keep]
    ws = np.asarray(workspace, np.float64)
    with np.errstate(invalid="ignore"):
        inb = ((p >= ws[0::2]) & (p <= ws[1::2])).all(1)
    if not inb.any():
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    return D.voxel_model(p, c, workspace, cell)


def point_model(c):
    cams = M.camera_ids(c["points"], c["size_left"], c["dense"])
    return (M.eligible_model(c["points"], cams, c["mask"], c["workspace"], c["cell"]),
            voxels_or_none(c["points"], cams, c["workspace"], c["cell"]))


def depth_model(images, masks, ws, pts=None):
    """(E, voxel model, packed mask, points) of one depth capture alone; pts: its deprojected points if the caller has them"""
    pts = D.deproject_ref(images) if pts is None else pts
    cams = D.image_index(images)
    packed = M.packed_masks(images, masks)
    return M.eligible_model(pts, cams, packed, ws), voxels_or_none(pts, cams, ws, M.CELL), packed, pts


def _box_or_wide(images):
    """the box of the capture's finite points, cut to 1 m around their median (u16_extremes reaches 16 m: at 3 mm its lattice
    would exceed the voxeliser's limit); a capture without a finite point: the wide box"""
    pts = D.deproject_ref(images)
    fin = pts[np.isfinite(pts).all(1)]
    if len(fin) == 0:
        return M.WIDE.copy()
    med = np.median(fin.astype(np.float64), axis=0)
    box = M.capture_box(images).reshape(3, 2)
    return np.stack([np.maximum(box[:, 0], med - 1.0), np.minimum(box[:, 1], med + 1.0)], axis=1).reshape(6)


_DEPTH = {}


def depth_batches() -> dict:
    """Cached, read-only.  edge: DB.edge_batch() with, capture after capture in turn, random masks in padded rows, a NULL second
    mask (a one-image capture: a packed random mask) and masks over the invalid pixels.  main: DB.main_batch() with the rectangle
    RECT on image 0 and image 1's mask NULL."""
    if _DEPTH:
        return _DEPTH
    rng = np.random.default_rng(2025)
    caps = DB.edge_batch()
    masks, wss = [], []
    for k, images in enumerate(caps):
        big = images[0]["data"].size > 10000
        frac = 0.02 if big else 0.4
        rand = [(rng.random(im["data"].shape) < frac).astype(np.uint8) * rng.integers(1, 256, im["data"].shape).astype(np.uint8)
                for im in images]
        kind = k % 3
        if kind == 0:
            ms = [M.padded_mask(rng, m, 1 + 2 * j) for j, m in enumerate(rand)]
        elif kind == 1:
            ms = [rand[0], None] if len(images) == 2 else [np.ascontiguousarray(rand[0])]
        else:
            ms = [(M.invalid_pixels(im) | (rng.random(im["data"].shape) < 0.5 * frac)).astype(np.uint8) for im in images]
        masks.append(ms)
        wss.append(D.main_case()[1].copy() if DB.EDGE_ORDER[k] in ("main", "one_image") else _box_or_wide(images))
    _DEPTH["edge"] = dict(captures=caps, masks=masks, workspaces=wss)
    caps, ws, origins = DB.main_batch()
    m0 = np.zeros(caps[0][0]["data"].shape, np.uint8)
    m0[RECT] = 1
    m0.setflags(write=False)
    _DEPTH["main"] = dict(captures=caps, masks=[[m0, None][:len(c)] for c in caps], workspaces=[ws.copy() for _ in caps],
                          origins=origins)
    return _DEPTH


def depth_counts(batch) -> list:
    return [DB.points_of(c) for c in batch["captures"]]
