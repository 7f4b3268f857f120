"""Captures with sample masks for the agh_localize_masked* tests, and a numpy model of the eligible voxels (numpy only).

A points case is a dict: `points` ((N, 3) or (N, 8) float32 records, x y z first), `size_left`, `dense`, `workspace`, `cell`,
`mask` ((N,) uint8, one byte per raw point).  A depth case is (images, masks, workspace): images as tests/depth_captures.py
makes them, masks one (H, W) uint8 array per image (rows possibly padded) or None.

  camera_ids       the voxeliser's camera id per raw point: the raw index for dense = 1, the rank rule for dense = 0
  eligible_model   E of include/agh.h (agh_localize_masked): the indices, in the voxelised cloud, of the voxels that hold a kept
                   masked point -- ranks among the per-camera unique voxels, camera 0 block first
  bit_positions    where the voxeliser's bitmap holds each kept point (camera, bit in that camera's lattice)
  point_cases / depth_cases   the inputs the tests run, each named after the regime tests/test_mask_cases.py proves it is in
"""
import numpy as np

from tests import depth_captures as D

F32 = np.float32
CELL = 0.003
WIDE = np.array([-10.0, 10.0, -10.0, 10.0, -10.0, 10.0])


def camera_ids(points: np.ndarray, size_left: int, dense) -> np.ndarray:
    p = np.asarray(points, F32)[:, :3]
    if dense:
        return (np.arange(len(p)) >= size_left).astype(np.int32)
    return D.rank_labels(p, size_left)


def _kept(points, workspace):
    ws = np.asarray(workspace, np.float64)
    p = np.asarray(points, F32)[:, :3]
    with np.errstate(invalid="ignore"):
        return ((p[:, 0] >= ws[0]) & (p[:, 0] <= ws[1]) & (p[:, 1] >= ws[2]) & (p[:, 1] <= ws[3]) & (p[:, 2] >= ws[4])
                & (p[:, 2] <= ws[5]))


def _voxels(points, cams, workspace, cell):
    """per camera: (raw indices of its kept points, their integer voxel coordinates)"""
    p = np.asarray(points, F32)[:, :3]
    inb = _kept(p, workspace)
    out = []
    for c in (0, 1):
        sel = np.flatnonzero(inb & (cams == c))
        if len(sel) == 0:
            out.append((sel, np.zeros((0, 3), np.int64)))
            continue
        q = p[sel].astype(np.float64)
        out.append((sel, np.floor((q - q.min(0)) / cell).astype(np.int64)))
    return out


def eligible_model(points, cams, mask, workspace, cell: float = CELL) -> np.ndarray:
    """E: ascending indices into D.voxel_model(points, cams, workspace, cell) of the voxels with a kept masked point."""
    mask = np.asarray(mask).reshape(-1)
    out, base = [], 0
    for sel, ijk in _voxels(points, cams, workspace, cell):
        if len(sel) == 0:
            continue
        uniq, inv = np.unique(ijk, axis=0, return_inverse=True)
        out.append(base + np.unique(inv.reshape(-1)[mask[sel] != 0]))
        base += len(uniq)
    e = np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)
    if (_kept(points, workspace) & (np.asarray(cams) >= 0)).any():
        assert base == len(D.voxel_model(np.asarray(points, F32)[:, :3], cams, workspace, cell)[0])
    return e


def voxel_counts(points, cams, workspace, cell: float = CELL):
    return [len(np.unique(ijk, axis=0)) if len(sel) else 0 for sel, ijk in _voxels(points, cams, workspace, cell)]


def bit_positions(points, cams, workspace, cell: float = CELL):
    """(raw index, camera, bit position in the camera's lattice, the lattice's dims) of every kept point: x-major, z-fastest."""
    out = []
    for c, (sel, ijk) in enumerate(_voxels(points, cams, workspace, cell)):
        if len(sel) == 0:
            continue
        dim = ijk.max(0) + 1
        pos = (ijk[:, 0] * dim[1] + ijk[:, 1]) * dim[2] + ijk[:, 2]
        out.append((sel, c, pos, dim))
    return out


def lattice(ijk, cell: float = 0.01, origin=(0.25, 0.25, 0.25)) -> np.ndarray:
    """Points in the middle of the voxels `ijk` of a lattice whose voxel (0, 0, 0) must be pinned by a point AT `origin`
    (corner()): the float32 rounding of a centre stays far from a face."""
    return (np.asarray(origin, np.float64) + (np.asarray(ijk, np.float64) + 0.5) * cell).astype(F32)


def corner(origin=(0.25, 0.25, 0.25)) -> np.ndarray:
    return np.asarray(origin, F32)[None, :]


def _case(points, mask, size_left=None, dense=False, workspace=WIDE, cell=0.01):
    points = np.ascontiguousarray(points, F32)
    mask = np.ascontiguousarray(mask, np.uint8)
    assert mask.shape == (len(points),)
    return dict(points=points, mask=mask, size_left=len(points) if size_left is None else size_left, dense=dense,
                workspace=np.asarray(workspace, np.float64), cell=cell)


def _random_cloud(rng, n, extent=0.05):
    return rng.uniform(0.3, 0.3 + extent, (n, 3)).astype(F32)


def point_cases() -> dict:
    rng = np.random.default_rng(2024)
    cases = {}
    cases["tiny"] = _case(np.concatenate([corner(), lattice([[2, 0, 0], [4, 1, 0]])]), [0, 1, 0])
    # three masked and two unmasked points in voxel (3, 0, 0); the corner and (6, 0, 0) unmasked
    cases["dup_voxel"] = _case(np.concatenate([corner(), lattice([[3, 0, 0]] * 5) + F32(0.001) * np.arange(5, dtype=F32)[:, None],
                                               lattice([[6, 0, 0]])]), [0, 1, 0, 1, 0, 1, 0])
    # a row of voxels 0..5: 1 and 3 and 4 eligible, 2 holds two unmasked points only
    row = lattice([[1, 0, 0], [2, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [5, 0, 0]])
    cases["neighbour_unmasked"] = _case(np.concatenate([corner(), row]), [0, 1, 0, 0, 1, 1, 0])
    # masked points the preprocessing drops: NaN, +-inf, and one float beyond each face of the workspace
    ws = np.array([0.25, 0.5, 0.25, 0.5, 0.25, 0.5])
    inside = lattice([[1, 1, 1], [5, 2, 3], [7, 7, 7]])
    out = []
    for a in range(3):
        for face, toward in ((0.25, 0.0), (0.5, 1.0)):
            q = np.array([0.3, 0.3, 0.3], F32)
            q[a] = np.nextafter(F32(face), F32(toward))
            out.append(q)
    bad = np.array([[np.nan, 0.3, 0.3], [0.3, np.inf, 0.3], [0.3, 0.3, -np.inf], [np.nan, np.nan, np.nan]], F32)
    dropped = np.concatenate([bad[:2], corner(), inside, np.stack(out), bad[2:]])
    m = np.ones(len(dropped), np.uint8)
    m[2:5] = 0  # the corner and two of the inside voxels unmasked; (7, 7, 7) masked
    cases["dropped"] = _case(dropped, m, workspace=ws)
    m = m.copy()
    m[5] = 0
    cases["all_dropped"] = _case(dropped, m, workspace=ws)
    # the same coordinates in both cameras, the mask on camera 1's points only
    half = np.concatenate([corner(), lattice(rng.integers(0, 12, (40, 3)))])
    cases["two_cameras_same_lattice"] = _case(np.concatenate([half, half]), np.r_[np.zeros(len(half)), rng.random(len(half)) < 0.5],
                                              size_left=len(half), dense=True)
    # one row of 40 voxels along z (bit = iz): bits 31 and 32, the last of a word and the first of the next
    col = np.stack([np.zeros(40), np.zeros(40), np.arange(40)], axis=1)
    m = np.zeros(41, np.uint8)
    m[1 + 31] = m[1 + 32] = 1
    cases["word_edge"] = _case(np.concatenate([corner(), lattice(col)]), m)
    # ny = nz = 64 pinned by the far corner: (31, 63, 63) and (32, 0, 0) are bits 131071 and 131072, the last of a 4096-word
    # block and the first of the next
    ijk = np.array([[33, 63, 63], [31, 63, 63], [32, 0, 0], [31, 63, 62], [32, 0, 1], [5, 5, 5]])
    cases["block_edge"] = _case(np.concatenate([corner(), lattice(ijk)]), [0, 0, 1, 1, 0, 0, 1])
    # a filled 33 x 64 x 64 lattice: every bit of the first block set (131072 voxels in it), a checkerboard mask
    g = np.stack(np.meshgrid(np.arange(33), np.arange(64), np.arange(64), indexing="ij"), axis=-1).reshape(-1, 3)
    full = lattice(g)
    full[0] = corner()[0]
    cases["dense_block"] = _case(full, (g.sum(1) % 2).astype(np.uint8))
    # dense = 0 with NaNs ahead of size_left: raw points 4 and 5 are camera 1 by raw index, camera 0 by rank
    o2 = (0.1, 0.25, 0.25)  # (below the first lattice in x: the raw-index rule would order the voxels differently)
    pts = np.concatenate([np.full((2, 3), np.nan, F32), corner(), lattice([[3, 1, 0], [5, 0, 2], [6, 2, 2]]),
                          corner(o2), lattice([[2, 2, 2], [4, 1, 1], [9, 9, 9]], origin=o2)])
    cases["rank_cameras"] = _case(pts, [1, 0, 0, 0, 1, 1, 0, 1, 0, 0], size_left=4, dense=False)
    # 32-byte records, the mask packed
    rec = np.full((300, 8), 7.0, F32)
    rec[:, :3] = _random_cloud(rng, 300)
    cases["stride32"] = _case(rec, rng.random(300) < 0.3, size_left=170, dense=True, cell=CELL)
    # every non-zero byte means eligible
    cases["values"] = _case(_random_cloud(rng, 257), rng.choice(np.array([0, 1, 2, 255], np.uint8), 257), size_left=100, cell=CELL)
    return cases


def padded_mask(rng, m: np.ndarray, pad: int) -> np.ndarray:
    """the same mask in rows `pad` bytes longer, the padding non-zero"""
    wide = rng.integers(1, 256, (m.shape[0], m.shape[1] + pad)).astype(np.uint8)
    wide[:, :m.shape[1]] = m
    return wide[:, :m.shape[1]]


def invalid_pixels(im) -> np.ndarray:
    d = im["data"]
    with np.errstate(invalid="ignore"):
        return (d == 0) if d.dtype == np.uint16 else ~((d > 0) & (d < np.inf))


def capture_box(images) -> np.ndarray:
    pts = D.deproject_ref(images)
    fin = pts[np.isfinite(pts).all(1)]
    return np.stack([fin.min(0), fin.max(0)], axis=1).reshape(6).astype(np.float64)


DEPTH_NAMES = ("u16_63x3", "f32_65x2", "u16_odd_stride", "total_1025", "main")


def depth_cases() -> dict:
    """name -> (images, masks, workspace): random masks in padded rows, image 1's mask NULL, masks over the invalid pixels"""
    rng = np.random.default_rng(99)
    edge = D.edge_cases()
    cases = {}
    for name in DEPTH_NAMES:
        images = edge[name]
        ws = D.main_case()[1] if name == "main" else capture_box(images)
        frac = 0.02 if name == "main" else 0.3
        rand = [(rng.random(im["data"].shape) < frac).astype(np.uint8) * rng.integers(1, 256, im["data"].shape).astype(np.uint8)
                for im in images]
        cases[name + "_random_padded"] = (images, [padded_mask(rng, m, 1 + 2 * k) for k, m in enumerate(rand)], ws)
        cases[name + "_packed"] = (images, [np.ascontiguousarray(m) for m in rand], ws)
        if len(images) == 2:
            cases[name + "_second_null"] = (images, [rand[0], None], ws)
            cases[name + "_first_null"] = (images, [None, padded_mask(rng, rand[1], 5)], ws)
        # every invalid pixel masked, and a few valid ones
        inv = [(invalid_pixels(im) | (rng.random(im["data"].shape) < 0.5 * frac)).astype(np.uint8) for im in images]
        cases[name + "_invalid_pixels"] = (images, inv, ws)
    return cases


def packed_masks(images, masks) -> np.ndarray:
    """the masks' rows end to end in image order, zeros for a None: the points form's mask of the deprojected capture"""
    return np.concatenate([np.zeros(im["data"].size, np.uint8) if m is None else np.ascontiguousarray(m, np.uint8).reshape(-1)
                           for im, m in zip(images, masks)])
