"""Captures for the agh_set_voxel_filter tests, and a numpy model of rules 1 to 3 of include/agh.h (numpy only).

The model works on the integer voxel coordinates of tests/mask_cases.py (`_voxels`): per camera the unique voxels of the kept
points in lexicographic order -- the order of the voxelised cloud, camera 0's block first -- and for each the number of OTHER
occupied voxels of the same camera within the integer ball dx^2 + dy^2 + dz^2 <= radius^2.  A voxel is kept iff that support is at
least min_neighbors; the lattice (and with it every surviving row of the unfiltered cloud) is untouched.

  ball_offsets / B        the ball without its centre; B(r) = 7, 33, 123, 257 positions with it
  support / support_brute the model (sorted keys of a padded lattice), and an O(N^2) restatement the CPU tests hold it against
  filter_model            keep flags over the rows of the unfiltered voxelised cloud, the six counts, the supports
  filtered_cloud          D.voxel_model's cloud with the model's rows removed
  filtered_eligible       E of a masked / labelled call under the filter: indices into the FILTERED cloud
  cases()                 name -> case: `points`, `size_left`, `dense`, `workspace`, `cell`, `radius`, `min_neighbors`, `check`
                          (a predicate over the case and its model: what the case exercises), `all_pruned` / `none_pruned` where
                          a case is named for that
  speckle_capture         a small raw capture with injected stray points, and the parameters the chain tests run it with
"""
from __future__ import annotations

import functools

import numpy as np

from tests import depth_captures as D
from tests import mask_cases as M

F32 = np.float32
CELL = 0.01
WIDE = M.WIDE
BLOCK_BITS = 4096 * 32
LIST_CAP = 4096


# ---- the model ----

@functools.lru_cache(maxsize=None)
def ball_offsets(r: int) -> np.ndarray:
    g = np.stack(np.meshgrid(*[np.arange(-r, r + 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    d2 = (g * g).sum(1)
    return g[(d2 <= r * r) & (d2 > 0)]


def B(r: int) -> int:
    return len(ball_offsets(r)) + 1


def support(ijk: np.ndarray, dim, r: int) -> np.ndarray:
    """ijk: unique voxels of ONE camera inside a lattice of dims `dim`.  Positions outside the lattice never support: the lattice
    is padded by r on every side, so that a neighbour's key is unique and an outside position matches no voxel."""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    if len(ijk) == 0:
        return np.zeros(0, np.int64)
    dim = np.asarray(dim, np.int64)
    assert (ijk >= 0).all() and (ijk < dim).all()
    py, pz = int(dim[1]) + 2 * r, int(dim[2]) + 2 * r
    key = lambda v: ((v[:, 0] + r) * py + v[:, 1] + r) * pz + v[:, 2] + r
    keys = np.sort(key(ijk))
    out = np.zeros(len(ijk), np.int64)
    for off in ball_offsets(r):
        k = key(ijk + off)
        pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        out += keys[pos] == k
    return out


def support_brute(ijk: np.ndarray, r: int) -> np.ndarray:
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    d = ijk[:, None, :] - ijk[None, :, :]
    return ((d * d).sum(-1) <= r * r).sum(1) - 1


def filter_model(points, cams, workspace, cell, radius: int, min_neighbors: int) -> dict:
    """keep: bool per row of D.voxel_model(points, cams, workspace, cell); counts: n_occupied[2], n_pruned[2], n_kept[2];
    support: per row; ijk, cam: the rows' integer voxels and cameras; dims: per camera"""
    keep, sup, vox, cam = [], [], [], []
    counts = np.zeros(6, np.int64)
    dims = [None, None]
    for c, (sel, ijk) in enumerate(M._voxels(points, cams, workspace, cell)):
        if len(sel) == 0:
            continue
        uniq = np.unique(ijk, axis=0)
        dims[c] = ijk.max(0) + 1
        s = support(uniq, dims[c], radius)
        k = s >= min_neighbors
        counts[c], counts[2 + c], counts[4 + c] = len(uniq), int((~k).sum()), int(k.sum())
        keep.append(k)
        sup.append(s)
        vox.append(uniq)
        cam.append(np.full(len(uniq), c, np.int32))
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    return dict(keep=cat(keep, np.zeros(0, bool)), counts=counts, support=cat(sup, np.zeros(0, np.int64)),
                ijk=cat(vox, np.zeros((0, 3), np.int64)), cam=cat(cam, np.zeros(0, np.int32)), dims=dims)


def unfiltered_cloud(points, cams, workspace, cell):
    p = np.asarray(points, F32)[:, :3]
    if not (M._kept(p, workspace) & (np.asarray(cams) >= 0)).any():
        return np.zeros((0, 3), F32), np.zeros(0, np.int32)
    return D.voxel_model(p, cams, workspace, cell)


def filtered_cloud(points, cams, workspace, cell, keep):
    xyz, cam = unfiltered_cloud(points, cams, workspace, cell)
    assert len(xyz) == len(keep)
    return xyz[keep], cam[keep]


def filtered_eligible(points, cams, mask, workspace, cell, keep) -> np.ndarray:
    """A voxel is eligible iff a masked kept raw point falls into a SURVIVING voxel; its index is its row in the filtered cloud."""
    e = M.eligible_model(points, cams, mask, workspace, cell)
    new_index = np.cumsum(keep) - 1
    return new_index[e[keep[e]]].astype(np.int32)


def case_cams(c) -> np.ndarray:
    return M.camera_ids(c["points"], c["size_left"], c["dense"])


def case_model(c) -> dict:
    return filter_model(c["points"], case_cams(c), c["workspace"], c["cell"], c["radius"], c["min_neighbors"])


def bit_of(v, dim) -> int:
    return (int(v[0]) * int(dim[1]) + int(v[1])) * int(dim[2]) + int(v[2])


def row_of(m: dict, v, cam: int = 0) -> int:
    hit = np.flatnonzero((m["cam"] == cam) & (m["ijk"] == np.asarray(v)).all(1))
    assert len(hit) == 1, (v, cam)
    return int(hit[0])


# ---- building clouds from lattice coordinates ----

ORIGIN0, ORIGIN1 = (0.25, 0.25, 0.25), (0.1, 0.3, 0.2)


def _points(ijk, origin=ORIGIN0, seed=0):
    """one point in the middle of every voxel of `ijk` (which holds (0, 0, 0): the corner pins the camera's minimum there), with a
    second point in every third voxel, shuffled"""
    ijk = np.unique(np.asarray(ijk, np.int64).reshape(-1, 3), axis=0)
    assert (ijk == 0).all(1).any() and (ijk >= 0).all()
    rest = ijk[~(ijk == 0).all(1)]
    pts = np.concatenate([M.corner(origin), M.lattice(rest, CELL, origin), M.lattice(rest[::3], CELL, origin) + F32(0.001)])
    return pts[np.random.default_rng(seed).permutation(len(pts))]


def _case(ijk0, radius, min_neighbors, check, ijk1=None, **more):
    left = _points(ijk0) if ijk0 is not None else np.zeros((0, 3), F32)
    right = _points(ijk1, ORIGIN1, 1) if ijk1 is not None else np.zeros((0, 3), F32)
    pts = np.ascontiguousarray(np.concatenate([left, right]), F32)
    pts.setflags(write=False)
    return dict(points=pts, size_left=len(left), dense=True, workspace=np.asarray(WIDE, np.float64), cell=CELL, radius=radius,
                min_neighbors=min_neighbors, check=check, **more)


def _with_pins(ijk, dim):
    """the voxels, the corner and the far corner of a lattice of dims `dim` (both isolated unless the voxels say otherwise)"""
    return np.concatenate([np.asarray(ijk, np.int64).reshape(-1, 3), [[0, 0, 0]], [np.asarray(dim) - 1]])


# ---- the cases ----

def _ball_shape(r: int, cam: int = 0):
    """For every offset of the (2 r + 1)^3 cube one centre and one partner, the pairs 2 r + 2 or more apart in every axis they
    differ in: a pair survives min_neighbors = 1 iff its offset lies in the ball."""
    offs = np.stack(np.meshgrid(*[np.arange(-r, r + 1)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    offs = offs[(offs != 0).any(1)]
    side = 2 * r + 1
    pitch = side + 2 * r + 2  # a cell's extent, then the gap
    n = int(np.ceil(len(offs) ** (1 / 3)))
    cell_of = np.stack(np.unravel_index(np.arange(len(offs)), (n, n, n)), axis=1)
    centres = pitch + cell_of * pitch + r  # (the first cell starts a pitch in: the corner pin stays alone)
    ijk = np.concatenate([centres, centres + offs, [[0, 0, 0]]])
    inside = (offs * offs).sum(1) <= r * r

    def check(c, m):
        ok = True
        for ctr, off, ins in zip(centres, offs, inside):
            a, b = row_of(m, ctr, cam), row_of(m, ctr + off, cam)
            ok &= m["support"][a] == int(ins) and m["support"][b] == int(ins) and m["keep"][a] == ins and m["keep"][b] == ins
        probe = {1: [((1, 0, 0), True), ((1, 1, 0), False)], 2: [((2, 0, 0), True), ((2, 1, 0), False), ((1, 1, 1), True)],
                 3: [((3, 0, 0), True), ((3, 1, 0), False), ((2, 2, 1), True), ((2, 2, 2), False)],
                 4: [((4, 0, 0), True), ((4, 1, 0), False), ((2, 2, 2), True), ((3, 2, 2), False)]}[r]
        for off, ins in probe:
            j = int(np.flatnonzero((offs == off).all(1))[0])
            ok &= bool(inside[j]) == ins
        return bool(ok) and inside.sum() == B(r) - 1

    return (ijk, check)


def _threshold(r: int, k: int):
    """centre A with exactly k - 1 supporters, centre B with exactly k: A goes, B stays"""
    rng = np.random.default_rng([r, k])
    offs = ball_offsets(r)[rng.permutation(B(r) - 1)]
    a, b = np.array([3 * r + 2] * 3), np.array([3 * r + 2, 3 * r + 2, 3 * r + 2 + 4 * r + 4])
    ijk = np.concatenate([[a], a + offs[:k - 1], [b], b + offs[:k], [[0, 0, 0]]])

    def check(c, m):
        ra, rb = row_of(m, a), row_of(m, b)
        return (m["support"][ra] == k - 1 and not m["keep"][ra] and m["support"][rb] == k and m["keep"][rb]
                and (k < B(r) - 1 or m["support"][rb] == B(r) - 1))

    return _case(ijk, r, k, check)


def _wrap_pairs(cam1=False):
    """ny = 7, nz = 8 (>= 2 r + 2 for r = 2): (x, y, nz - 1) and (x, y + 1, 0) are adjacent bits and no neighbours, nor are
    (x, ny - 1, nz - 1) and (x + 1, 0, 0); a real pair beside them survives"""
    dim = (12, 7, 8)
    ijk = _with_pins([[2, 3, 7], [2, 4, 0], [5, 6, 7], [6, 0, 0], [9, 3, 3], [9, 3, 5]], dim)
    c = 1 if cam1 else 0

    def check(case, m):
        d = m["dims"][c]
        adj = (bit_of((2, 4, 0), d) - bit_of((2, 3, 7), d) == 1) and (bit_of((6, 0, 0), d) - bit_of((5, 6, 7), d) == 1)
        gone = all(not m["keep"][row_of(m, v, c)] and m["support"][row_of(m, v, c)] == 0
                   for v in ([2, 3, 7], [2, 4, 0], [5, 6, 7], [6, 0, 0]))
        return adj and gone and tuple(d) == dim and m["keep"][row_of(m, [9, 3, 3], c)] and m["keep"][row_of(m, [9, 3, 5], c)]

    return ijk, check


def _filled_box(cam1=False):
    """a filled 6 x 7 x 8 lattice at radius 2: a corner has the 10 neighbours of its octant, an edge, a face and the inside more;
    min_neighbors = 11 takes exactly the eight corners out -- a run that wrapped into the next row would keep them"""
    dim = (6, 7, 8)
    g = np.stack(np.meshgrid(*[np.arange(n) for n in dim], indexing="ij"), axis=-1).reshape(-1, 3)
    c = 1 if cam1 else 0

    def check(case, m):
        sel = m["cam"] == c
        v, keep, sup = m["ijk"][sel], m["keep"][sel], m["support"][sel]
        corner = ((v == 0) | (v == np.asarray(dim) - 1)).all(1)
        inner = ((v >= 2) & (v <= np.asarray(dim) - 3)).all(1)
        face = (v[:, 0] == 0) & ((v[:, 1:] >= 2) & (v[:, 1:] <= np.asarray(dim)[1:] - 3)).all(1)
        return (corner.sum() == 8 and (sup[corner] == 10).all() and np.array_equal(~keep, corner) and (sup[inner] == 32).all()
                and (sup[face] == 22).all() and face.any() and inner.any())

    return g, check


def _seams():
    """nz = 37, ny = 50, nx = 72: (70, 42, 17) and (70, 42, 18) are bits 131071 and 131072 -- the z-run of either straddles the
    4096-word block boundary; runs along z everywhere else straddle 32-bit words (37 is odd); isolated voxels go"""
    dim = (72, 50, 37)
    rng = np.random.default_rng(37)
    run = [[70, 42, z] for z in (16, 17, 18, 19)]
    blobs = []
    for ctr in rng.integers(3, [68, 47, 34], (40, 3)):
        blobs.append(ctr + ball_offsets(2)[rng.permutation(32)[:6]])
        blobs.append(ctr[None, :])
    lone = [[70, 45, 17], [69, 42, 30], [40, 0, 36], [41, 49, 0]]
    ijk = _with_pins(np.concatenate([run, lone] + blobs), dim)

    def check(case, m, c=0):
        d = m["dims"][c]
        rows = [row_of(m, v, c) for v in run]
        words = {bit_of(v, d) // 32 for v in m["ijk"][m["cam"] == c]}
        return (tuple(d) == dim and bit_of(run[1], d) == BLOCK_BITS - 1 and bit_of(run[2], d) == BLOCK_BITS
                and all(m["keep"][r] for r in rows) and [int(m["support"][r]) for r in rows] == [2, 3, 3, 2]
                and all(not m["keep"][row_of(m, v, c)] for v in lone) and len(words) > 50)

    return ijk, check


def _block_neighbours():
    """ny = 64, nz = 32 (64 x-layers are one block): the only supporter of (63, y, z) is (64, y, z), in the next block, and the
    other way round; (63, 40, 9) has none"""
    dim = (130, 64, 32)
    pairs = [[63, 5, 5], [64, 5, 5], [63, 63, 31], [64, 63, 31], [63, 0, 0], [64, 0, 0], [127, 20, 31], [128, 20, 31]]
    ijk = _with_pins(pairs + [[63, 40, 9], [64, 30, 9]], dim)

    def check(case, m, c=0):
        d = m["dims"][c]
        blocks = [bit_of(v, d) // BLOCK_BITS for v in pairs]
        return (blocks == [0, 1, 0, 1, 0, 1, 1, 2] and all(m["keep"][row_of(m, v, c)] and m["support"][row_of(m, v, c)] == 1 for v in pairs)
                and not m["keep"][row_of(m, [63, 40, 9], c)] and not m["keep"][row_of(m, [64, 30, 9], c)])

    return ijk, check


def _dense_block():
    """a 40 x 40 x 40 lattice (one block) 60 % filled -- more than 4096 set bits: the walk-your-own-words path -- with isolated
    voxels in holes cut for them"""
    rng = np.random.default_rng(40)
    occ = rng.random((40, 40, 40)) < 0.62
    lone = [(5, 5, 5), (20, 31, 7), (33, 12, 36), (11, 25, 20)]
    for v in lone:
        occ[tuple(slice(max(x - 2, 0), x + 3) for x in v)] = False
        occ[v] = True
    occ[0, 0, 0] = occ[39, 39, 39] = True
    ijk = np.argwhere(occ)

    def check(case, m):
        return (len(m["ijk"]) > 0.6 * 64000 and len(m["ijk"]) > LIST_CAP and all(not m["keep"][row_of(m, v)] for v in lone)
                and all(m["support"][row_of(m, v)] == 0 for v in lone) and m["keep"].mean() > 0.99)

    return _case(ijk, 2, 4, check)


def _degenerate(dim, r=2, k=3):
    """a lattice one or two voxels thin: a filled patch, whose rim has fewer neighbours than its middle, and isolated voxels"""
    dim = np.asarray(dim)
    g = np.stack(np.meshgrid(*[np.arange(min(n, 5)) for n in dim], indexing="ij"), axis=-1).reshape(-1, 3)
    ijk = _with_pins(g, dim)

    def check(case, m):
        return tuple(m["dims"][0]) == tuple(dim) and np.array_equal(m["support"], support_brute(m["ijk"], r))

    return _case(ijk, r, k, check)


def _last_word():
    """5 x 3 x 7 = 105 bits: the last word holds bits 96 .. 104, (4, 2, 6) the last of them, with two neighbours"""
    ijk = _with_pins([[4, 2, 5], [4, 1, 6], [2, 1, 3]], (5, 3, 7))

    def check(case, m):
        d = m["dims"][0]
        return (int(np.prod(d)) % 32 != 0 and bit_of((4, 2, 6), d) == 104 and m["keep"][row_of(m, (4, 2, 6))]
                and m["support"][row_of(m, (4, 2, 6))] == 2 and not m["keep"][row_of(m, (2, 1, 3))])

    return _case(ijk, 1, 2, check)


def _camera0_inside_camera1():
    """camera 1: a filled 5^3 cluster; camera 0: its corner and ONE voxel whose point lies in the middle of camera 1's cluster --
    it has no neighbour in its own lattice and goes, the cluster's inside stays"""
    g = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    mid = M.lattice([[2, 2, 2]], CELL, ORIGIN1)[0].astype(np.float64)  # the centre of camera 1's voxel (2, 2, 2) ...
    v0 = np.floor((mid - np.asarray(ORIGIN0)) / CELL)                    # ... seen from camera 0's lattice
    o0 = tuple(np.asarray(ORIGIN0) + np.minimum(v0, 0) * CELL)           # (its corner moved so that the voxel index is >= 0)
    v0 = np.floor((mid - np.asarray(o0)) / CELL).astype(np.int64)
    left = np.concatenate([M.corner(o0), mid.astype(F32)[None, :]])
    right = _points(g, ORIGIN1, 1)
    pts = np.ascontiguousarray(np.concatenate([left, right]), F32)

    def check(case, m):
        c0, c1 = m["cam"] == 0, m["cam"] == 1
        return (c0.sum() == 2 and not m["keep"][c0].any() and (m["support"][c0] == 0).all() and c1.sum() == 125
                and m["keep"][row_of(m, (2, 2, 2), 1)] and m["counts"].tolist()[:2] == [2, 125])

    return dict(points=pts, size_left=2, dense=True, workspace=np.asarray(WIDE, np.float64), cell=CELL, radius=2, min_neighbors=11,
                check=check)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {}
    for r in (1, 2, 3, 4):
        ijk, check = _ball_shape(r)
        out["ball_r%d" % r] = _case(ijk, r, 1, check)
    for r, k in ((1, 1), (1, 4), (1, 6), (2, 1), (2, 4), (2, 32), (3, 4), (3, 122), (4, 1), (4, 256)):
        out["threshold_r%d_k%d" % (r, k)] = _threshold(r, k)
    ijk, check = _wrap_pairs()
    out["wrap_pairs"] = _case(ijk, 2, 1, check)
    ijk, check = _filled_box()
    out["wrap_filled_box"] = _case(ijk, 2, 11, check)
    out["thin_nz1"] = _degenerate((9, 8, 1))
    out["thin_nz2"] = _degenerate((9, 8, 2))
    out["thin_ny1"] = _degenerate((9, 1, 8))
    out["one_voxel"] = dict(_case([[0, 0, 0]], 2, 1, lambda c, m: len(m["keep"]) == 1 and not m["keep"].any()), all_pruned=True)
    ijk, check = _seams()
    out["seams"] = _case(ijk, 2, 2, check)
    ijk, check = _block_neighbours()
    out["block_neighbours"] = _case(ijk, 1, 1, check)
    out["dense_block"] = _dense_block()
    out["last_word"] = _last_word()
    # the same in camera 1's lattice, behind a camera 0 of its own (word_ofs[1] != 0), and with no camera-0 point at all
    small0 = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [7, 3, 2]]
    for name, (ijk, check) in (("seams", _seams()), ("wrap_pairs", _wrap_pairs(True)), ("wrap_filled_box", _filled_box(True)),
                               ("block_neighbours", _block_neighbours())):
        chk = check if name.startswith("wrap") else (lambda c, m, f=check: f(c, m, 1))
        r, k = {"seams": (2, 2), "wrap_pairs": (2, 1), "wrap_filled_box": (2, 11), "block_neighbours": (1, 1)}[name]
        out["cam1_" + name] = _case(small0, r, k, chk, ijk1=ijk)
    ijk, check = _wrap_pairs(True)
    out["only_cam1_wrap_pairs"] = _case(None, 2, 1, check, ijk1=ijk)
    out["camera0_inside_camera1"] = _camera0_inside_camera1()
    return out


# ---- a raw capture with speckle, for the chains ----

SPECKLE = dict(radius=2, min_neighbors=4, cell=0.003, n_injected=400)  # (tests/test_voxel_filter_cases.py: >= 90 % / <= 1 %)


def inject(xyz, size_left, ws, n_injected, seed):
    """n_injected stray points, uniform in the box of each camera stretch's kept points and appended to that stretch; returns the
    points, the raw index where camera 1's stretch now starts, and the flags of the injected points"""
    rng = np.random.default_rng(seed)
    parts, flags = [], []
    for lo, hi in ((0, size_left), (size_left, len(xyz))):
        p = xyz[lo:hi]
        ok = M._kept(p, ws)
        stray = rng.uniform(p[ok].min(0), p[ok].max(0), (n_injected // 2, 3)).astype(F32)
        parts += [p, stray]
        flags += [np.zeros(len(p), bool), np.ones(len(stray), bool)]
    pts = np.ascontiguousarray(np.concatenate(parts), F32)
    pts.setflags(write=False)
    return pts, size_left + n_injected // 2, np.concatenate(flags)


@functools.lru_cache(maxsize=None)
def speckle_capture() -> dict:
    """tests/test_cpp_adapter.py's raw two-view capture (NaNs, points outside the workspace) with SPECKLE['n_injected'] stray
    points.  It runs with dense = 0: size_left is the RANK at which camera 1's stretch starts."""
    from tests.test_cpp_adapter import _raw_cloud

    xyz, size_left, ws, origins = _raw_cloud()
    pts, first_right, injected = inject(xyz, size_left, ws, SPECKLE["n_injected"], 400)
    return dict(points=pts, size_left=int(np.isfinite(pts[:first_right]).all(1).sum()), dense=False, workspace=ws,
                cell=SPECKLE["cell"], origins=origins, injected=injected, radius=SPECKLE["radius"],
                min_neighbors=SPECKLE["min_neighbors"])
