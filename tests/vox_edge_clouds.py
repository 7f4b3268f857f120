"""Captures at the voxeliser's launch-shape limits (agile_grasp_amd/csrc/voxelize.hip), and a numpy model of its bitmap layout
(numpy only).  tests/test_vox_edge_clouds.py proves on the CPU that every case reaches the path it is named for;
tests/test_gpu_vox_edges.py holds the GPU to the references on them, bit for bit.

The layout, as voxelize.hip documents it: per camera a bitmap over the lattice of the kept points, x-major and z-fastest (bit =
(ix * ny + iy) * nz + iz), in 32-bit words, rounded up to whole blocks of 4096 words; camera 1 starts on a block boundary.  The raw
points are counted in blocks of 1024 (k_vox_count), the counts are scanned 1024 per pass by one work-group (k_vox_scan), and the
camera id of a point is (rank >= size_left): its rank among the finite points for dense = 0, its raw index for dense = 1.

  raw_block_counts / lattice_words / block_popcounts    the model
  raw_scan_case       (a) clouds around 2^20 points (the scan's second pass) and their small twins, with the tested size_left
  emit_cases          (b) blocks of the bitmap at 4095 / 4096 / 4097 set bits (kListCap of k_vox_emit), dense next to sparse
  limit_cases         (c) lattices of exactly 2^28 words (kVoxMaxWords), and one step beyond
  batch_mixes         (d) captures of very different sizes in one agh_localize_batch

A case is a dict: `points` ((N, 3) float32), `size_left`, `dense`, `workspace`, `cell`.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import mask_cases as M

F32 = np.float32
RAW_BLOCK = 1024            # raw points per block of k_vox_count / k_vox_classify
SCAN_PASS = 1024            # block counts per pass of k_vox_scan
WORDS_PER_BLOCK = 4096      # bitmap words per block of k_vox_popcount / k_vox_emit
BLOCK_BITS = WORDS_PER_BLOCK * 32
LIST_CAP = 4096             # k_vox_emit lists a block's set bits in LDS up to this many
MAX_WORDS = 1 << 28         # kVoxMaxWords
M20 = 1 << 20               # the raw points one pass of k_vox_scan covers

RAW_CELL = 0.003
EMIT_CELL = 0.01
LIMIT_CELL = 2.0 ** -8
WIDE = M.WIDE


# ---- the model ----

def raw_block_counts(xyz, dense=False) -> np.ndarray:
    """The points k_vox_classify ranks per block of 1024 raw points: the finite ones (k_vox_count), or all for dense = 1."""
    p = np.asarray(xyz, F32)[:, :3]
    ok = np.ones(len(p), bool) if dense else np.isfinite(p).all(1)
    nb = (len(p) + RAW_BLOCK - 1) // RAW_BLOCK
    return np.bincount(np.arange(len(p)) // RAW_BLOCK, weights=ok, minlength=nb).astype(np.int64)


def scan_carries(counts) -> np.ndarray:
    """What k_vox_scan carries into pass 1, 2, ...: the sum of the first 1024, 2048, ... block counts."""
    c = np.cumsum(np.asarray(counts, np.int64))
    return c[SCAN_PASS - 1::SCAN_PASS][:(len(c) - 1) // SCAN_PASS]


def _cams(points, cams_or_size_left, dense):
    if np.ndim(cams_or_size_left) == 0:
        return M.camera_ids(points, int(cams_or_size_left), dense)
    return np.asarray(cams_or_size_left)


def lattice_words(points, cams_or_size_left, workspace, cell, dense=False) -> int:
    """The words of the capture's voxel bitmap: per camera the lattice's bits in words, rounded up to whole blocks."""
    words = 0
    for _sel, _cam, _pos, dim in M.bit_positions(points, _cams(points, cams_or_size_left, dense), workspace, cell):
        w = (int(dim[0]) * int(dim[1]) * int(dim[2]) + 31) // 32
        words += (w + WORDS_PER_BLOCK - 1) // WORDS_PER_BLOCK * WORDS_PER_BLOCK
    return words


def block_popcounts(points, cams_or_size_left, workspace, cell, dense=False) -> np.ndarray:
    """The set bits per 4096-word block of the bitmap, camera 0's blocks first."""
    out = []
    for _sel, _cam, pos, dim in M.bit_positions(points, _cams(points, cams_or_size_left, dense), workspace, cell):
        bits = int(dim[0]) * int(dim[1]) * int(dim[2])
        out.append(np.bincount(np.unique(pos) // BLOCK_BITS, minlength=(bits + BLOCK_BITS - 1) // BLOCK_BITS))
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


def case(points, size_left=None, dense=False, workspace=WIDE, cell=EMIT_CELL, **more) -> dict:
    points = np.ascontiguousarray(points, F32)
    points.setflags(write=False)
    return dict(points=points, size_left=len(points) if size_left is None else int(size_left), dense=bool(dense),
                workspace=np.asarray(workspace, np.float64), cell=cell, **more)


def records(points, pad=5) -> np.ndarray:
    """The points as 32-byte records (pcl::PointXYZRGBA-like), the padding non-zero."""
    return np.ascontiguousarray(np.concatenate([points, np.full((len(points), pad), 7.0, F32)], axis=1))


# ---- (a) the raw scan and the camera-switch rank ----

RAW_BIG = (M20 - 1, M20, M20 + 1, M20 + 1025, M20 + 1324)  # 1024, 1024, 1025, 1026 and 1026 raw blocks
RAW_TWINS = (1023, 1024, 1025, 2049)
_ENDS, _B1023, _CARRY = ("zero", "all_left", "beyond"), ("block1023-1", "block1023", "block1023+1"), ("carry-1", "carry", "carry+1")
RAW_BIG_SIZES = {M20 - 1: _ENDS + _B1023, M20: _ENDS + _B1023, M20 + 1: _ENDS + _B1023 + _CARRY[:1],
                 M20 + 1025: _ENDS + _CARRY + ("block1025",), M20 + 1324: _ENDS + _CARRY + ("mid_wave",)}  # the names in `sizes`
RAW_WORKSPACE = np.array([-0.05, 1.0, -1.0, 1.0, -1.0, 1.0])  # (cuts a slice off the cube: a dropped point keeps its rank)
NAN_BLOCK, FULL_BLOCK = 5, 7  # raw blocks of the large clouds without a finite point / without a NaN
MID_WAVE = 1025 * RAW_BLOCK + 2 * 64 + 29  # raw index: block 1025, wave 2, lane 29
MARKER_WINDOW = 64


def _bad_rows(rng, k):
    """k records the NaN removal drops: NaN in one coordinate, +-inf in one, all NaN"""
    rows = rng.uniform(-0.05, 0.05, (k, 3)).astype(F32)
    kind = rng.integers(0, 4, k)
    rows[kind == 0, 0] = np.nan
    rows[kind == 1, 1] = np.nan
    rows[kind == 2, 2] = np.where(rng.random(int((kind == 2).sum())) < 0.5, np.inf, -np.inf)
    rows[kind == 3] = np.nan
    return rows


@functools.lru_cache(maxsize=6)
def raw_scan_case(n: int, dense: bool = False) -> dict:
    """A cloud of n raw points for the first scan and the rank behind it, and the size_left values to run it with.

    The rows are drawn with replacement from 3000 points of a +-6 cm cube, so that the voxelised cloud stays small; about 1 % are
    NaN or inf records.  A large cloud has one raw block without a finite point and one without a NaN, and, for dense = 0, NaNs at
    raw 2^20 - 1 and 2^20, the last point of the scan's first pass and the first of its second.  (For dense = 1 those two stay
    finite: there the rank is the raw index, and a switch at 2^20 would otherwise move nothing.)  A twin has NaNs ahead of every
    edge it tests.

    `sizes`: name -> size_left.  A rank for dense = 0, a raw index for dense = 1.
      zero, all_left, beyond   no point in camera 0, every point in camera 0, a value past the last rank
      carry-1, carry, carry+1  the rank of the first finite point of raw block 1024: what k_vox_scan's first pass carries into
                               its second (n > 2^20; for n = 2^20 + 1 block 1024 is the NaN alone and the carry is all_left)
      block1023-1, ...         the last count of the first pass (n <= 2^20: the scan has one pass)
      block1025, mid_wave      the only point of block 1025 (n = 2^20 + 1025); lane 29 of wave 2 of block 1025 (n = 2^20 + 1324:
                               at 2^20 + 1025 block 1025 holds one point and has no wave to be in the middle of)
      rank63 ... rank1025      (twins) the switch at ranks 63 / 64 / 65, 255 / 256 / 257, 1023 / 1024 / 1025
      raw64-1 ... raw1024+1    (twins) the switch at the point of raw index 64 / 256 / 1024 -- the first lane of a wave, of a
                               round and of a block of k_vox_classify -- whose rank the NaNs ahead of it have lowered
    The finite points with a rank within 64 of a tested size_left are markers: each is moved to a voxel of its own on a sheet
    outside the cube (two cells apart, so whatever the camera's minimum), and a rank off by one changes both cameras' voxels."""
    rng = np.random.default_rng([n, int(dense), 77])
    big = n >= M20 - 1
    base = rng.uniform(-0.06, 0.06, (3000, 3)).astype(F32)
    pts = base[rng.integers(0, len(base), n)]
    bad = rng.random(n) < 0.01
    if big:
        bad[NAN_BLOCK * RAW_BLOCK:(NAN_BLOCK + 1) * RAW_BLOCK] = True
        bad[FULL_BLOCK * RAW_BLOCK:(FULL_BLOCK + 1) * RAW_BLOCK] = False
    else:
        bad[[2, 3, 17, 40, 41, 61, 200, 230, 253, 900, 1000, 1021]] = True  # ahead of the edges, outside their windows below
    # the raw indices the switch is tested at, and what has to be finite around them
    at_raw = {}
    if big:
        if n > M20 + 1:
            at_raw["carry"] = M20 + (0 if dense else 1)
        else:
            at_raw["block1023"] = 1023 * RAW_BLOCK
        if n == M20 + 1025:
            at_raw["block1025"] = 1025 * RAW_BLOCK
        if n > MID_WAVE + 64:
            at_raw["mid_wave"] = MID_WAVE
    else:
        for r in (64, 256, 1024):
            if r + 1 <= n:
                at_raw["raw%d" % r] = r
    for r in at_raw.values():
        bad[max(r - 2, 0):min(r + 2, n)] = False
    if dense:  # (the two ends as well: there the switch at 0 and at n moves the first and the last raw point)
        bad[:2] = bad[n - 2:] = False
    if big and not dense:
        bad[M20 - 1:M20 + 1] = True  # (the slice ends with the cloud)
    pts[bad] = _bad_rows(rng, int(bad.sum()))
    fin = ~bad
    nf = int(fin.sum())
    rank_of_raw = np.cumsum(fin) - fin  # finite points ahead of each raw index
    top = n if dense else nf  # the first size_left that leaves camera 1 empty
    sizes = {"zero": 0, "all_left": top, "beyond": top + 1000}
    for name, r in at_raw.items():
        s = r if dense else int(rank_of_raw[r])
        if name in ("block1025", "mid_wave"):
            sizes[name] = s
        else:
            sizes.update({name + "-1": s - 1, name: s, name + "+1": s + 1})
    if big and n == M20 + 1:
        sizes["carry-1"] = top - 1  # (block 1024 is one NaN for dense = 0, one point for dense = 1: the carry is `top` or top - 1)
    if not big:
        for s in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
            if s + 1 <= top:
                sizes["rank%d" % s] = s
    seen = set()
    sizes = {k: v for k, v in sizes.items() if not (v in seen or seen.add(v))}  # (one name per value: the first)
    # markers: the finite points whose rank (raw index for dense = 1) is within the window of a tested size_left
    order = np.arange(n) if dense else np.flatnonzero(fin)
    near = np.zeros(len(order) + 1, bool)
    for s in sizes.values():
        near[max(s - MARKER_WINDOW, 0):min(s + MARKER_WINDOW, len(order))] = True
    mark = order[np.flatnonzero(near[:len(order)])]
    mark = mark[fin[mark]]
    j = np.arange(len(mark))
    sheet = np.stack([0.1 + 2 * RAW_CELL * (j % 32), 0.1 + 2 * RAW_CELL * (j // 32), np.full(len(j), 0.1)], axis=1)
    pts[mark] = sheet.astype(F32)
    return case(pts, 0, dense, RAW_WORKSPACE, RAW_CELL, sizes=sizes, n_finite=nf, markers=mark)


def moved_point_is_kept(c: dict, s: int) -> bool:
    """Whether raising size_left from s to s + 1 moves a kept point (one that reaches the voxels) from camera 1 to camera 0."""
    p = c["points"]
    order = np.arange(len(p)) if c["dense"] else np.flatnonzero(np.isfinite(p).all(1))
    return 0 <= s < len(order) and bool(M._kept(p[order[s]:order[s] + 1], c["workspace"])[0])


# ---- (b) the emit list cap ----

def _pick(rng, lo, hi, k, ny=64, nz=32, without=()):
    """k distinct voxels with ix in [lo, hi), none of them in `without`"""
    taken = {tuple(v) for v in without}
    flat = rng.permutation((hi - lo) * ny * nz)
    out = []
    for f in flat:
        v = (lo + int(f) // (ny * nz), int(f) // nz % ny, int(f) % nz)
        if v not in taken:
            out.append(v)
            if len(out) == k:
                break
    assert len(out) == k
    return out


def _emit_points(rng, ijk, origin=(0.25, 0.25, 0.25)):
    """the corner point (voxel (0, 0, 0), which pins the minimum) and the centres of `ijk` (without (0, 0, 0)), shuffled"""
    assert (0, 0, 0) not in {tuple(v) for v in ijk}
    pts = np.concatenate([M.corner(origin), M.lattice(np.asarray(ijk), EMIT_CELL, origin)])
    return pts[rng.permutation(len(pts))]


@functools.lru_cache(maxsize=None)
def emit_cases() -> dict:
    """name -> case, cell 1 cm.  ny = 64 and nz = 32: 64 x-layers are exactly one block of 4096 words (131 072 bits)."""
    rng = np.random.default_rng(4096)
    far = (63, 63, 31)
    out = {}
    for k in (LIST_CAP - 1, LIST_CAP, LIST_CAP + 1):  # one block, K set bits with the corner and the far corner among them
        out["k%d" % k] = case(_emit_points(rng, [far] + _pick(rng, 0, 64, k - 2, without=[(0, 0, 0), far])))
    # 4097 bits in the first 1024 words of the block (ix < 16): waves 1 to 3 of k_vox_emit count nothing
    pin = (15, 63, 31)
    out["first_quarter"] = case(_emit_points(rng, [pin] + _pick(rng, 0, 16, LIST_CAP - 1, without=[(0, 0, 0), pin])))
    # 4097 bits in the last 1024 words of block 1 (112 <= ix < 128): waves 0 to 2 count nothing.  (The corner is the one bit of
    # block 0: a lattice's first block always holds its minimum.)
    pin = (127, 63, 31)
    out["last_quarter"] = case(_emit_points(rng, [pin] + _pick(rng, 112, 128, LIST_CAP, without=[pin])))
    # camera 0: 4097 voxels in block 0; camera 1: 100 voxels of a lattice of its own, in block 1
    left = _emit_points(rng, [far] + _pick(rng, 0, 64, LIST_CAP - 1, without=[(0, 0, 0), far]))
    right = _emit_points(rng, [far] + _pick(rng, 0, 64, 98, without=[(0, 0, 0), far]), origin=(0.1, 0.3, 0.2))
    out["two_cameras"] = case(np.concatenate([left, right]), size_left=len(left))
    # one camera over three blocks: sparse, dense or exactly at the cap, sparse; the last bit of block 1 and the first of block 2
    for name, k in (("three_blocks", 5000), ("three_blocks_cap", LIST_CAP)):
        edge = [(127, 63, 31), (128, 0, 0), (191, 63, 31)]
        ijk = (_pick(rng, 0, 64, 49, without=[(0, 0, 0)]) + edge[:1] + _pick(rng, 64, 128, k - 1, without=edge)
               + edge[1:] + _pick(rng, 128, 192, 60, without=edge))
        out[name] = case(_emit_points(rng, ijk))
    return out


# ---- (c) the lattice size limit ----

LIMIT_ORIGIN = (-4.0, -4.0, -4.0)


def _limit_points(ijk, origin=LIMIT_ORIGIN):
    """the corner and the centres of `ijk`: at 2^-8 m cells every coordinate is a multiple of 2^-9, exact in float32 and double"""
    pts = np.concatenate([M.corner(origin), M.lattice(np.asarray(ijk), LIMIT_CELL, origin)])
    assert np.array_equal(pts.astype(np.float64) * 512, np.round(pts.astype(np.float64) * 512))
    return pts


@functools.lru_cache(maxsize=None)
def limit_cases() -> dict:
    from agile_grasp_amd import synthetic

    rng = np.random.default_rng(33)
    out = {}
    rand = [tuple(int(x) for x in v) for v in rng.integers(1, 2047, (5, 3))]
    one = [(2047, 2047, 2047), (2047, 2047, 2046), (2047, 0, 0), (1024, 0, 0), (1024, 0, 1), (1023, 2047, 2047)] + rand
    out["fits_one"] = case(_limit_points(one), cell=LIMIT_CELL)  # 2048^3 bits: exactly 2^28 words, the top voxel is bit 2^33 - 1
    out["over_one"] = case(_limit_points(one + [(2048, 5, 5)]), cell=LIMIT_CELL)  # 2049 x 2048 x 2048
    # both cameras 2048 x 2048 x 1024: 2^27 words each; camera 1's lattice is its own (another origin)
    half = [(2047, 2047, 1023), (2047, 2047, 1022), (2047, 0, 0), (1024, 0, 0), (1024, 0, 1), (1023, 2047, 1023)]
    half += [(x, y, z // 2) for x, y, z in rand]
    o1 = (-3.0, -2.5, 1.0)
    left = _limit_points(half)
    out["fits_two"] = case(np.concatenate([left, _limit_points(half, o1)]), size_left=len(left), cell=LIMIT_CELL)
    out["over_two"] = case(np.concatenate([left, _limit_points(half + [(7, 7, 1024)], o1)]), size_left=len(left), cell=LIMIT_CELL)
    rc = synthetic.make_raw_cloud(20_000, 5)
    out["after_big"] = case(rc.xyz, rc.size_left, False, rc.workspace, 0.003)
    return out


# ---- (d) batches ----

@functools.lru_cache(maxsize=None)
def batch_mixes() -> dict:
    """name -> list of (capture name, case, size_left): the captures of one agh_localize_batch (one cell size per batch)"""
    rng = np.random.default_rng(5)
    big, twin, dense = raw_scan_case(M20 + 1025), raw_scan_case(1025), raw_scan_case(2049, True)
    raw = dict(workspace=RAW_WORKSPACE, cell=RAW_CELL)
    sizes = [("big", big, big["sizes"]["carry"]),
             ("one_point", case(np.array([[0.01, -0.02, 0.03]], F32), **raw), 1),
             ("empty", case(np.zeros((0, 3), F32), **raw), 0),
             ("all_nan", case(_bad_rows(rng, 300), **raw), 100),
             ("dense", dense, dense["sizes"]["raw1024"]),
             ("twin", twin, twin["sizes"]["raw1024"])]
    e = emit_cases()
    emit = [(n, e[n], e[n]["size_left"]) for n in ("k4097", "k4095", "three_blocks")]
    return {"sizes": sizes, "emit": emit}
