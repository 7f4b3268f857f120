"""Room-scale inputs for the grid build (csrc/grid.hip): boxes whose cell histogram needs more scan tiles than k_cell_scan has
work-groups (a second pass), boxes on and beyond the cell cap (the cell doubles), and sequences of builds on one context
that change the cell size (tests/test_grid_scale_clouds.py checks every case on the CPU, tests/test_gpu_grid_scale.py runs
them on the GPU).

Plain numpy, no GPU.  Every cloud is a real searchable scene (synthetic.config) plus SPARSE extra points that only shape the
box: two corner points whose coordinates are multiples of 2^-8 m (exact in float32, and their difference exact in double)
fix the dims, some hundreds of random points fill the room.  The random points keep more than r_hands + r_taubin from every
sample, so the searches see the plain scene; the cases that put samples among extra points say so.

The model below restates desc_finish / desc_next of grid.hip: float32 extrema in, double arithmetic, as written there.
"""
from __future__ import annotations

import dataclasses

import numpy as np

BASE_CELL = 0.02
CELL_CAP = 1 << 21    # kCellCap
SCAN_BLOCK = 4096     # kScanBlock: cells per scan tile
GRID_MARGIN = 2       # kGridMargin
SCAN_GROUPS_SINGLE, SCAN_GROUPS_BATCH = 256, 64  # work-groups of k_cell_scan per cloud
R_HANDS, R_TAUBIN = 0.08, 0.03
LATTICE = 1.0 / 256.0


def base_cell(r_hands=R_HANDS):
    return max(BASE_CELL, r_hands / 4.0)


@dataclasses.dataclass
class Desc:
    mn: tuple
    cell: float
    dim: tuple
    open: int = 0

    @property
    def ncell(self):
        return self.dim[0] * self.dim[1] * self.dim[2]

    @property
    def tiles(self):
        return -(-self.ncell // SCAN_BLOCK)

    def as_dict(self):
        return {"mn": tuple(float(v) for v in self.mn), "cell": float(self.cell), "dim": tuple(int(v) for v in self.dim),
                "open": int(self.open)}


def extrema(xyz):
    """float32 minima / maxima over the rows without a non-finite coordinate (None: no such row)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok = np.isfinite(xyz).all(1)
    if not ok.any():
        return None
    return xyz[ok].min(0), xyz[ok].max(0)


def desc_finish(ext, base):
    mn = np.zeros(3) if ext is None else ext[0].astype(np.float64)
    mx = np.zeros(3) if ext is None else ext[1].astype(np.float64)
    cell = float(base)
    while True:
        cnt = np.floor((mx - mn) / cell) + 1.0
        if cnt[0] * cnt[1] * cnt[2] <= float(CELL_CAP):
            break
        cell *= 2.0
    return Desc(tuple(mn), cell, tuple(int(c) for c in cnt))


def desc_next(u, ext, base, cold):
    """(open faces of the used descriptor `u`, the descriptor the next build keeps, True if `u` itself is kept)."""
    t = desc_finish(ext, base)
    any_pt = ext is not None
    opn = 0
    fits = (not cold) and any_pt and u.cell == t.cell
    if any_pt:
        inv = 1.0 / u.cell
        for a in range(3):
            if np.floor((float(ext[0][a]) - u.mn[a]) * inv) < 0.0:
                opn |= 1 << (2 * a)
            if np.floor((float(ext[1][a]) - u.mn[a]) * inv) > float(u.dim[a] - 1):
                opn |= 2 << (2 * a)
            fits = fits and u.dim[a] - t.dim[a] <= 4 * GRID_MARGIN
    if fits and not opn:
        return opn, Desc(u.mn, u.cell, u.dim), True
    m = GRID_MARGIN
    if float(t.dim[0] + 2 * m) * float(t.dim[1] + 2 * m) * float(t.dim[2] + 2 * m) > float(CELL_CAP):
        m = 0
    return opn, Desc(tuple(t.mn[a] - m * t.cell for a in range(3)), t.cell, tuple(d + 2 * m for d in t.dim)), False


class GridModel:
    """The grid state of one context over a sequence of builds: build(clouds) returns, per cloud, the descriptor the build
    uses (with its open faces) and its regime -- "cold", "kept" (used again next time), "refit" (covered, but the next build
    takes another descriptor) or "miss" (points beyond an open face) -- and `stats` follows agh_get_grid_stats."""

    def __init__(self, r_hands=R_HANDS):
        self.base = base_cell(r_hands)
        self.next = None
        self.stats = {"builds": 0, "cold": 0, "misses": 0}

    def build(self, clouds):
        cold = self.next is None or len(self.next) != len(clouds)
        out, nxt = [], []
        for k, xyz in enumerate(clouds):
            ext = extrema(xyz)
            u = desc_finish(ext, self.base) if cold else self.next[k]
            opn, n, kept = desc_next(u, ext, self.base, cold)
            out.append((Desc(u.mn, u.cell, u.dim, opn), "cold" if cold else ("miss" if opn else ("kept" if kept else "refit"))))
            nxt.append(n)
            self.stats["misses"] += 1 if opn else 0
        self.next = nxt
        self.stats["builds"] += 1
        self.stats["cold"] += 1 if cold else 0
        return out


def cell_index(d, xyz):
    """Cell of every point in descriptor `d` (cell_coord: multiply by 1 / cell, floor, clamp), x fastest."""
    inv = 1.0 / d.cell
    c = [np.clip(np.floor((np.asarray(xyz, np.float32)[:, a].astype(np.float64) - d.mn[a]) * inv), 0, d.dim[a] - 1).astype(np.int64)
         for a in range(3)]
    return (c[2] * d.dim[1] + c[1]) * d.dim[0] + c[0]


def crosses_cell_face(d, q, r=R_HANDS):
    """Per query point: does its ball of radius r reach into more than one cell of `d` along some axis?"""
    q = np.asarray(q, np.float32).astype(np.float64).reshape(-1, 3)
    out = np.zeros(len(q), bool)
    for a in range(3):
        lo = np.clip(np.floor((q[:, a] - r - d.mn[a]) / d.cell), 0, d.dim[a] - 1)
        hi = np.clip(np.floor((q[:, a] + r - d.mn[a]) / d.cell), 0, d.dim[a] - 1)
        out |= hi > lo
    return out


# ---- clouds ------------------------------------------------------------------------------------------------------------
def extent_for(dims, cell):
    """Box extents on the 2^-8 m lattice that give `dims` cells of size `cell`: half a cell inside the last one."""
    ext = np.round((np.asarray(dims, np.float64) - 0.5) * cell / LATTICE) * LATTICE
    assert (np.floor(ext / cell) + 1 == np.asarray(dims)).all()
    return ext


@dataclasses.dataclass
class Cloud:
    xyz: np.ndarray
    cam: np.ndarray
    samples: np.ndarray
    cam_origins: np.ndarray
    n_scene: int  # the first n_scene rows are the scene, the rest the extra points


def scene(name):
    from agile_grasp_amd import synthetic

    return synthetic.config(name)


def subset(sc, k, seed=5):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(sc.samples, size=min(k, sc.samples.size), replace=False)).astype(np.int32)


def boxed(sc, samples, ext, frac=(0.5, 0.5, 0.5), n_fill=600, seed=0, extra=()):
    """`sc` inside a box of extents `ext` (lattice multiples): the box's low corner lies on the lattice, `frac` of the free room
    below the scene along every axis.  Two corner points fix the box; n_fill random points fill it, none within
    r_hands + r_taubin of a sample; `extra` rows are appended as they are."""
    lo_s, hi_s = sc.xyz.min(0).astype(np.float64), sc.xyz.max(0).astype(np.float64)
    ext = np.asarray(ext, np.float64)
    free = ext - (hi_s - lo_s)
    assert (free > 2 * LATTICE).all(), "the box must hold the scene"
    lo = np.floor((lo_s - np.asarray(frac) * free) / LATTICE) * LATTICE
    hi = lo + ext
    assert (lo < lo_s).all() and (hi > hi_s).all()
    rng = np.random.default_rng(seed)
    fill = (lo + rng.random((n_fill, 3)) * ext).astype(np.float32)
    fill = np.clip(fill, lo.astype(np.float32), hi.astype(np.float32))
    q = sc.xyz[samples].astype(np.float64)
    far = np.ones(len(fill), bool)
    for i in range(0, len(fill), 256):
        d2 = ((fill[i:i + 256, None, :].astype(np.float64) - q[None]) ** 2).sum(2)
        far[i:i + 256] = (d2 > (R_HANDS + R_TAUBIN + 0.01) ** 2).all(1) if len(q) else True
    parts = [sc.xyz, np.stack([lo, hi]).astype(np.float32), fill[far]] + [np.asarray(e, np.float32).reshape(-1, 3) for e in extra]
    xyz = np.ascontiguousarray(np.concatenate(parts), np.float32)
    assert np.array_equal(xyz[sc.n].astype(np.float64), lo) and np.array_equal(xyz[sc.n + 1].astype(np.float64), hi)
    cam = np.concatenate([sc.cam, (rng.random(len(xyz) - sc.n) < 0.5).astype(np.int32)]).astype(np.int32)
    return Cloud(xyz, cam, np.asarray(samples, np.int32), sc.cam_origins, sc.n)


def plain(sc, samples):
    return Cloud(sc.xyz, sc.cam, np.asarray(samples, np.int32), sc.cam_origins, sc.n)


A_DIMS = (160, 120, 100)  # 1.92 M cells, 469 tiles: a second pass for 213 of the 256 work-groups


def case_a(n_samples=120):
    """Second pass at the base cell.  x is fastest in the cell index, so tile 256 begins in z layer 54 of 100: the scene is
    placed about that layer, and has points and samples in tiles on both sides."""
    sc = scene("small")
    ext = extent_for(A_DIMS, BASE_CELL)
    hz = float(sc.xyz[:, 2].max() - sc.xyz[:, 2].min())
    fz = (54.6 * BASE_CELL - hz / 2) / (ext[2] - hz)
    return boxed(sc, subset(sc, n_samples, 11), ext, frac=(0.3, 0.6, fz), seed=1)


def case_b(which, n_samples=64):
    """The cap edge: "fit" is 128 x 128 x 128 = 2^21 cells at the base cell, "over" one cell more along x (doubles)."""
    sc = scene("tiny")
    dims = (128, 128, 128) if which == "fit" else (129, 128, 128)
    # ("over" keeps the low corner of "fit" -- the same frac of a box one cell longer moves it by less than a lattice step
    # only by luck -- so the box is given by the "fit" corner and the longer extent)
    c = boxed(sc, subset(sc, n_samples, 12), extent_for((128, 128, 128), BASE_CELL), frac=(0.4, 0.5, 0.5), seed=2)
    if which != "fit":
        c.xyz[c.n_scene + 1] = c.xyz[c.n_scene] + extent_for(dims, BASE_CELL).astype(np.float32)
    return c


C_CELLS = {"0.04": 0.04, "0.08": 0.08}
C_DIMS = (150, 125, 88)  # at the doubled cell (the 6 x 5 x 3.5 m room at 0.04)


def case_c(which, n_samples=100):
    """Doubled cells, each built cold.  "0.04" / "0.08": rooms of 150 x 125 x 88 cells of that size.  "1.28-one" / "1.28-two":
    one far point at (100, 100, 100); the scene lies in one cell, or (a second extra point, one cell below the samples' median
    along x) in two."""
    sc = scene("small")
    s = subset(sc, n_samples, 13)
    if which in C_CELLS:
        return boxed(sc, s, extent_for(C_DIMS, C_CELLS[which]), frac=(0.45, 0.5, 0.4), n_fill=2000, seed=3)
    pts = [[100.0, 100.0, 100.0]]
    if which == "1.28-two":
        lo = np.floor(sc.xyz.min(0).astype(np.float64) / LATTICE) * LATTICE
        mid = np.floor(float(np.median(sc.xyz[s, 0])) / LATTICE) * LATTICE  # the cell face x = mid goes through the samples
        pts.append([mid - 1.28, lo[1], lo[2]])
    xyz = np.ascontiguousarray(np.concatenate([sc.xyz, np.array(pts, np.float32)]), np.float32)
    cam = np.concatenate([sc.cam, np.zeros(len(pts), np.int32)]).astype(np.int32)
    return Cloud(xyz, cam, s, sc.cam_origins, sc.n)


D_SHIFT = np.array([0.0, 0.13, 0.10], np.float32)


def case_d(n_samples=100):
    """Transitions on one context: (table, room).  The room is the table scene, a copy of it moved by D_SHIFT -- dense points
    beyond the y and z faces of the table's kept box, for samples among them -- and a sparse 0.04 m room around both."""
    sc = scene("small")
    s = subset(sc, n_samples, 14)
    room = boxed(sc, s, extent_for(C_DIMS, 0.04), frac=(0.5, 0.45, 0.5), n_fill=1500, seed=4, extra=[sc.xyz + D_SHIFT])
    return plain(sc, s), room


E_R_HANDS = 0.1


def case_e(n_samples=100):
    """nn_radius_hands = 0.1: a base cell of 0.025 m, and a room that doubles once from there, to 0.05 m."""
    sc = scene("small")
    return boxed(sc, subset(sc, n_samples, 15), extent_for(C_DIMS, 0.05), frac=(0.5, 0.5, 0.5), n_fill=2000, seed=5)


F_C4_DIMS = (120, 72, 80)    # C4's extents: 169 tiles
F_C2X_DIMS = (104, 84, 83)   # the largest box of the older suite: 178 tiles


def case_f(n, n_samples=40):
    """A batch of n = 2 or 8 clouds.  Among them: more than 256 tiles, more than 64 (twice in the batch of 8), a doubled cell,
    a far outlier, `tiny`, a plain scene and an empty cloud."""
    small, tiny = scene("small"), scene("tiny")
    a = boxed(small, subset(small, n_samples, 21), extent_for(A_DIMS, BASE_CELL), frac=(0.5, 0.5, 0.45), seed=6)
    c4 = boxed(tiny, subset(tiny, n_samples, 22), extent_for(F_C4_DIMS, BASE_CELL), frac=(0.3, 0.5, 0.6), seed=7)
    if n == 2:
        return [a, c4]
    room = boxed(small, subset(small, n_samples, 23), extent_for(C_DIMS, 0.04), frac=(0.5, 0.5, 0.5), n_fill=1500, seed=8)
    c2x = boxed(small, subset(small, n_samples, 24), extent_for(F_C2X_DIMS, BASE_CELL), frac=(0.6, 0.4, 0.5), seed=9)
    far = case_c("1.28-two", n_samples)
    empty = Cloud(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), small.cam_origins, 0)
    return [c4, a, room, plain(tiny, subset(tiny, n_samples, 25)), empty, plain(small, subset(small, n_samples, 26)), c2x, far]


F_MOVE = np.array([-0.4, 0.25, 0.3], np.float32)
F_MOVED = {2: 1, 8: 0}  # the large cloud of each batch that the third build translates (the C4-sized one)


G_WORKSPACE = np.array([-2.75, 3.75, -3.0, 3.0, -3.0, 3.0])
G_DIMS = ((70, 70, 70), A_DIMS, C_DIMS)  # per capture: at 0.08 m, at the base cell (a second pass), at 0.04 m
G_CELLS = (0.08, BASE_CELL, 0.04)


def case_g(n_fill=1200):
    """Three raw captures for the fused chains, inside a workspace of +-3 m: a tabletop capture each (synthetic.make_raw_cloud)
    plus sparse room points in the left camera's block.  The voxeliser moves every point by less than a voxel, so the
    boxes are close to G_DIMS cells of G_CELLS; the tests take the exact figures from the voxelised cloud."""
    from agile_grasp_amd import synthetic

    out = []
    for k, (dims, cell) in enumerate(zip(G_DIMS, G_CELLS)):
        rc = synthetic.make_raw_cloud(40_000, seed=31 + k)
        ext = extent_for(dims, cell)
        lo_s, hi_s = np.nanmin(rc.xyz, 0).astype(np.float64), np.nanmax(rc.xyz, 0).astype(np.float64)
        lo = np.floor((lo_s - 0.5 * (ext - (hi_s - lo_s))) / LATTICE) * LATTICE
        assert (lo > G_WORKSPACE[0::2] + 0.01).all() and (lo + ext < G_WORKSPACE[1::2] - 0.01).all()
        rng = np.random.default_rng(40 + k)
        fill = np.concatenate([np.stack([lo, lo + ext]), lo + rng.random((n_fill, 3)) * ext]).astype(np.float32)
        # (all of them in the left camera's block: the voxeliser's two per-camera lattices share 2^33 cells, and two lattices
        # of the 5.6 m room would need 1.3e10)
        xyz = np.ascontiguousarray(np.concatenate([rc.xyz[:rc.size_left], fill, rc.xyz[rc.size_left:]]), np.float32)
        out.append(synthetic.RawCloud(xyz, rc.size_left + len(fill), G_WORKSPACE.copy(), rc.cam_origins))
    return out


def case_h(which, n_samples=64):
    """Extreme but finite: "1e6" one point a million metres out, "1e30" two points at +-1e30 m along every axis, "mixed" the
    1e30 pair and 1 % non-finite rows (as test_gpu_grid_kept.test_non_finite_points makes them)."""
    sc = scene("tiny")
    s = subset(sc, n_samples, 16)
    pts = {"1e6": [[1e6, -1e6, 1e6]], "1e30": [[1e30, 1e30, 1e30], [-1e30, -1e30, -1e30]],
           "mixed": [[1e30, 1e30, 1e30], [-1e30, -1e30, -1e30]]}[which]
    xyz = np.ascontiguousarray(np.concatenate([sc.xyz, np.array(pts, np.float32)]), np.float32)
    cam = np.concatenate([sc.cam, np.zeros(len(pts), np.int32)]).astype(np.int32)
    if which == "mixed":
        rng = np.random.default_rng(7)
        bad = np.setdiff1d(rng.permutation(sc.n)[: sc.n // 100], s)
        q = bad.size // 4
        xyz[bad[:q], rng.integers(0, 3, q)] = np.nan
        xyz[bad[q:2 * q]] = np.inf
        xyz[bad[2 * q:3 * q], 1] = -np.inf
        xyz[bad[3 * q:]] = np.nan
        s = np.unique(np.concatenate([s, bad[:8]])).astype(np.int32)
    return Cloud(xyz, cam, s, sc.cam_origins, sc.n)
