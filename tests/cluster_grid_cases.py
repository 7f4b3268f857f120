"""Captures that take the cluster stage (csrc/sample_cluster.hip) to where the search grid changes shape, and a numpy restatement
of what k_cluster_link derives from the grid's descriptor (numpy only).  tests/test_cluster_grid_cases.py proves every case's
regime on the CPU, tests/test_gpu_cluster_grid.py runs them.

A case is a dict as tests/cluster_cases.py makes them (`points`, `size_left`, `dense`, `workspace`, `cell`, `cp`).  Voxels are
placed with mask_cases.lattice on the case's own voxel size, both cameras pinned by a point at the case's origin; the support
plane is z = the origin's z, so a voxel's height is its k times the voxel size.  The reference stays cluster_cases.cluster_model:
brute-force float32 d2 over all pairs, no cell structure.

  link_regime      reach, owners / foreground / candidates per 2-cell group and the cell offset of every adjacent pair, from a
                   voxel cloud, a grid_scale_clouds.Desc and the cluster parameters
  faulty_model     cluster_model with the pairs a plausible fault of k_cluster_link would lose taken out
  cases            the single-call cases, each built cold
  sequence         the calls of one context: cold, miss with open faces, kept, the doubled room, back
  depth_steps      two depth captures for one context (a small one, then one that leaves its box), and a doubled one
  bitmap_chain_runs  how often each call of a sequence runs its chain (the voxel bitmap's sizing rule of agh_preprocess)
"""
import functools

import numpy as np

from tests import cluster_cases as CC
from tests import depth_captures as D
from tests import grid_scale_clouds as gs
from tests import mask_cases as M

F32 = np.float32
ORIGIN = CC.ORIGIN
GROUP_X, TILE, MAX_REACH = 2, 256, 3  # kClusterGroupX, kClusterTile, kClusterReach


# ---- what k_cluster_link derives from the descriptor -------------------------------------------------------------------------
def reach_of(tolerance: float, cell: float) -> int:
    """min(floor(tolerance * inv_cell * 1.0001) + 1, kClusterReach), in double as the kernel has it"""
    return min(int(np.floor(np.float64(tolerance) * (1.0 / np.float64(cell)) * 1.0001)) + 1, MAX_REACH)


def cell_coords(d, xyz, clamp=True):
    """(N, 3) cell coordinates in descriptor `d` (cell_coord of the library: multiply by 1 / cell, floor, clamp)"""
    inv = 1.0 / d.cell
    c = np.stack([np.floor((np.asarray(xyz, F32)[:, a].astype(np.float64) - d.mn[a]) * inv) for a in range(3)], 1)
    if clamp:
        c = np.clip(c, 0, np.asarray(d.dim, np.float64) - 1)
    return c.astype(np.int64)


def link_regime(xyz, d, cp) -> dict:
    """reach; per non-empty group (GROUP_X cells along x of one (y, z) row) `owners`, `owners_fg`, `first_cell` /
    `first_cell_fg` (its first cell's voxels) and `candidates` (the voxels of the cells within reach); per adjacent pair (a < b,
    voxel indices) `offsets` = cell of b - cell of a, and `clamped`, per voxel, true where cell_coord clamped it."""
    xyz = np.ascontiguousarray(xyz, F32)
    reach = reach_of(cp["tolerance"], d.cell)
    cc = cell_coords(d, xyz)
    clamped = (cell_coords(d, xyz, clamp=False) != cc).any(1)
    fgm = CC.foreground(xyz, cp)
    dim = np.asarray(d.dim, np.int64)
    counts = np.zeros(tuple(dim), np.int64)
    np.add.at(counts, (cc[:, 0], cc[:, 1], cc[:, 2]), 1)
    counts_fg = np.zeros(tuple(dim), np.int64)
    np.add.at(counts_fg, (cc[fgm, 0], cc[fgm, 1], cc[fgm, 2]), 1)
    gx = -(-int(dim[0]) // GROUP_X)
    pad = np.zeros((gx * GROUP_X,) + tuple(dim[1:]), np.int64)
    pad[:dim[0]] = counts
    own = pad.reshape(gx, GROUP_X, dim[1], dim[2]).sum(1)
    pad_fg = np.zeros_like(pad)
    pad_fg[:dim[0]] = counts_fg
    own_fg = pad_fg.reshape(gx, GROUP_X, dim[1], dim[2]).sum(1)
    groups = np.argwhere(own > 0)
    # candidates: the cells x0 - reach .. x1 + reach - 1 of the (2 reach + 1)^2 rows around the group, by a summed-area table
    sat = np.zeros(tuple(dim + 1), np.int64)
    sat[1:, 1:, 1:] = counts.cumsum(0).cumsum(1).cumsum(2)

    def box(lo, hi):
        lo, hi = np.clip(lo, 0, dim), np.clip(hi, 0, dim)
        (x0, y0, z0), (x1, y1, z1) = lo.T, hi.T
        return (sat[x1, y1, z1] - sat[x0, y1, z1] - sat[x1, y0, z1] - sat[x1, y1, z0] + sat[x0, y0, z1] + sat[x0, y1, z0]
                + sat[x1, y0, z0] - sat[x0, y0, z0])

    g0 = groups * np.array([GROUP_X, 1, 1])
    cand = box(g0 - reach, g0 + np.array([GROUP_X, 1, 1]) + reach)
    fg, a, b = CC.adjacent_pairs(xyz, cp)
    at = tuple(groups.T)
    return dict(reach=reach, groups=groups, owners=own[at], owners_fg=own_fg[at], first_cell=pad[::GROUP_X][at],
                first_cell_fg=pad_fg[::GROUP_X][at], candidates=cand, pairs=(fg, a, b), offsets=cc[fg[b]] - cc[fg[a]],
                clamped=clamped, cells=cc)


def x_window(cx, reach: int):
    """first and last cell along x of the candidate runs of the group that owns cell cx (before they are clipped to the grid)"""
    x0 = cx - cx % GROUP_X
    return x0 - reach, x0 + GROUP_X + reach - 1


FAULTS = ("two_cells", "clamped_dropped", "first_tile", "plus_side_short", "minus_side_short")


def faulty_model(xyz, d, cp, fault: str, axes=(0, 1, 2)) -> dict:
    """cluster_model of the pairs that are left when k_cluster_link had the fault:
      two_cells         a window of at most 2 cells per axis where the reach is 3
      clamped_dropped   a pair with an end outside the descriptor's box is not found (a geometric window, no open faces)
      first_tile        only the first 256 owners of a group link (owners ordered by cell, then by voxel index -- within a cell
                        the sorted array's order is the scatter's, so the cases keep whole cells on one side of the cut)
      plus_side_short / minus_side_short
                        a pair is united from the side of the LARGER voxel index b, which finds a among its candidates: the
                        candidate window one cell short on that side of the `axes` -- along y and z the rows
                        cy - reach .. cy + reach around the owner's cell, along x the run x0 - reach .. x1 + reach - 1
                        around the owner's GROUP (x_window)
    """
    r = link_regime(xyz, d, cp)
    fg, a, b = r["pairs"]
    off = r["offsets"]
    if fault == "two_cells":
        keep = (np.abs(off) <= 2).all(1)
    elif fault == "clamped_dropped":
        keep = ~(r["clamped"][fg[a]] | r["clamped"][fg[b]])
    elif fault == "first_tile":
        cc, dim = r["cells"], np.asarray(d.dim, np.int64)
        grp = ((cc[:, 2] * dim[1] + cc[:, 1]) * (-(-dim[0] // GROUP_X)) + cc[:, 0] // GROUP_X)
        order = np.lexsort((np.arange(len(cc)), cc[:, 0], grp))
        rank = np.empty(len(cc), np.int64)
        start = np.r_[0, np.flatnonzero(np.diff(grp[order])) + 1]
        rank[order] = np.arange(len(cc)) - np.repeat(start, np.diff(np.r_[start, len(cc)]))
        keep = rank[fg[b]] < TILE
    elif fault in ("plus_side_short", "minus_side_short"):
        ca, cb = r["cells"][fg[a]], r["cells"][fg[b]]
        lo, hi = cb - r["reach"], cb + r["reach"]
        lo[:, 0], hi[:, 0] = x_window(cb[:, 0], r["reach"])
        ax = list(axes)
        keep = ((ca <= hi - 1) if fault == "plus_side_short" else (ca >= lo + 1))[:, ax].all(1)
    else:
        raise KeyError(fault)
    return CC.cluster_model(xyz, cp, pairs=(fg, a[keep], b[keep]))


# ---- building cases -------------------------------------------------------------------------------------------------------
def _case(ijk0, ijk1=None, cell=M.CELL, origin=ORIGIN, **cp):
    """voxels ijk0 of camera 0 and ijk1 of camera 1 on the lattice of `cell` at `origin`, both cameras pinned there"""
    blocks = []
    for ijk in (ijk0, ijk1):
        ijk = np.zeros((0, 3), np.int64) if ijk is None else np.asarray(ijk, np.int64).reshape(-1, 3)
        assert (ijk >= 0).all()
        blocks.append(np.concatenate([M.corner(origin), M.lattice(ijk, cell, origin)]))
    plane = (0.0, 0.0, 1.0, -float(F32(origin[2])))
    return dict(points=np.ascontiguousarray(np.concatenate(blocks), F32), size_left=len(blocks[0]), dense=True,
                workspace=M.WIDE.copy(), cell=cell, cp=dict(CC.DEFAULTS, plane=plane, **cp))


def _box(i, j, k):
    return np.stack(np.meshgrid(np.arange(*i), np.arange(*j), np.arange(*k), indexing="ij"), -1).reshape(-1, 3)


# The bridge cases: voxels of 0.25 mm, a bridge per 0.12 m slot along x.  A grid cell is 80 voxels; an end at 79 (mod 80) lies a
# voxel below a cell face, one at 1 (mod 80) a voxel above it, so 79 -> 241 is 40.5 mm and three cells apart.  The corner bridge,
# (79, 79, 79) -> (241, 161, 161), is 49.8 mm long and (3, 2, 2) cells: no lattice coarser than 0.25 mm has such a pair.
# k_cluster_link takes its x range per GROUP of two cells, x0 - reach .. x1 + reach - 1 (x0 even, x1 = x0 + 2), so along x a
# partner is at the window's edge only if the owner -- the end with the larger voxel index -- is in the right cell of its group:
# the first cell for a partner on the - side, the second for one on the + side.  The slots are shifted by a cell where that needs it.
FINE = 0.00025
SLOT = 480  # voxels from slot to slot
BRIDGES = ("x", "y", "z", "corner")
# per span in cells (= the reach): the tolerance, and how far outwards along the bridge the second voxel of an end's part lies
# (within the tolerance of its end, beyond it from the other end; 0: the ends are single voxels)
BRIDGE_SETS = {1: dict(tolerance=0.011, buddy=0), 2: dict(tolerance=0.03, buddy=100), 3: dict(tolerance=0.05, buddy=48)}
BRIDGE_CASES = {1: "reach_one_edges", 2: "reach_two_edges", 3: "reach_three"}


def bridges(span: int):
    """per bridge of `span` cells (axis or, for span 3, corner; larger index on the + or the - side): its low end (a) and high
    end (b), in voxels"""
    out = []
    kinds = BRIDGES if span == 3 else BRIDGES[:3]
    for s, (kind, plus) in enumerate((k, p) for k in kinds for p in (True, False)):
        # the low end's cell along x: odd, so that the - side owner is a group's second cell -- but of the parity of the span
        # where the + side owns, so that the high end's cell is even, a group's first
        shift = 0 if plus and span % 2 == 0 else 1
        base = np.array([SLOT * s + 80 * shift, 0, 0]) + 160
        a = np.array([79, 79, 79]) if kind == "corner" else np.array([100, 100, 100])
        b = a.copy()
        if kind == "corner":
            b = np.array([241, 161, 161])
        else:
            ax = "xyz".index(kind)
            a[ax], b[ax] = 79, 80 * span + 1
        out.append((kind, plus, base + a, base + b))
    return out


def reach_three_bridges():
    return bridges(3)


def _bridge_case(span):
    cams = ([], [])
    buddy = BRIDGE_SETS[span]["buddy"]
    for kind, plus, a, b in bridges(span):
        # the + end in camera 1 (the larger indices) or in camera 0
        lo, hi = (0, 1) if plus else (1, 0)
        step = np.eye(3, dtype=np.int64)[0 if kind == "corner" else "xyz".index(kind)] * buddy
        cams[lo].extend([a, a - step] if buddy else [a])
        cams[hi].extend([b, b + step] if buddy else [b])
    return _case(cams[0], cams[1], cell=FINE, tolerance=BRIDGE_SETS[span]["tolerance"], max_objects=16)


def _reach_two_exact():
    """voxels of 4 mm: three lines along the axes, ten voxels (0.04 m, the tolerance itself) from one voxel to the next, and a
    line nine voxels apart that is adjacent beyond doubt"""
    ten = [(10 * q + 3, 3, 3) for q in range(8)] + [(3, 10 * q + 23, 3) for q in range(8)] + [(3, 3, 10 * q + 23) for q in range(8)]
    nine = [(9 * q + 3, 120, 12) for q in range(9)]
    return _case(ten, nine, cell=0.004, tolerance=0.04, max_objects=32)


OWNER_MIN_HEIGHT = 0.0125  # layers k <= 4 of the 3 mm lattice lie below it


def _owner_tiles():
    """3 mm voxels, seven per grid cell and axis (voxels 0 .. 6, 7 .. 13, 14 .. 19), both cameras seeing every voxel.  Block 1
    fills cells x = 0 and 1 of row (y, z) = (0, 0): 14 x 7 x 7 voxels.  Block 2, in row (2, 0): layers 0 .. 4 only -- background --
    in cell x = 0, all seven layers in cell x = 1."""
    b1 = _box((0, 14), (0, 7), (0, 7))
    b2 = np.concatenate([_box((0, 7), (14, 20), (0, 5)), _box((7, 14), (14, 20), (0, 7))])
    ijk = np.concatenate([b1, b2])
    return _case(ijk, ijk, tolerance=0.0031, min_height=OWNER_MIN_HEIGHT, max_objects=4)


def big_snake_path(rows=52, length=100):
    path = []
    for r in range(rows):
        ys = range(length) if r % 2 == 0 else range(length - 1, -1, -1)
        path += [(2 * r, y, 6) for y in ys]
        if r < rows - 1:
            path.append((2 * r + 1, length - 1 if r % 2 == 0 else 0, 6))
    return path


def _big_component():
    """a 150 x 150 sheet in layer 2, a snake of 52 rows of 100 in layer 6, and 20 x 20 components of one and two voxels in
    layers 10 and 11, two voxels apart -- x-major voxel order interleaves the three along every column"""
    sheet = _box((0, 150), (0, 150), (2, 3))
    small = []
    for q, (i, j) in enumerate((i, j) for i in range(20) for j in range(20)):
        small += [(2 * i, 2 * j, 10)] + ([(2 * i, 2 * j, 11)] if q % 3 == 0 else [])
    return _case(np.concatenate([sheet, np.array(big_snake_path()), np.array(small)]), tolerance=0.0031, max_objects=8)


def _many_roots(min_voxels, max_objects):
    """45 x 45 columns of 1, 2 or 3 voxels, three voxels apart"""
    ijk = [(3 * i, 3 * j, 2 + k) for i in range(45) for j in range(45) for k in range(1 + ((45 * i + j) * 7) % 3)]
    return _case(ijk, tolerance=0.0031, min_voxels=min_voxels, max_objects=max_objects)


ROOM_CELL = 0.01
ROOM_ORIGIN = {0.04: (-1.85, -1.85, -1.0), 0.08: (-3.5, -3.5, -2.0)}
ROOM_FAR = {0.04: (419, 419, 301), 0.08: (839, 839, 603)}


def _room(grid_cell, tolerance):
    """1 cm voxels.  Two far corners (camera 0) stretch the box; inside stand a 14 x 14 x 10 block seen by both cameras, a
    10 x 10 x 10 block 4 cm from it (camera 1), a 20 x 20 plate (camera 0) and a row of single voxels."""
    a = _box((200, 214), (200, 214), (20, 30))
    b = _box((217, 227), (202, 212), (20, 30))
    plate = _box((240, 260), (200, 220), (25, 26))
    dots = np.array([(200 + 7 * q, 190, 20 + q % 3) for q in range(9)])
    far = np.array([ROOM_FAR[grid_cell]])
    return _case(np.concatenate([a, plate, far]), np.concatenate([a, b, dots]), cell=ROOM_CELL, origin=ROOM_ORIGIN[grid_cell],
                 tolerance=tolerance, min_voxels=1, max_objects=8)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {"reach_three": _bridge_case(3), "reach_two_edges": _bridge_case(2), "reach_one_edges": _bridge_case(1), "reach_two_exact": _reach_two_exact(), "owner_tiles": _owner_tiles(),
           "big_component": _big_component()}
    for mv in (1, 2):
        for K in (64, 1):
            out[f"many_roots_min{mv}_K{K}"] = _many_roots(mv, K)
    for gc in (0.04, 0.08):
        for tol in (0.05, 0.011):
            out[f"doubled_cells_{gc}_tol{tol}"] = _room(gc, tol)
    return out


# ---- the sequence of one context ------------------------------------------------------------------------------------------------
SMALL_CELL, OUT_CELL = 0.001, 0.002
OUT_ORIGIN = tuple(v - 0.061 for v in ORIGIN)  # the small cloud's kept box begins 0.04 m below ORIGIN: at voxel 10.5 of OUT_CELL


def _small():
    """1 mm voxels, the parts three voxels apart: a 10 x 10 x 4 block (camera 0), a line seen by both cameras, a few single
    voxels; both cameras see a far voxel at (319, 319, 319), so the call sizes the context's voxel bitmap for what follows"""
    block = 3 * _box((10, 20), (10, 20), (3, 7))
    line = np.array([(3 * q + 90, 150, 30) for q in range(30)])
    dots = np.array([(200 + 9 * q, 40, 12) for q in range(8)])
    far = np.array([(319, 319, 319)])
    return _case(np.concatenate([block, line, far]), np.concatenate([line, dots, far]), cell=SMALL_CELL, tolerance=0.0031,
                 max_objects=8)


def out_parts() -> dict:
    """The parts of the cloud that leaves the small cloud's kept box -- voxels 11 .. 210 of OUT_CELL from OUT_ORIGIN on every
    axis, voxel u in cell floor((u - 10.5) / 10) -- as name -> (camera, voxels).  The tolerance is 0.03 m = 15 voxels."""
    p = {}
    p["inside"] = (0, 10 * _box((6, 11), (6, 11), (4, 7)))
    p["beyond_high_x"] = (1, [(215, 100, 100), (229, 100, 100), (229, 100, 110)])
    p["beyond_low_y"] = (0, [(100, 2, 100), (100, 8, 100)])
    p["beyond_low_z"] = (1, [(150, 150, 4), (160, 150, 4), (160, 150, 8)])
    # chains that cross a face: the last voxel inside the box (in the last cell but one) is 12 or 13 voxels from the first beyond
    p["across_high_x"] = (0, [(180, 40, 40), (190, 40, 40), (200, 40, 40), (212, 40, 40), (222, 40, 40)])
    p["across_low_x"] = (1, [(8, 160, 60), (21, 160, 60), (31, 160, 60)])
    p["across_high_y"] = (1, [(40, 190, 40), (40, 200, 40), (40, 212, 40), (40, 222, 40)])
    p["across_high_z"] = (0, [(40, 40, 200), (40, 40, 212), (40, 40, 224)])
    # 21 voxels apart, both in the border cell (19, 4, 4)
    p["same_border_cell_1"] = (0, [(214, 55, 55), (214, 58, 55)])
    p["same_border_cell_2"] = (1, [(235, 55, 55), (235, 58, 58)])
    p["beyond_corner"] = (0, [(214, 216, 100), (226, 222, 100)])
    return p


def _out():
    cams = ([], [])
    for cam, ijk in out_parts().values():
        cams[cam].extend(np.asarray(ijk).tolist())
    return _case(cams[0], cams[1], cell=OUT_CELL, origin=OUT_ORIGIN, tolerance=0.03, max_objects=16)


ROOM_STEP = "doubled_cells_0.04_tol0.05"


@functools.lru_cache(maxsize=None)
def sequence():
    """[(name, case, regime the grid model must give)] for the calls of one context, in order"""
    small, out, room = _small(), _out(), cases()[ROOM_STEP]
    return [("small_cold", small, "cold"), ("out_miss", out, "miss"), ("out_kept", out, "kept"), ("room_miss", room, "miss"),
            ("room_kept", room, "kept"), ("small_refit", small, "refit"), ("small_kept", small, "kept")]


def lattice_words(c=None, points=None, cams=None, cell=None) -> int:
    """n_words of the voxeliser's descriptor, of a case or of points with camera ids in the wide workspace: per camera the
    lattice's bits in 32-bit words, rounded up to blocks of 4096"""
    if c is not None:
        points, cams, cell = c["points"], M.camera_ids(c["points"], c["size_left"], c["dense"]), c["cell"]
    words = 0
    for sel, ijk in M._voxels(points, cams, M.WIDE, cell):
        bits = int(np.prod(ijk.max(0) + 1)) if len(sel) else 0
        words += -(-(-(-bits // 32)) // 4096) * 4096
    return words


def bitmap_chain_runs(words) -> list:
    """How often each call of a context runs its chain, from the calls' lattice sizes: a context without a bitmap sizes one from
    the call's lattice plus a quarter; a bitmap more than 8 times the LAST lattice plus 2^20 words is dropped first; a lattice
    that outgrows the bitmap runs the chain a second time (agh_preprocess and the end of a chain)."""
    cap, last, runs = 0, 0, []
    for w in words:
        if cap and last > 0 and cap > 8 * last + (1 << 20):
            cap = 0
        if cap and w > cap:
            cap, n = 0, 2
        else:
            n = 1
        if not cap:
            cap = ((w + w // 4) // 4096 + 1) * 4096
        last = w
        runs.append(n)
    return runs


# ---- models, computed once ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(name: str) -> dict:
    """of a case of cases() or a step of sequence(): the voxelised cloud (`xyz`, `cams`) and cluster_model of it (`m`), read-only"""
    if name not in cases():
        same = {"small_refit": "small_cold", "small_kept": "small_cold", "out_kept": "out_miss", "room_miss": ROOM_STEP,
                "room_kept": ROOM_STEP}
        if name in same:
            return model(same[name])
    c = cases()[name] if name in cases() else {n: s for n, s, _ in sequence()}[name]
    xyz, cams = CC.voxel_cloud(c)
    xyz.setflags(write=False)
    cams.setflags(write=False)
    return dict(case=c, xyz=xyz, cams=cams, m=CC.cluster_model(xyz, c["cp"]))


@functools.lru_cache(maxsize=None)
def sequence_descs():
    """per step of sequence(): (the descriptor its build uses, its regime, the model's counters after it)"""
    g, out = gs.GridModel(), []
    for name, _c, _want in sequence():
        (d, regime), = g.build([model(name)["xyz"]])
        out.append((d, regime, dict(g.stats)))
    return out


# ---- depth captures ---------------------------------------------------------------------------------------------------------------
DEPTH_W, DEPTH_H, DEPTH_F = 320, 240, 260.0


def _camera_points(cam_xyz):
    """points given in camera 0's optical frame, in the cloud's frame"""
    pose = D.scene_pose(0)
    return (np.asarray(cam_xyz, np.float64) @ pose[:, :3].T + pose[:, 3]).astype(F32)


def _patch(cx, cy, z, n=24, step=0.01):
    g = (np.arange(n) - (n - 1) / 2) * step
    u, v = np.meshgrid(g, g, indexing="ij")
    return np.stack([cx + u.ravel(), cy + v.ravel(), np.full(u.size, z)], 1)


def depth_plane():
    """the support plane of the depth cases: height = depth along camera 0's axis"""
    pose = D.scene_pose(0)
    n = pose[:, 2] / np.linalg.norm(pose[:, 2])
    return (float(n[0]), float(n[1]), float(n[2]), float(-n @ pose[:, 3]))


DEPTH_CP = dict(min_height=0.3, max_height=1.2, tolerance=0.03, min_voxels=5, max_objects=6)


@functools.lru_cache(maxsize=None)
def depth_steps() -> dict:
    """name -> (images, cp, voxel size): `small`, three patches 0.7 m in front of camera 0; `out`, the same with patches further
    out on every side, nearer and further away (beyond all six faces of `small`'s kept box); `doubled`, the small scene with single far points that stretch the box past the cell cap.
    `small` is voxelised at 4 mm, so that its call sizes a voxel bitmap that holds `out` at 1 cm."""
    near = np.concatenate([_patch(-0.20, 0.0, 0.70), _patch(0.10, 0.0, 0.70), _patch(0.10, 0.22, 0.72, n=12)])
    wider = np.concatenate([near, _patch(-0.5, -0.33, 1.0, n=10), _patch(0.5, 0.33, 1.0, n=10), _patch(0.5, -0.33, 1.0, n=10),
                            _patch(-0.5, 0.33, 1.0, n=10), _patch(-0.05, -0.15, 0.5, n=8)])
    far = np.array([[sx * 2.0, sy * 1.5, 4.5] for sx in (-1, 1) for sy in (-1, 1)] + [[0.0, 0.0, 0.45]])
    cp = dict(DEPTH_CP, plane=depth_plane())
    out = {}
    for name, pts in (("small", near), ("out", wider), ("doubled", np.concatenate([near, far]))):
        world = _camera_points(pts)
        out[name] = ([D.render_depth(world, k, DEPTH_W, DEPTH_H, D.U16, DEPTH_F, pad=1 + 2 * k) for k in range(2)], cp,
                     0.004 if name == "small" else 0.01)
    return out


def depth_cloud(images, cell=0.01):
    """the voxelised cloud of a depth capture by the numpy models (deproject_ref, voxel_model)"""
    return D.voxel_model(D.deproject_ref(images), D.image_index(images), M.WIDE, cell)
