"""Captures for the agh_localize_clustered* tests, and a numpy model of the contract in include/agh.h (numpy only).

A case is a dict: `points` ((N, 3) float32), `size_left`, `dense`, `workspace`, `cell` -- what tests/mask_cases.py's cases hold
-- and `cp`, the fields of agh_cluster_params.  The contract is stated on the VOXELISED cloud (tests/depth_captures.py,
voxel_model: per camera the unique voxels in lexicographic order, each at ijk * cell + the camera's minimum), so a case places
voxels, on mask_cases.lattice, and pins each camera's minimum with a point at the lattice's origin.

  cluster_model    labels, counts, ids, sizes and the lists E_j of a voxelised cloud: brute force, pairwise float32 d2
                   (adjacent_pairs), then the components of that graph
  cases            the inputs the tests run, each named after the regime tests/test_cluster_cases.py proves it is in
  table_scene      a table with three boxes, both cameras: the chain-equality scene of the GPU tests
"""
import numpy as np

from tests import depth_captures as D
from tests import mask_cases as M

F32 = np.float32
CELL = 0.01
ORIGIN = (0.25, 0.25, 0.25)
PLANE = (0.0, 0.0, 1.0, -0.25)  # z = 0.25: the lattice's floor
DEFAULTS = dict(plane=PLANE, min_height=0.005, max_height=0.5, tolerance=0.011, min_voxels=1, max_objects=4)


def heights(xyz: np.ndarray, plane) -> np.ndarray:
    """h = ((a x + b y) + c z) + d in double on the float coordinates, left to right"""
    p = np.asarray(xyz, F32).astype(np.float64)
    a, b, c, d = (np.float64(v) for v in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + d


def foreground(xyz: np.ndarray, cp: dict) -> np.ndarray:
    h = heights(xyz, cp["plane"])
    with np.errstate(invalid="ignore"):
        return np.isfinite(h) & (h > cp["min_height"]) & (h < cp["max_height"])


def d2_f32(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(dx dx + dy dy) + dz dz in float32, rows of p against rows of q"""
    d = p[:, None, :] - q[None, :, :]
    assert d.dtype == F32
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def tol2(tolerance: float) -> np.float32:
    return F32(np.float64(tolerance) * np.float64(tolerance))


def adjacent_pairs(xyz: np.ndarray, cp: dict):
    """(fg, a, b): the foreground voxel indices (ascending) and every adjacent pair fg[a] < fg[b] of them, by brute force: the
    float32 rule on all pairs, 256 rows at a time -- against the voxels whose x lies within the tolerance of the rows' only (the
    voxels sorted by x: what is left out is further away along x alone than any adjacent pair can be).  No cell structure."""
    xyz = np.ascontiguousarray(xyz, F32)
    fg = np.flatnonzero(foreground(xyz, cp))
    p = xyz[fg]
    t2 = tol2(cp["tolerance"])
    order = np.argsort(p[:, 0], kind="stable")
    ps, xs = p[order], p[order, 0].astype(np.float64)
    margin = 1.001 * float(cp["tolerance"]) + 1e-6
    out_a, out_b = [], []
    for i0 in range(0, len(fg), 256):
        i1 = min(i0 + 256, len(fg))
        hi = int(np.searchsorted(xs, xs[i1 - 1] + margin, "right"))
        i, j = np.nonzero(d2_f32(ps[i0:i1], ps[i0:hi]) <= t2)
        keep = i < j
        a, b = order[i0 + i[keep]], order[i0 + j[keep]]
        out_a.append(np.minimum(a, b))
        out_b.append(np.maximum(a, b))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    return fg, cat(out_a), cat(out_b)


def component_roots(n: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """per node 0 .. n - 1 the smallest node of its component under the edges (a, b)"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        parent = np.arange(n)

        def find(q):
            while parent[q] != q:
                parent[q] = parent[parent[q]]
                q = parent[q]
            return q

        for i, j in zip(a, b):
            i, j = find(i), find(j)
            if i != j:
                parent[max(i, j)] = min(i, j)
        return np.array([find(q) for q in range(n)], np.int64)
    _, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
    first = np.full(int(comp.max()) + 1 if n else 0, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp]


def cluster_model(xyz: np.ndarray, cp: dict, pairs=None) -> dict:
    """The contract of agh_localize_clustered on the voxelised cloud `xyz`: `labels` (per voxel 0 or j + 1), n_foreground,
    n_components, n_objects, `sizes` and `ids` (K entries: M_j, and the smallest voxel index or -1) and `lists` (E_j).  `pairs`:
    (fg, a, b) in place of adjacent_pairs' -- what a stage that lost some pairs would compute."""
    xyz = np.ascontiguousarray(xyz, F32)
    K = int(cp["max_objects"])
    fg, a, b = adjacent_pairs(xyz, cp) if pairs is None else pairs
    roots = component_roots(len(fg), a, b)  # (fg ascends: the root is the component's smallest voxel index)
    comp_ids, inv, sizes = (np.unique(fg[roots], return_inverse=True, return_counts=True) if len(fg)
                            else (np.zeros(0, np.int64),) * 3)
    ok = sizes >= int(cp["min_voxels"])
    cand = np.flatnonzero(ok)
    order = cand[np.lexsort((comp_ids[cand], -sizes[cand]))][:K]
    labels = np.zeros(len(xyz), np.uint8)
    out_sizes, out_ids, lists = np.zeros(K, np.int64), np.full(K, -1, np.int32), []
    inv = np.asarray(inv).reshape(-1)
    for j, q in enumerate(order):
        members = fg[inv == q]
        labels[members] = j + 1
        out_sizes[j], out_ids[j] = len(members), comp_ids[q]
        lists.append(members.astype(np.int32))
    lists += [np.zeros(0, np.int32)] * (K - len(order))
    return dict(labels=labels, n_foreground=len(fg), n_components=len(comp_ids), n_objects=len(order), sizes=out_sizes, ids=out_ids,
                lists=lists, n_qualifying=int(ok.sum()))


def voxel_cloud(c: dict):
    """the voxelised cloud of a case (xyz, camera ids), by the numpy model of the preprocessing"""
    cams = M.camera_ids(c["points"], c["size_left"], c["dense"])
    keep = cams >= 0
    return D.voxel_model(c["points"][keep, :3], cams[keep], c["workspace"], c["cell"])


def _case(ijk, ijk1=None, points=None, dense=True, size_left=None, **cp):
    """voxels `ijk` seen by camera 0 (and `ijk1` by camera 1), each camera's lattice pinned by a point at the origin"""
    if points is None:
        blocks = [np.concatenate([M.corner(ORIGIN), M.lattice(np.asarray(ijk).reshape(-1, 3), CELL, ORIGIN)])]
        if ijk1 is not None:
            blocks.append(np.concatenate([M.corner(ORIGIN), M.lattice(np.asarray(ijk1).reshape(-1, 3), CELL, ORIGIN)]))
        points, size_left = np.concatenate(blocks), len(blocks[0])
    return dict(points=np.ascontiguousarray(points, F32), size_left=size_left, dense=dense, workspace=M.WIDE.copy(), cell=CELL,
                cp=dict(DEFAULTS, **cp))


def _line(i0, i1, j, k):
    return [(i, j, k) for i in range(i0, i1)]


def _bridge_tolerance(c, want_above: bool) -> float:
    """A tolerance whose float32 bound (float) (tol * tol) is the bridging pair's float32 d2 exactly -- or, want_above, the
    float below it, so that the pair sits one float above the bound.  The pair: voxels (3, 0, 2) and (6, 1, 2)."""
    xyz, _ = voxel_cloud(c)
    a, b = bridge_pair(xyz)
    d2 = d2_f32(xyz[a:a + 1], xyz[b:b + 1])[0, 0]
    bound = np.nextafter(d2, F32(0)) if want_above else d2
    tol = float(np.sqrt(np.float64(bound)))
    for _ in range(64):  # (sqrt then square in double, rounded to float: a few steps at the most)
        got = tol2(tol)
        if got == bound:
            return tol
        tol = float(np.nextafter(tol, np.inf if got < bound else -np.inf))
    raise AssertionError("no double squares to that float")


def bridge_pair(xyz: np.ndarray):
    """the voxel indices of (3, 0, 2) and (6, 1, 2) in a threshold_neighbours cloud"""
    want = M.lattice([[3, 0, 2], [6, 1, 2]], CELL, ORIGIN) - F32(0.5 * CELL)
    return [int(np.argmin(np.abs(xyz - w).sum(1))) for w in want]


def snake_path():
    """the voxels of the snake in walking order: 20 rows of 30 along y at x = 0, 2, 4, ..., joined by one voxel at alternating ends"""
    path = []
    for r in range(20):
        ys = range(30) if r % 2 == 0 else range(29, -1, -1)
        path += [(2 * r, y, 2) for y in ys]
        if r < 19:
            path.append((2 * r + 1, 29 if r % 2 == 0 else 0, 2))
    return path


def cases() -> dict:
    out = {}
    # two lines along x whose closest voxels, (3, 0, 2) and (6, 1, 2), are sqrt(10) cells apart; every other pair across is further
    two_lines = _line(0, 4, 0, 2) + _line(6, 10, 1, 2)
    c = _case(two_lines)
    out["threshold_neighbours"] = _case(two_lines, tolerance=_bridge_tolerance(c, False))
    out["threshold_neighbours_above"] = _case(two_lines, tolerance=_bridge_tolerance(c, True))
    # layers k = 1 .. 5 of a 3 x 3 column; the bounds ARE the heights of layers 1 and 5 (background), 2 .. 4 lie inside -- and in
    # the twin the bounds are the doubles just outside, so that layers 1 and 5 are inside too
    col = [(i, j, k) for i in range(3) for j in range(3) for k in range(1, 6)]
    xyz, _ = voxel_cloud(_case(col))
    hs = np.unique(heights(xyz, PLANE))
    assert len(hs) == 6  # (the corner's layer and the five)
    out["strict_heights"] = _case(col, min_height=float(hs[1]), max_height=float(hs[5]))
    out["strict_heights_inside"] = _case(col, min_height=float(np.nextafter(hs[1], -np.inf)), max_height=float(np.nextafter(hs[5], np.inf)))
    out["snake"] = _case(snake_path())
    # one line along x, its even voxels seen by camera 0 and its odd ones by camera 1
    out["both_cameras"] = _case([(i, 1, 2) for i in range(0, 12, 2)], [(i, 1, 2) for i in range(1, 12, 2)])
    out["size_ties"] = _case(_line(0, 5, 0, 2) + _line(0, 5, 4, 3) + _line(0, 5, 8, 2), max_objects=3)
    # 75 columns along z on a 9 x 9 board, three cells apart: 70 of 3 .. 6 voxels, 5 of 2
    cols = []
    for q in range(75):
        size = 2 if q % 15 == 7 else 3 + (q * 7) % 4
        cols += [(3 * (q // 9), 3 * (q % 9), 2 + k) for k in range(size)]
    out["seventy_components"] = _case(cols, min_voxels=3, max_objects=64)
    out["no_foreground"] = _case([(i, j, 0) for i in range(4) for j in range(4)])
    out["all_one_component"] = _case([(i, j, k) for i in range(6) for j in range(6) for k in range(2, 5)], max_objects=2)
    out["fewer_objects_than_K"] = _case(_line(0, 6, 0, 2) + _line(0, 3, 5, 2), max_objects=5)
    # dense = 0 with drop-outs ahead of size_left: the ranks decide the cameras (mask_cases, rank_cameras)
    nan = np.full((3, 3), np.nan, F32)
    pts = np.concatenate([nan[:2], M.corner(ORIGIN), M.lattice(_line(0, 4, 0, 2), CELL, ORIGIN), nan[2:],
                          M.corner(ORIGIN), M.lattice(_line(4, 8, 0, 2) + _line(0, 3, 6, 3), CELL, ORIGIN),
                          np.array([[np.inf, 0.3, 0.3]], F32)])
    out["non_finite"] = _case(None, points=pts, dense=False, size_left=5)
    return out


def table_scene(seed: int = 5):
    """An axis-aligned 36 x 36 cm table at z = -0.099 with three axis-aligned cubes of 6, 4.5 and 3 cm on it, on the 3 mm lattice,
    each camera keeping 0.8 of the points: (points, size_left, workspace, camera origins, cp fields)."""
    from agile_grasp_amd import synthetic

    rng = np.random.default_rng(seed)
    zt = -0.099
    g = np.arange(-60, 61)
    u, v = np.meshgrid(g, g, indexing="ij")
    parts = [np.stack([u.ravel(), v.ravel(), np.zeros(u.size, np.int64)], 1)]
    for cx, cy, half in ((-30, -25, 10), (25, -20, 7), (0, 30, 5)):
        b = np.arange(-half, half + 1)
        h = np.arange(1, 2 * half + 1)
        bu, bv = np.meshgrid(b, b, indexing="ij")
        parts.append(np.stack([cx + bu.ravel(), cy + bv.ravel(), np.full(bu.size, 2 * half)], 1))
        su, sh = np.meshgrid(b, h[:-1], indexing="ij")
        for sgn in (-1, 1):
            parts.append(np.stack([cx + su.ravel(), np.full(su.size, cy + sgn * half), sh.ravel()], 1))
            parts.append(np.stack([np.full(su.size, cx + sgn * half), cy + su.ravel(), sh.ravel()], 1))
    ijk = np.unique(np.concatenate(parts), axis=0)
    pts = ijk * 0.003 + np.array([0.75, 0.0, zt])
    clouds = [pts[rng.random(len(pts)) < 0.8] for _cam in range(2)]
    xyz = np.ascontiguousarray(np.concatenate(clouds), F32)
    ws = np.array([0.5, 1.0, -0.25, 0.25, -0.2, 0.2])
    cp = dict(plane=(0.0, 0.0, 1.0, -zt), min_height=0.004, max_height=0.5, tolerance=0.007, min_voxels=50, max_objects=4)
    return xyz, len(clouds[0]), ws, synthetic.camera_origins(), cp
