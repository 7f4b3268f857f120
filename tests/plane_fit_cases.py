"""Captures for the agh_localize_clustered_fit* tests, and a numpy model of rules 1 to 6 of the contract in include/agh.h (numpy
and the oracle's smallest_eigvec3 only).

A case is what tests/cluster_cases.py's cases hold -- `points`, `size_left`, `dense`, `workspace`, `cell`, `cp` (whose plane the
fitted call does not read) -- and `fp`, the fields of agh_plane_fit_params, `origins` (the context's two camera origins) and
`table` (None, or the one row of an agh_set_cloud_cam_origins table).  Everything is stated on the VOXELISED cloud
(cluster_cases.voxel_cloud).

  draw, candidates, counts     rules 1 to 3: all arithmetic in double, products and sums in the order the header writes them
  refit_sums                   rule 5's contributors and ten sums as exact Python integers
  fit_model                    rules 1 to 6: what agh_get_plane_fit and agh_get_plane_fit_candidates report
  cases                        the inputs the tests run, each named after the regime tests/test_plane_fit_cases.py proves it is in
  rotated_scene                cluster_cases.table_scene() turned 33 degrees about x and -19 about y, origins and plane with it
"""
import numpy as np

from tests import cluster_cases as CC
from tests import mask_cases as M

F32 = np.float32
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ABOVE = np.array([[0.3, 0.3, 2.0], [0.3, 0.3, 2.0]])  # the lattice cases' cameras: over the floor
FP_DEFAULTS = dict(n_candidates=128, refine=1, min_inliers=3, distance_threshold=0.01, seed=1)
LATTICE_THRESHOLD = 0.004  # the lattice cases': below the 1 cm between two levels


def splitmix64(x: int) -> int:
    x = (x + GOLDEN) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def draw(N: int, C: int, seed: int) -> np.ndarray:
    """rule 1: (C, 3) voxel indices; -1 everywhere with N < 3"""
    out = np.full((C, 3), -1, np.int32)
    if N >= 3:
        for c in range(C):
            for s in range(3):
                out[c, s] = splitmix64((seed ^ (((3 * c + s) * GOLDEN) & MASK64)) & MASK64) % N
    return out


def candidates(xyz: np.ndarray, C: int, seed: int):
    """rules 1 and 2: (idx (C, 3), planes (C, 4), valid (C,)); an invalid candidate's plane is zeros"""
    xyz = np.ascontiguousarray(xyz, F32)
    idx = draw(len(xyz), C, seed)
    planes, valid = np.zeros((C, 4), np.float64), np.zeros(C, bool)
    if len(xyz) < 3:
        return idx, planes, valid
    p = xyz.astype(np.float64)[idx]  # (C, 3, 3)
    with np.errstate(all="ignore"):
        u, v = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                      u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        valid = np.isfinite(l2) & (l2 > 0.0)
        n = n / np.sqrt(l2)[:, None]
        d = -((n[:, 0] * p[:, 0, 0] + n[:, 1] * p[:, 0, 1]) + n[:, 2] * p[:, 0, 2])
    planes[valid, :3] = n[valid]
    planes[valid, 3] = d[valid]
    return idx, planes, valid


def inliers(xyz: np.ndarray, plane, threshold: float) -> np.ndarray:
    """rule 3, one plane: cluster_cases.heights is the evaluation order"""
    with np.errstate(invalid="ignore"):
        return np.abs(CC.heights(xyz, plane)) <= np.float64(threshold)


def counts(xyz: np.ndarray, planes: np.ndarray, valid: np.ndarray, threshold: float) -> np.ndarray:
    return np.array([int(inliers(xyz, planes[c], threshold).sum()) if valid[c] else 0 for c in range(len(planes))], np.int64)


def refit_sums(xyz: np.ndarray, members: np.ndarray, p0: np.ndarray):
    """rule 5: (n_refit, [Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz]) over the voxels `members`, as Python integers, and the
    largest |q| met"""
    xyz = np.ascontiguousarray(xyz, F32)
    d = xyz[members] - np.asarray(p0, F32)[None, :]
    assert d.dtype == F32
    d = d[(np.abs(d) < F32(8.0)).all(1)]
    q = [[int(t) for t in np.rint(d[:, a].astype(np.float64) * 65536.0)] for a in range(3)]
    S = [sum(q[a]) for a in range(3)]
    S += [sum(x * y for x, y in zip(q[a], q[b])) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return len(d), S, max([abs(t) for a in range(3) for t in q[a]], default=0)


def fit_model(xyz: np.ndarray, fp: dict, origin) -> dict:
    """rules 1 to 6 on the voxelised cloud `xyz` with camera 0's origin `origin`: the fields of agh_plane_fit_result, and `idx`,
    `planes`, `counts` per candidate (planes before refit and orientation)"""
    from oracle import oracle_py

    xyz = np.ascontiguousarray(xyz, F32)
    f = dict(FP_DEFAULTS, **fp)
    idx, planes, valid = candidates(xyz, f["n_candidates"], f["seed"])
    cnt = counts(xyz, planes, valid, f["distance_threshold"])
    best = int(np.argmax(cnt))  # (the first of the largest: ties to the smaller c)
    n_inl = int(cnt[best])
    found = n_inl >= max(f["min_inliers"], 3)
    out = dict(idx=idx, planes=planes, counts=cnt, n_voxels=len(xyz), n_inliers=n_inl, n_refit=0, best_candidate=best if n_inl > 0 else -1,
               found=int(found), refined=0, plane=np.zeros(4))
    if not found:
        return out
    plane = planes[best].copy()
    if f["refine"]:
        p0 = xyz[idx[best, 0]]
        members = np.flatnonzero(inliers(xyz, planes[best], f["distance_threshold"]))
        n_refit, S, _ = refit_sums(xyz, members, p0)
        out["n_refit"] = n_refit
        if 3 <= n_refit <= (1 << 24):
            Nn = np.float64(n_refit)
            S = [np.float64(float(s)) for s in S]  # (int -> double: round to nearest, as the conversion of an int64)
            m = [(S[a] / Nn) * np.float64(2.0 ** -16) for a in range(3)]
            pair = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
            Mv = [(S[3 + k] / Nn) * np.float64(2.0 ** -32) - m[a] * m[b] for k, (a, b) in enumerate(pair)]
            M3 = np.array([[Mv[0], Mv[1], Mv[2]], [Mv[1], Mv[3], Mv[4]], [Mv[2], Mv[4], Mv[5]]])
            axis = oracle_py.smallest_eigvec3(M3)
            if np.isfinite(axis).all():
                c = [np.float64(p0[a]) + m[a] for a in range(3)]
                plane = np.array([axis[0], axis[1], axis[2], -((axis[0] * c[0] + axis[1] * c[1]) + axis[2] * c[2])])
                out["refined"] = 1
    o = np.asarray(origin, np.float64)
    s = ((plane[0] * o[0] + plane[1] * o[1]) + plane[2] * o[2]) + plane[3]
    out["s"] = float(s)
    if s < 0.0:
        plane = -plane
    out["plane"] = plane
    return out


def origin_of(c: dict) -> np.ndarray:
    """camera 0's origin in force for the case"""
    return np.asarray(c["table"][0] if c["table"] is not None else c["origins"][0], np.float64)


def voxel_cloud(c: dict):
    """cluster_cases.voxel_cloud, and the empty cloud of a capture without a kept point"""
    ws = c["workspace"]
    p = c["points"][:, :3]
    with np.errstate(invalid="ignore"):
        if not ((p >= ws[0::2]) & (p <= ws[1::2])).all(1).any():
            return np.zeros((0, 3), F32), np.zeros(0, np.int32)
    return CC.voxel_cloud(c)


def case_model(c: dict) -> dict:
    xyz, _ = voxel_cloud(c)
    return fit_model(xyz, c["fp"], origin_of(c))


# ---- the cases ----

def _floor(nx, ny, k=0):
    return [(i, j, k) for i in range(nx) for j in range(ny)]


def _block(i0, j0, side, height, k0=1):
    return [(i0 + i, j0 + j, k0 + k) for i in range(side) for j in range(side) for k in range(height)]


SMALL = _floor(12, 12) + _block(2, 2, 3, 3) + _block(8, 7, 2, 4)


def _case(ijk, ijk1=None, fp=None, table=None, points=None, size_left=None, **cp):
    c = CC._case(ijk, ijk1, points=points, size_left=size_left, **dict(dict(min_height=0.005, tolerance=0.011, min_voxels=4), **cp))
    c.update(fp=dict(FP_DEFAULTS, **dict(dict(distance_threshold=LATTICE_THRESHOLD), **(fp or {}))), origins=ABOVE.copy(), table=None if table is None else np.asarray(table, np.float64))
    return c


def is_level(plane) -> bool:
    """a candidate through three voxels of one lattice level: n = (0, 0, +-1) exactly"""
    return plane[0] == 0.0 and plane[1] == 0.0 and abs(plane[2]) == 1.0


def _first_seed(ok, limit=400) -> int:
    for seed in range(1, limit):
        if ok(seed):
            return seed
    raise AssertionError("no seed below %d puts the case in its regime" % limit)


def layer_threshold(ijk, level: int) -> float:
    """the height of lattice level `level` over level 0 as the double difference of the two float32 coordinates"""
    xyz, _ = CC.voxel_cloud(_case(ijk))
    z = np.unique(xyz[:, 2])
    return float(np.float64(z[level]) - np.float64(z[0]))


def cases() -> dict:
    out = {}
    out["floor_blocks_small"] = _case(SMALL)
    # 40 x 41 and two blocks: several work-groups, N no multiple of 64
    large = _floor(40, 41) + _block(5, 5, 6, 5) + _block(25, 30, 4, 7)
    out["floor_blocks_large"] = _case(large)
    # an exactly planar floor under one cube: every candidate inside the floor counts the whole floor
    tied = _floor(12, 12) + _block(3, 3, 5, 5)
    xyz, _ = CC.voxel_cloud(_case(tied))

    def tie_not_first(seed):
        _i, pl, va = candidates(xyz, 128, seed)
        cn = counts(xyz, pl, va, LATTICE_THRESHOLD)
        return int(np.argmax(cn)) != 0 and is_level(pl[int(np.argmax(cn))]) and int((cn == cn.max()).sum()) >= 2

    out["ties"] = _case(tied, fp=dict(seed=_first_seed(tie_not_first)))
    # a layer of eight voxels whose height IS the threshold; the twin's threshold is the double below
    layered = _floor(12, 12) + [(i, j, 1) for i in range(4, 8) for j in range(5, 7)]
    thr = layer_threshold(layered, 1)
    xyz, _ = CC.voxel_cloud(_case(layered))

    def level_wins_both(seed):
        _i, pl, va = candidates(xyz, 16, seed)
        for t in (thr, float(np.nextafter(thr, 0.0))):
            cn = counts(xyz, pl, va, t)
            if not is_level(pl[int(np.argmax(cn))]) or pl[int(np.argmax(cn)), 3] != -pl[int(np.argmax(cn)), 2] * np.float64(xyz[0, 2]):
                return False
        return True

    seed = _first_seed(level_wins_both)
    out["threshold_exact"] = _case(layered, fp=dict(n_candidates=16, seed=seed, distance_threshold=thr))
    out["threshold_below"] = _case(layered, fp=dict(n_candidates=16, seed=seed, distance_threshold=float(np.nextafter(thr, 0.0))))
    # N = 0 (the one point lies outside the workspace), 1, 2, 3 on a line -- and three voxels that do span a plane
    out["too_few_0"] = _case(None, points=np.array([[20.0, 0.0, 0.0]], F32), size_left=1)
    out["too_few_1"] = _case(np.zeros((0, 3), int))
    out["too_few_2"] = _case([(3, 0, 0)])
    out["too_few_3"] = _case([(3, 0, 0), (6, 0, 0)])
    out["three_voxels"] = _case([(3, 0, 0), (0, 4, 0)])
    out["collinear"] = _case([(i, 0, 0) for i in range(1, 30)])
    # a planar patch of 25 voxels: every valid candidate counts 25
    out["min_inliers_above"] = _case(_floor(5, 5), fp=dict(min_inliers=26))
    out["min_inliers_equal"] = _case(_floor(5, 5), fp=dict(min_inliers=25))
    out["camera_below"] = _case(SMALL, table=[[0.3, 0.3, 0.0], [0.3, 0.3, 0.0]])
    # the camera ON the chosen candidate's plane: s == 0 (no refit, so that the plane is the level's, exactly)
    z0 = float(np.float64(xyz[0, 2]))
    out["camera_on_plane"] = _case(tied, fp=dict(out["ties"]["fp"], refine=0), table=[[0.3, 0.3, z0], [0.3, 0.3, z0]])
    # two floor voxels 8.5 m along x: inliers, and no part of the refit
    far = tied + [(850, 3, 0), (851, 8, 0)]
    fxyz, _ = CC.voxel_cloud(_case(far))

    def near_p0(seed):
        i, pl, va = candidates(fxyz, 128, seed)
        b = int(np.argmax(counts(fxyz, pl, va, LATTICE_THRESHOLD)))
        return is_level(pl[b]) and fxyz[i[b, 0], 0] < 1.0

    out["far_inliers"] = _case(far, fp=dict(seed=_first_seed(near_p0)))
    out["refine_off"] = _case(SMALL, fp=dict(refine=0))
    out["one_candidate"] = _case(SMALL, fp=dict(n_candidates=1, seed=_first_seed(lambda s: candidates(CC.voxel_cloud(_case(SMALL))[0], 1, s)[2][0])))
    out["max_candidates"] = _case(SMALL, fp=dict(n_candidates=256))
    out["seed_zero"] = _case(SMALL, fp=dict(seed=0))
    out["seed_max"] = _case(SMALL, fp=dict(seed=MASK64))
    # the floor's even columns seen by camera 0, its odd ones by camera 1; a block each
    out["both_cameras"] = _case([v for v in _floor(12, 12) if v[0] % 2 == 0] + _block(2, 2, 3, 3),
                                [v for v in _floor(12, 12) if v[0] % 2 == 1] + _block(8, 7, 2, 4))
    return out


CHAIN_CASES = ("floor_blocks_small", "floor_blocks_large", "both_cameras")


def rotation() -> np.ndarray:
    ax, ay = np.deg2rad(33.0), np.deg2rad(-19.0)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    return Ry @ Rx


def rotated_scene():
    """table_scene() turned: (points, size_left, workspace, origins, cp fields with the TRUE plane, the table's centre)"""
    xyz, size_left, _ws, origins, cp = CC.table_scene()
    R = rotation()
    pts = np.ascontiguousarray((xyz.astype(np.float64) @ R.T), F32)
    a, b, c, d = cp["plane"]
    n = R @ np.array([a, b, c])
    centre = R @ np.array([0.75, 0.0, -0.099])
    cp = dict(cp, plane=(float(n[0]), float(n[1]), float(n[2]), float(d)))
    return pts, size_left, M.WIDE.copy(), np.asarray(origins, np.float64) @ R.T, cp, centre
