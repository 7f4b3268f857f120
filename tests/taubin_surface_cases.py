"""Inputs for the Taubin frame stage (k_taubin_moments -> k_taubin_eigen -> k_taubin_frame / k_taubin_frame_huge) on exact, tied
and singular surfaces: planes in every capacity class and lattice orientation, symmetric curved surfaces, more than 4096 samples
on a singular pencil, the all-points pass on planes, neighbourhoods of 3 .. 8 points, and coordinates far from the origin or in
other units (tests/test_taubin_surface_cases.py checks every case against the oracle and numpy on the CPU;
tests/test_gpu_taubin_surfaces.py runs them on the GPU).

Plain numpy and the oracle, no GPU.  Every coordinate is a multiple of 2^-20 m or coarser, at most 8 m from the origin, so it is
exact in float32 (`_exact` asserts it): a plane is a plane to the last bit and the mirror images of a symmetric surface are
mirror images to the last bit.  Camera ids follow a fixed pattern (index % 3 == 0 is camera 1).  Clouds and the oracle's answers
are built once per process and shared by the tests; nobody writes to them.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from tests import capacity_clouds as cc

H8 = 2.0 ** -8
C0 = np.array([180, 13, -12]) * H8  # the patch centre of tests/test_taubin_solver.py: (0.703, 0.051, -0.047), on every lattice here
FAR = np.array([1536, -768, 512]) * H8  # (6, -3, 2) m
FINE = 2.0 ** 20  # curved surfaces are rounded to the 2^-20 m lattice (1 um)
R_TAUBIN, R_NORMALS = 0.03, 0.01
DISC = 0.045  # patch radius: the balls of the samples at the centre are full

# neighbour counts a capacity class of the sample pass owns (taubin.hip: k_taubin_frame<1152 / 4096 / 6144>, k_taubin_frame_huge)
CLASS_RANGE = {"1152": (1, 1152), "4096": (1153, 4096), "6144": (4097, 6144), "huge": (6145, 1 << 30)}
# ... and of the all-points pass (k_taubin_frame<128, 64> with a column per lane up to 64 normals, <1152> beyond 128)
ALLPOINTS_RANGE = {"lane": (1, 64), "128": (65, 128), "1152": (129, 1152)}

# two lattice vectors that span the plane through the origin with the given normal
PLANE_BASIS = {
    "z": ((1, 0, 0), (0, 1, 0)),
    "x": ((0, 1, 0), (0, 0, 1)),
    "110": ((1, -1, 0), (0, 0, 1)),
    "10m1": ((1, 0, 1), (0, 1, 0)),
    "111": ((1, -1, 0), (0, 1, -1)),
}
PLANE_NORMAL = {"z": (0, 0, 1), "x": (1, 0, 0), "110": (1, 1, 0), "10m1": (1, 0, -1), "111": (1, 1, 1)}


class Case(NamedTuple):
    xyz: np.ndarray  # (N, 3) float32
    cam: np.ndarray  # (N,) int32
    samples: np.ndarray  # (S,) int32
    classes: tuple  # per sample: key of CLASS_RANGE
    normal: tuple | None = None  # plane cases: the lattice normal
    axis: tuple | None = None  # the cylinder's axis
    ties: tuple | None = None  # (least, most) columns within the filter's margin of the best column sum, or None: not stated


def _exact(p):
    """float32 rows of p, which must hold them exactly."""
    p = np.asarray(p, np.float64)
    q = p.astype(np.float32)
    assert np.array_equal(q.astype(np.float64), p)
    return np.ascontiguousarray(q)


def _cam(n):
    return (np.arange(n) % 3 == 0).astype(np.int32)


def _nearest(p, centre, k):
    d = ((np.asarray(p, np.float64) - centre) ** 2).sum(1)
    return np.argsort(d, kind="stable")[:k].astype(np.int32)


def _lattice_disc(normal, hu, hv, radius=DISC):
    """Local coordinates (float64, exact) of the lattice points i hu e1 + j hv e2 within `radius` of the origin."""
    e1, e2 = (np.asarray(e, np.float64) for e in PLANE_BASIS[normal])
    m = int(radius / min(hu, hv)) + 1
    i, j = np.meshgrid(np.arange(-m, m + 1), np.arange(-m, m + 1), indexing="ij")
    p = i.ravel()[:, None] * hu * e1 + j.ravel()[:, None] * hv * e2
    return p[(p * p).sum(1) <= radius * radius]


def _patch(local, centre, classes, extra_samples=(), **kw):
    xyz = _exact(local + centre)
    s = np.concatenate([_nearest(local, 0.0, 3), np.asarray(extra_samples, np.int32)]).astype(np.int32)
    return Case(xyz, _cam(len(xyz)), s, tuple(classes), **kw)


# ---- A: exactly planar discs, one per capacity class ------------------------------------------------------------------
DISC_STEPS = {"1152": (2.0 ** -9, 2.0 ** -9), "4096": (2.0 ** -10, 2.0 ** -10), "6144": (2.0 ** -10, 2.0 ** -11),
              "huge": (2.0 ** -11, 2.0 ** -11)}
PLANE_CASES = tuple(f"plane-{c}-{n}" for c in ("1152", "4096", "6144") for n in ("z", "x")) + tuple(
    f"plane-4096-{n}" for n in ("110", "10m1", "111"))
HUGE_CASES = ("plane-huge-z", "plane-huge-x")
RIM_CUT = 33 * 2.0 ** -10  # plane-4096-z ends in a straight edge at u = 32.2 mm (beyond the central samples' balls)


def _plane_case(cls, normal, centre=C0):
    hu, hv = DISC_STEPS[cls]
    local = _lattice_disc(normal, hu, hv)
    classes, extra = [cls] * 3, ()
    if (cls, normal) == ("4096", "z"):
        # a fourth sample whose neighbourhood stays in the 1152 class, in one launch with three the list walk takes.  The rim of
        # the full disc does not give one (a ball on the rim still holds 1270 of these points), so the disc is cut along a
        # chord and the sample sits in the corner between chord and rim.
        local = local[local[:, 0] <= RIM_CUT]
        corner = np.flatnonzero(local[:, 0] == RIM_CUT)
        extra = (corner[np.argmax(local[corner, 1])],)
        classes.append("1152")
    return _patch(local, centre, classes, extra, normal=PLANE_NORMAL[normal])


# ---- B: exact symmetric surfaces in the 4096 class ----------------------------------------------------------------------
SURFACE_CASES = ("cylinder", "ridge", "sphere", "saddle")
CYL_R, SPHERE_R = 0.04, 0.05


def _fine(v):
    return np.round(np.asarray(v, np.float64) * FINE) / FINE


def _surface_local(kind):
    """Local coordinates: the surface passes through the origin, convex towards -x (the cameras) where it is convex at all."""
    if kind == "cylinder":  # radius 0.04 about the z direction: 2 pi / 512 steps of angle (0.49 mm of arc) x 2^-9 m along the axis
        k, j = np.meshgrid(np.arange(-128, 129), np.arange(-24, 25), indexing="ij")
        th = k.ravel() * (2.0 * np.pi / 512)
        p = np.stack([_fine(CYL_R - CYL_R * np.cos(th)), _fine(CYL_R * np.sin(th)), j.ravel() * 2.0 ** -9], 1)
    else:
        g = np.arange(-47, 48) * 2.0 ** -10
        u, v = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
        keep = u * u + v * v <= DISC * DISC
        u, v = u[keep], v[keep]
        if kind == "ridge":  # x = |u|: two half planes that meet at a right angle
            w = np.abs(u)
        elif kind == "sphere":
            w = _fine(SPHERE_R - np.sqrt(SPHERE_R ** 2 - u * u - v * v))
        else:  # saddle: 6 u v is a multiple of 2^-20
            w = 6.0 * u * v
        p = np.stack([w, u, v], 1)
    return p[(p * p).sum(1) <= DISC * DISC]


SURFACE_TIES = {"cylinder": (8, None), "ridge": (16, None), "sphere": (1, 4), "saddle": (1, 4)}


def _surface_case(kind, centre=C0, ties=True):
    return _patch(_surface_local(kind), centre, ["4096"] * 3, axis=(0, 0, 1) if kind == "cylinder" else None,
                  ties=SURFACE_TIES[kind] if ties else None)


# ---- C: more than 4096 samples on a singular pencil ---------------------------------------------------------------------
MANY_CASES = ("many-z", "many-x")
MANY_SIDE = 72  # 72 x 72 = 5184 points on the 2^-8 m lattice, every one a sample
MANY_FIRST = 4096
# On the x plane the quadric of fifteen samples (all among the first 4096) has a gradient of exactly zero at one of their
# neighbours, a point on the zero line of the fit's second linear factor: that neighbour's normal is 0 / 0, M3 and every column
# sum are NaN, and the frame's normal, axis and binormal are NaN with valid = 1; max_index is 0, which the oracle's sequential
# `s > best` never leaves.  The case is kept for that: the kernels must give the same records, and no hypothesis, for those
# samples (k_taubin_frame kept whichever column a lane had summed first until this case showed it).
NONFINITE_CASES = ("many-x",)
FRAME_FLOATS = ("sample", "normal", "axis", "binormal", "params", "eigenvalue")


def finite_rows(frames):
    """Mask of the frames all of whose floating-point entries are finite."""
    return np.logical_and.reduce([np.isfinite(frames[f]).reshape(len(frames), -1).all(1) for f in FRAME_FLOATS])


def _many_case(normal):
    e1, e2 = (np.asarray(e, np.float64) for e in PLANE_BASIS[normal])
    i, j = np.meshgrid(np.arange(MANY_SIDE) - MANY_SIDE // 2, np.arange(MANY_SIDE) - MANY_SIDE // 2, indexing="ij")
    xyz = _exact(i.ravel()[:, None] * H8 * e1 + j.ravel()[:, None] * H8 * e2 + C0)
    n = len(xyz)
    return Case(xyz, _cam(n), np.arange(n, dtype=np.int32), ("1152",) * n, normal=PLANE_NORMAL[normal])


# Three collinear neighbours with a zero gradient at one of them: the (1,1,0) plane on the 2^-7 m lattice under a Taubin radius of
# 0.01 m (rows 7.8 mm apart, the next row 11 mm away).  A few dozen of its 2304 samples have a NaN frame.  With every point a
# sample and both radii 0.01 the sample pass takes them through the 1152 class's one-column-at-a-time sums and the all-points
# pass through the column-per-lane form of the 128 class.
SPARSE_CASE = "sparse-110"
SPARSE_RADIUS = 0.01
SPARSE_SIDE = 48


def _sparse_case():
    e1, e2 = (np.asarray(e, np.float64) for e in PLANE_BASIS["110"])
    i, j = np.meshgrid(np.arange(SPARSE_SIDE) - SPARSE_SIDE // 2, np.arange(SPARSE_SIDE) - SPARSE_SIDE // 2, indexing="ij")
    xyz = _exact(i.ravel()[:, None] * 2.0 ** -7 * e1 + j.ravel()[:, None] * 2.0 ** -7 * e2 + C0)
    n = len(xyz)
    return Case(xyz, _cam(n), np.arange(n, dtype=np.int32), ("1152",) * n, normal=PLANE_NORMAL["110"])


@functools.lru_cache(maxsize=None)
def sparse_reference():
    """The oracle's find_hands with the all-points pass for SPARSE_CASE under nn_radius_taubin = SPARSE_RADIUS (read only)."""
    from oracle import oracle_py as O

    c = case(SPARSE_CASE)
    return O.find_hands(params(nn_radius_taubin=SPARSE_RADIUS), c.xyz, c.cam, c.samples, calculates_antipodal=True)


# ---- D: the all-points pass (r = 0.01) on exact planes --------------------------------------------------------------------
ALLPOINTS_STEPS = {"lane": (2.0 ** -8, 64), "128": (2.0 ** -9, 64), "1152": (2.0 ** -10, 96)}  # step, points per side
ALLPOINTS_CASES = tuple(f"allpoints-{c}-{n}" for c in ALLPOINTS_STEPS for n in ("z", "x"))


def _allpoints_case(cls, normal):
    h, side = ALLPOINTS_STEPS[cls]
    e1, e2 = (np.asarray(e, np.float64) for e in PLANE_BASIS[normal])
    i, j = np.meshgrid(np.arange(side) - side // 2, np.arange(side) - side // 2, indexing="ij")
    local = i.ravel()[:, None] * h * e1 + j.ravel()[:, None] * h * e2
    xyz = _exact(local + C0)
    s = _nearest(local, 0.0, 3)
    sample_cls = {2.0 ** -8: "1152", 2.0 ** -9: "1152", 2.0 ** -10: "4096"}[h]
    return Case(xyz, _cam(len(xyz)), s, (sample_cls,) * 3, normal=PLANE_NORMAL[normal])


# ---- E: under-determined neighbourhoods -----------------------------------------------------------------------------------
# one cluster per site, its first point the sample; offsets in lattice steps of 2^-8 m (3.9 mm), every one within three steps
# per coordinate of the sample: at most 20.3 mm away, inside the ball of 30 mm, and 0.25 m from the next cluster
CLUSTER_OFFSETS = (
    ("three", [(0, 0, 0), (2, 1, -1), (-1, 3, 2)]),
    ("four", [(0, 0, 0), (2, 1, -1), (-1, 3, 2), (1, -2, 3)]),
    ("five", [(0, 0, 0), (2, 1, -1), (-1, 3, 2), (1, -2, 3), (-3, -1, -2)]),
    ("six", [(0, 0, 0), (2, 1, -1), (-1, 3, 2), (1, -2, 3), (-3, -1, -2), (3, 2, 1)]),
    ("seven", [(0, 0, 0), (2, 1, -1), (-1, 3, 2), (1, -2, 3), (-3, -1, -2), (3, 2, 1), (-2, 2, -3)]),
    ("eight", [(0, 0, 0), (2, 1, -1), (-1, 3, 2), (1, -2, 3), (-3, -1, -2), (3, 2, 1), (-2, 2, -3), (1, 1, 2)]),
    ("coplanar4", [(0, 0, 0), (2, 1, 0), (-1, 3, 0), (-3, -2, 0)]),
    ("collinear3", [(0, 0, 0), (1, 2, -1), (-1, -2, 1)]),
    ("duplicate", [(0, 0, 0), (2, 1, -1), (-1, 3, 2), (2, 1, -1), (1, -2, 3)]),
)
CLUSTER_SIZES = tuple(len(o) for _, o in CLUSTER_OFFSETS)


def _cluster_case():
    parts, samples, n = [], [], 0
    for k, (_, offs) in enumerate(CLUSTER_OFFSETS):
        site = np.round(cc._site(k) / H8) * H8
        parts.append(site + np.asarray(offs, np.float64) * H8)
        samples.append(n)
        n += len(offs)
    xyz = _exact(np.concatenate(parts))
    return Case(xyz, _cam(n), np.array(samples, np.int32), ("1152",) * len(samples))


# ---- F: conditioning ------------------------------------------------------------------------------------------------------
FAR_CASES = ("far-plane", "far-cylinder")
UNIT = 8.0  # the scaled scene's unit: a power of two keeps every float exact
LENGTHS = dict(finger_width=0.01, hand_outer_diameter=0.09, hand_depth=0.06, hand_height=0.02, init_bite=0.01,
               nn_radius_taubin=0.03, nn_radius_hands=0.08, nn_radius_normals=0.01)  # the defaults (include/agh.h)


SCALED_HAND_DEPTH = 0.01 * UNIT + 0.07


def scaled_lengths():
    """Every length parameter of the context and of the oracle in the scaled scene's unit.  hand_depth alone cannot follow: the
    hand deepens in steps of 5 mm in any unit (finger_hand.cpp:199-204) and the context takes at most 15 of them, so the scaled
    hand is the scaled init_bite plus 14 steps deep."""
    return {**{k: v * UNIT for k, v in LENGTHS.items()}, "hand_depth": SCALED_HAND_DEPTH}


@functools.lru_cache(maxsize=None)
def scaled_scene():
    """The tilted `tiny` scene with every coordinate and both camera origins times 8."""
    from agile_grasp_amd import synthetic

    sc = synthetic.config("tiny")
    return _exact(sc.xyz.astype(np.float64) * UNIT), sc.cam, sc.cam_origins * UNIT, sc.samples


# ---- the cases by name ----------------------------------------------------------------------------------------------------
CLUSTER_CASE = "clusters"
DET_CASES = PLANE_CASES + SURFACE_CASES  # deterministic mode, one context per case
RAND50_CASES = ("plane-1152-z", "plane-1152-x", "plane-4096-z", "plane-4096-x")
RAND50_SEEDS = (1, 7)
ALL_CASES = DET_CASES + HUGE_CASES + MANY_CASES + (SPARSE_CASE,) + ALLPOINTS_CASES + (CLUSTER_CASE,) + FAR_CASES


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    part = name.split("-")
    if part[0] == "plane":
        return _plane_case(part[1], part[2])
    if name in SURFACE_CASES:
        return _surface_case(name)
    if part[0] == "many":
        return _many_case(part[1])
    if name == SPARSE_CASE:
        return _sparse_case()
    if part[0] == "allpoints":
        return _allpoints_case(part[1], part[2])
    if name == CLUSTER_CASE:
        return _cluster_case()
    if name == "far-plane":
        return _plane_case("1152", "z", centre=FAR)
    if name == "far-cylinder":
        return _surface_case("cylinder", centre=FAR, ties=False)  # (7 m out, rounding separates the mirror images' sums)
    raise KeyError(name)


def params(**kw):
    """The oracle's parameters for cc.cams(), the camera origins every case but the scaled scene uses."""
    return cc._params({}, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, mode=0, seed=1, antipodal=False):
    """The oracle's find_hands for a case (read only)."""
    from oracle import oracle_py as O

    c = case(name)
    return O.find_hands(params(normals_mode=mode, rand_seed=seed), c.xyz, c.cam, c.samples, calculates_antipodal=antipodal)


@functools.lru_cache(maxsize=None)
def all_points_frames(name):
    """The oracle's frame of every point of a case at r = 0.01 (the all-points pass; read only)."""
    from oracle import oracle_py as O

    c = case(name)
    return O.fit_frames(params(), c.xyz, c.cam, np.arange(len(c.xyz), dtype=np.int32), R_NORMALS)


@functools.lru_cache(maxsize=None)
def scaled_reference():
    from oracle import oracle_py as O

    xyz, cam, cams, s = scaled_scene()
    return O.find_hands(O.default_params(cams, num_threads=16, **scaled_lengths()), xyz, cam, s)


# ---- the independent count of tied columns --------------------------------------------------------------------------------
def gradient_normals(xyz, q, frame_params, r=R_TAUBIN):
    """Unit gradients of the frame's quadric at the points of q's ball, in float64 numpy (quadric.cpp:238-247)."""
    p = np.asarray(xyz)[cc.in_ball(xyz, q, r)].astype(np.float64)
    a, b, c = frame_params[:3]
    d, e, f = 2.0 * frame_params[3:6]
    g, h, i = frame_params[6:9]
    x, y, z = p.T
    n = np.stack([2 * a * x + d * y + f * z + g, 2 * b * y + d * x + e * z + h, 2 * c * z + e * y + f * x + i], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return n / np.linalg.norm(n, axis=1, keepdims=True)


def tied_columns(normals):
    """Columns of quadric.cpp:283-284 within the filter's margin (1e-9 n + 1e-7 max) of the largest 6th-power column sum."""
    n = len(normals)
    sums = np.empty(n)
    for j0 in range(0, n, 1024):
        g = normals @ normals[j0:j0 + 1024].T
        g *= g
        sums[j0:j0 + 1024] = (g * g * g).sum(0)
    top = sums.max()
    return int((sums >= top - (1e-9 * n + 1e-7 * abs(top))).sum())
