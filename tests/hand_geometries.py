"""Hand geometries off the node's defaults, and three small clouds that take the hand search to the ends of its tables
(tests/test_hand_geometries.py pins every property on the CPU; tests/test_gpu_hand_geometries.py runs them on the GPU).

Plain numpy, no GPU.  `derive` restates what build_geometry (csrc/api.hip) makes of a geometry: the de-duplicated list of
finger-slot thresholds, the `d += 0.005` bite depths and the look-up cell formula.  It classifies the fixtures -- which
kernel instantiation a geometry selects, how many compares a cell needs, whether creation is refused -- and is the
reference for no result: every result is compared with the oracle.
"""
from __future__ import annotations

import numpy as np

DEFAULTS = dict(finger_width=0.01, hand_outer_diameter=0.09, hand_depth=0.06, hand_height=0.02, init_bite=0.01)
LUT_PROBE = 4  # kLutProbe: thresholds (or depths) one look-up cell may hold
MAX_DEPTHS = 16  # HandGeom::depths
X_CELLS, Y_CELLS = 1024, 64


def params(geom):
    return {**DEFAULTS, **geom}


def thresholds(fw, od):
    """The sorted, de-duplicated slot edges fs_i and fs_i + fw of the 20 finger placements (finger_hand.cpp:8-15, 63, 77)."""
    high = od - fw
    fstep = (high - 0.0) / 9.0
    fs = np.zeros(20)
    for i in range(10):
        h = 0.0 + i * fstep
        fs[i] = (h - od) + fw
        fs[10 + i] = h
    return fs, np.unique(np.concatenate([fs, fs + fw]))


def depths(init_bite, hand_depth):
    """init_bite, then repeated += 0.005 while <= hand_depth (finger_hand.cpp:199-204), however many that gives."""
    out = [init_bite]
    d = init_bite + 0.005
    while d <= hand_depth:
        out.append(d)
        d += 0.005
    return np.array(out)


def cells(tab, ncell):
    """(int) fmin(fmax((v - lo) * scale, 0), ncell - 1) of every table entry."""
    lo, hi = tab[0], tab[-1]
    scale = ncell / (hi - lo) if hi > lo else 0.0
    return np.array([int(min(max((v - lo) * scale, 0.0), float(ncell - 1))) for v in tab]), scale


def derive(geom):
    """What build_geometry derives: n_thr, the fullest x and y cells, n_depths, and `refused` (None, "depths", "cell")."""
    p = params(geom)
    fs, t = thresholds(p["finger_width"], p["hand_outer_diameter"])
    d = depths(p["init_bite"], p["hand_depth"])
    refused = "depths" if len(d) > MAX_DEPTHS else None
    d = d[:MAX_DEPTHS]
    xc, _ = cells(t, X_CELLS)
    yc, yscale = cells(d, Y_CELLS)
    x_probes, y_probes = int(np.bincount(xc).max()), int(np.bincount(yc).max())
    if refused is None and max(x_probes, y_probes) > LUT_PROBE:
        refused = "cell"
    return dict(n_thr=len(t), x_probes=x_probes, y_probes=y_probes, n_depths=len(d), ylut_scale=yscale, refused=refused,
                few=x_probes <= 2 and y_probes <= 1)


# name -> (parameters that differ from DEFAULTS, the properties the name stands for)
TABLE = {
    "default": ({}, dict(n_thr=40, x_probes=2, n_depths=11, refused=None)),
    "one_per_cell": (dict(finger_width=0.015, hand_outer_diameter=0.105, hand_depth=0.05, init_bite=0.02, hand_height=0.03),
                     dict(n_thr=38, x_probes=1, n_depths=7, refused=None)),
    "three_a": (dict(finger_width=0.01, hand_outer_diameter=0.1), dict(n_thr=30, x_probes=3, n_depths=11, refused=None)),
    "three_b": (dict(finger_width=0.0225, hand_outer_diameter=0.09), dict(n_thr=34, x_probes=3, n_depths=11, refused=None)),
    "four": (dict(finger_width=0.0898, hand_outer_diameter=0.09), dict(x_probes=4, n_depths=11, refused=None)),
    "one_depth": (dict(init_bite=0.058), dict(x_probes=2, n_depths=1, refused=None)),
    "two_depths": (dict(init_bite=0.055), dict(x_probes=2, n_depths=2, refused=None)),
    "sixteen_depths": (dict(init_bite=0.005, hand_depth=0.08), dict(x_probes=2, n_depths=16, refused=None)),
    "refused_depths": (dict(init_bite=0.005, hand_depth=0.086), dict(refused="depths")),
    "refused_cell": (dict(finger_width=0.0998, hand_outer_diameter=0.1), dict(x_probes=5, refused="cell")),
}
ACCEPTED = tuple(k for k, (_, want) in TABLE.items() if want["refused"] is None)
REFUSED = tuple(k for k, (_, want) in TABLE.items() if want["refused"] is not None)
GENERAL = tuple(k for k in ACCEPTED if not derive(TABLE[k][0])["few"])  # the kLutProbe instantiations' geometries
# the clouds each accepted geometry runs on: together they reach both ends of its bite-depth table (tiny's hands seldom
# deepen to the end, the rod's always can; one_depth and two_depths find next to nothing on tiny, three_b's wide fingers too)
CLOUDS = {
    "default": ("tiny", "rod"), "one_per_cell": ("tiny", "rod"), "three_a": ("tiny", "rod", "plate", "sheets"), "three_b": ("rod", "plate"),
    "four": ("tiny", "rod", "plate"), "one_depth": ("rod",), "two_depths": ("rod",), "sixteen_depths": ("tiny", "rod"),
}
EMPTY = ("four",)  # the oracle finds no hand with it on any of the clouds


def geom(name):
    return dict(TABLE[name][0])


# ---- the clouds ----------------------------------------------------------------------------------------------------
N_SAMPLES = 96
GRID, JITTER = 0.003, 0.0002


def _finish(pts, seed):
    rng = np.random.default_rng(seed)
    xyz = (pts + rng.uniform(-JITTER, JITTER, pts.shape)).astype(np.float32)
    cam = (np.arange(len(xyz)) % 2).astype(np.int32)  # the cameras alternate
    samples = np.sort(rng.permutation(len(xyz))[:N_SAMPLES]).astype(np.int32)
    return np.ascontiguousarray(xyz), cam, samples


def rod():
    """A vertical cylinder of radius 1 cm and height 0.2 m at x = 0.6 on a 3 mm grid: thin enough for every hand to close
    around it at any depth, so the deepening runs to the end of the table."""
    r, h = 0.01, 0.2
    na = int(round(2 * np.pi * r / GRID))
    a, z = np.meshgrid(np.arange(na) * (2 * np.pi / na), np.arange(0.0, h, GRID) - h / 2, indexing="ij")
    pts = np.stack([0.6 + r * np.cos(a.ravel()), r * np.sin(a.ravel()), z.ravel()], 1)
    return _finish(pts, 41)


def plate():
    """Both faces of a 4 mm thick plate of 0.12 m x 0.16 m at x = 0.6: hands that close over an edge, at many finger slots."""
    u, v = np.meshgrid(np.arange(0.0, 0.12, GRID) - 0.06, np.arange(0.0, 0.16, GRID) - 0.08, indexing="ij")
    face = np.stack([np.zeros(u.size), u.ravel(), v.ravel()], 1)
    pts = np.concatenate([face + [0.598, 0, 0], face + [0.602, 0, 0]])
    return _finish(pts, 43)


SHEET_OFFSETS = (-0.05, 0.0, 0.05)
SHEET_JITTER = 5e-5  # across the sheets; GRID / JITTER within them


def sheets():
    """Three parallel sheets of 0.12 m x 0.16 m, 5 cm apart and flat to 0.05 mm; the samples lie on the middle one.  Seen
    along the sheet (orientations 0 and 4) every point of the middle sheet has a hand-frame x within 0.05 mm of zero -- for
    three_a inside the look-up cell that holds its three thresholds next to zero (fs_10 = 0 and the two sums that round to
    1e-17) -- and nothing else lies in the slot (0, 0.01) of finger 9.  Whether that finger is blocked hangs on the cell's
    third compare: the sheet 5 cm in front gives the finger its point beyond the slot, the outer sheets block hands 3 to 5,
    and the hand picked is 2 of {1, 2, 6, 7} -- 6 of {1, 2, 6, 7, 9} for a sweep that compares twice."""
    rng = np.random.default_rng(1)
    parts = []
    for d in SHEET_OFFSETS:
        u, v = np.meshgrid(np.arange(0.0, 0.12, GRID) - 0.06, np.arange(0.0, 0.16, GRID) - 0.08, indexing="ij")
        shift = rng.uniform(0, GRID, 2)
        p = np.stack([np.full(u.size, 0.6 + d), u.ravel() + shift[0], v.ravel() + shift[1]], 1)
        p[:, 0] += rng.uniform(-SHEET_JITTER, SHEET_JITTER, len(p))
        p[:, 1:] += rng.uniform(-JITTER, JITTER, (len(p), 2))
        parts.append(p)
    xyz = np.concatenate(parts).astype(np.float32)
    cam = (np.arange(len(xyz)) % 2).astype(np.int32)
    n1 = len(parts[0])
    samples = np.sort(n1 * SHEET_OFFSETS.index(0.0) + rng.permutation(n1)[:N_SAMPLES]).astype(np.int32)
    return np.ascontiguousarray(xyz), cam, samples


def cloud(name):
    """(xyz, cam, samples) of `tiny`, `rod`, `plate` or `sheets`; all are searched with tiny's camera origins."""
    if name == "tiny":
        from agile_grasp_amd import synthetic

        sc = synthetic.config("tiny")
        return sc.xyz, sc.cam, sc.samples
    return {"rod": rod, "plate": plate, "sheets": sheets}[name]()


def cam_origins():
    from agile_grasp_amd import synthetic

    return synthetic.to_scene_frame(synthetic.camera_origins())


PADDED_SAMPLES = 4100  # more than kSweepWg4MinSamples


SHEETS_SHIFT = np.array([0.0, 1.0, 0.0], np.float32)  # clear of tiny


def padded_tiny():
    """tiny, the sheets beside it, and their sample lists padded to PADDED_SAMPLES the way capacity_clouds.tile_cloud("wg4")
    pads: the further samples are the points of a filler patch of their own, beyond the reach of every ball of the others.
    Returns (xyz, cam, samples, n_tiny, n_own): samples [0, n_tiny) are tiny's, [n_tiny, n_own) the sheets'."""
    from tests import capacity_clouds as cc

    xyz, cam, s = cloud("tiny")
    xs, cs, ss = sheets()
    rng = np.random.default_rng(47)
    n_own = len(s) + len(ss)
    pad = PADDED_SAMPLES - n_own
    n = len(xyz) + len(xs)
    xyz = np.concatenate([xyz, xs + SHEETS_SHIFT])
    centre = np.array([xyz[:, 0].mean(), xyz[:, 1].max() + 0.5, xyz[:, 2].mean()], np.float64)
    fill = cc._surface(rng, centre, pad, 0.1, noise=2e-3).astype(np.float32)
    return (np.ascontiguousarray(np.concatenate([xyz, fill])), np.concatenate([cam, cs, (rng.random(pad) < 0.5).astype(np.int32)]),
            np.concatenate([s, ss + len(cam), np.arange(n, n + pad, dtype=np.int32)]), len(s), n_own)


_REFERENCE = {}


def reference(name, cloud_name, mode):
    """The oracle's result for a geometry on a cloud, computed once: mode "plain" and "antipodal" give find_hands with
    images, "training" find_hands_training and the frames of the samples."""
    import os

    from oracle import oracle_py as O

    key = (name, cloud_name, mode)
    if key not in _REFERENCE:
        xyz, cam, s = cloud(cloud_name)
        p = O.default_params(cam_origins(), num_threads=min(os.cpu_count() or 1, 16), **geom(name))
        if mode == "training":
            ref = O.find_hands_training(p, xyz, cam, s)
            ref["frames"] = O.fit_frames(p, xyz, cam, s, p.nn_radius_taubin)
        else:
            ref = O.find_hands(p, xyz, cam, s, calculates_antipodal=mode == "antipodal", want_images=True)
        _REFERENCE[key] = ref
    return _REFERENCE[key]
