"""Inputs that take agh_remove_plane (csrc/plane.hip) off its defaults: parameters, inlier counts of the refit, point counts,
clouds RANSAC does not leave early, non-finite points, the threshold rule and the cloud layouts -- and the shared check
against the host restatement tests/cpp/plane_ref.cpp (tests/test_plane_clouds.py pins the regime of every case on the
restatement alone, tests/test_gpu_plane_edges.py runs them on the GPU; tests/test_gpu_plane.py checks through `check`).

Plain numpy, no GPU for the builders.  The case tables tie each case to the constant of plane.hip it sits on.
"""
from __future__ import annotations

import numpy as np

from tests import plane_ref_lib as R

DEFAULTS = dict(max_iterations=100, threshold=0.01, probability=0.99, seed=12345, optimize=True)


def bits(a):
    """float32 values as their uint32 patterns (NaN rows compare equal to themselves, -0 differs from +0)."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def value_bits(a):
    """bits() for COMPUTED values: every NaN becomes the one pattern 0x7fc00000.  IEEE 754 leaves the sign and payload of a NaN
    that an operation produces open, and the host and the GPU use that freedom differently (on the non-finite blob 22 of 101
    candidate planes differ in the sign bit of a NaN, 0xffc00000 against 0x7fc00000, and in nothing else); no comparison and
    no count can depend on those bits.  Points that are only copied (the kept cloud) are compared with bits()."""
    b = bits(a).copy()
    b[np.isnan(np.ascontiguousarray(a, np.float32))] = 0x7FC00000
    return b


def check(ctx, xyz, cam, by_position, **params):
    """remove_plane on the context's cloud (xyz, cam as the context holds them; xyz may carry padding columns, cam may be
    None) against the restatement run with the same parameters; returns the GPU result.  Floats are compared as bits (value_bits for computed planes, bits for copied points)."""
    from agile_grasp_amd import binding

    p = {**DEFAULTS, **params}
    pts = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    ids = np.zeros(len(pts), np.int32) if cam is None else np.asarray(cam, np.int32)
    ref = R.segment(pts, **p)
    res = ctx.remove_plane(max_iterations=p["max_iterations"], distance_threshold=p["threshold"], probability=p["probability"],
                           seed=p["seed"], optimize=p["optimize"], cam_ids_by_position=by_position)
    assert res["found"] == ref["found"]
    assert res["iterations"] == ref["iterations"]
    g = ctx.plane_candidates()
    k = ref["planes"].shape[0]
    assert g["planes"].shape[0] >= k
    assert np.array_equal(value_bits(g["planes"][:k]), value_bits(ref["planes"]))
    assert np.array_equal(g["samples"][:k], ref["samples"]) and np.array_equal(g["counts"][:k], ref["counts"])
    if not ref["found"]:
        assert res["n_remaining"] == len(pts) and res["n_inliers"] == 0
        assert ctx.plane_inliers().size == 0
        vx, vc = ctx.cloud()
        assert np.array_equal(bits(vx), bits(pts)) and np.array_equal(vc, ids)
        return res
    assert binding.plane_replay(g["counts"], len(pts), p["max_iterations"], p["probability"]) == (ref["best"], ref["iterations"])
    assert np.array_equal(value_bits(res["coefficients"]), value_bits(ref["coefficients"]))
    assert np.array_equal(ctx.plane_inliers(), ref["inliers"])
    m = ref["mask"]
    M = int((~m).sum())
    assert res["n_inliers"] == int(m.sum()) and res["n_remaining"] == M
    kx, kc = ctx.cloud()
    assert kx.shape == (M, 3) and np.array_equal(bits(kx), bits(pts[~m]))
    assert np.array_equal(kc, ids[:M] if by_position else ids[~m])
    if cam is None:
        assert not kc.any()
    return res


# ---- builders (each returns float32 points and int32 camera ids) ---------------------------------------------------
def _cam(rng, n):
    return (rng.random(n) < 0.5).astype(np.int32)


def patch_cloud(m, k, seed, z=0.25, noise=0.0, zlo=0.3):
    """m points of the plane z = float32(z) exactly (noise > 0: plus N(0, noise), a table that the refit has to fit) with
    random x, y, and k points at z in [zlo, 0.6], all shuffled together."""
    rng = np.random.default_rng(seed)
    xyz = np.empty((m + k, 3), np.float32)
    xyz[:, :2] = rng.uniform(-0.3, 0.3, (m + k, 2))
    xyz[:m, 2] = np.float32(z)
    if noise:
        xyz[:m, 2] += np.random.default_rng([seed, 1]).normal(0.0, noise, m).astype(np.float32)  # (x, y and the rest stay)
    xyz[m:, 2] = rng.uniform(zlo, 0.6, k)
    xyz = np.ascontiguousarray(xyz[rng.permutation(m + k)])
    return xyz, _cam(rng, m + k)


def blob(n, seed):
    """n points uniform in the unit cube: no plane holds more than a few per cent of them, RANSAC runs to its cap."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)), _cam(rng, n)


def nonfinite(xyz, seed):
    """The cloud with NaN in every seventh row (one coordinate, or all three) and +-inf in some coordinates of other rows."""
    rng = np.random.default_rng(seed)
    out = np.array(xyz, np.float32, copy=True)
    rows = np.arange(0, len(out), 7)
    one = rows[::2]
    out[one, rng.integers(0, 3, one.size)] = np.nan
    out[rows[1::2], :3] = np.nan
    inf = np.arange(3, len(out), 31)
    inf = inf[inf % 7 != 0]
    out[inf, rng.integers(0, 3, inf.size)] = np.where(rng.random(inf.size) < 0.5, np.inf, -np.inf).astype(np.float32)
    return out


def threshold_probe(t, seed, n_zero=400, per=2, n_far=40):
    """Points whose distance to the plane RANSAC finds is exactly float32(t) and its two float neighbours.  n_zero points
    have z = 0.0f, so a sample of three of them gives the plane (0, 0, +-1, -+0) exactly and |dot| = |z| exactly; `per`
    points each at z = +-float32(t), +-nextafter towards 0 and +-nextafter away from 0 sit near the middle (a plane through
    one of them and two of the wide-spread z = 0 points tilts away from most of the others); n_far points lie beyond 0.3.
    Returns (xyz, cam, probes): probes maps "at" / "below" / "above" to the rows of those points."""
    rng = np.random.default_rng(seed)
    f = np.float32(t)
    levels = {"at": f, "below": np.nextafter(f, np.float32(0.0)), "above": np.nextafter(f, np.float32(np.inf))}
    parts, kinds = [], []
    zero = np.zeros((n_zero, 3), np.float32)
    zero[:, :2] = rng.uniform(-1.0, 1.0, (n_zero, 2))
    parts.append(zero)
    kinds += ["zero"] * n_zero
    for name, v in levels.items():
        for sign in (1.0, -1.0):
            q = np.zeros((per, 3), np.float32)
            q[:, :2] = rng.uniform(-0.05, 0.05, (per, 2))
            q[:, 2] = np.float32(sign) * v
            parts.append(q)
            kinds += [name] * per
    far = np.zeros((n_far, 3), np.float32)
    far[:, :2] = rng.uniform(-1.0, 1.0, (n_far, 2))
    far[:, 2] = rng.uniform(0.3, 0.6, n_far) * np.where(rng.random(n_far) < 0.5, 1.0, -1.0)
    parts.append(far)
    kinds += ["far"] * n_far
    xyz = np.concatenate(parts)
    perm = rng.permutation(len(xyz))
    xyz = np.ascontiguousarray(xyz[perm])
    kinds = np.array(kinds)[perm]
    return xyz, _cam(rng, len(xyz)), {name: np.nonzero(kinds == name)[0] for name in levels}


def padded(xyz, fill=7.0):
    """The points as the first three columns of an (n, 8) array (32 bytes per point) whose other columns hold `fill`."""
    out = np.full((len(xyz), 8), fill, np.float32)
    out[:, :3] = xyz
    return out


# ---- the cases (shared by the CPU regime check and the GPU tests) ----------------------------------------------------
# inliers of the chosen plane, on k_plane_moments' edges (kPlaneChunk = 512, sums four at a time with a scalar tail; the refit
# needs 4): m -> (k outliers, seed, lowest outlier z).  k = m // 3 + 5; seed = m and z from 0.3, except for 3 and 4, where a
# plane through other points then held one point more (nine or ten points leave few seeds without such a plane).
COUNT_CASES = {3: (6, 231, 0.4), 4: (6, 17, 0.4), 5: (6, 5, 0.3), 6: (7, 6, 0.3), 7: (7, 7, 0.3), 511: (175, 511, 0.3),
               512: (175, 512, 0.3), 513: (176, 513, 0.3), 1023: (346, 1023, 0.3), 1024: (346, 1024, 0.3),
               1025: (346, 1025, 0.3)}
COUNT_ROUGH = 2e-4  # sigma of the rough variant's patch: far inside the threshold, the counts stay
COUNT_ORDER = (1025, 3, 512, 1024, 4, 513, 5, 1023, 6, 511, 7)  # on one context: d_terms shrinks and grows in use
# cloud sizes: the smallest that draws; the 256-point tile of k_plane_count / _terms / _split; a k_plane_score work-group's
# 256 x 8 points; k_plane_scan's per = 1 -> 2 at 1024 / 1025 tiles.  262145 first, then 3: stale tile counts beyond nblk.
POINT_COUNTS = (262145, 3, 255, 256, 257, 2047, 2048, 2049, 262144)
BLOB_N, BLOB_SEED = 3000, 12345
# (name, parameters) in the order the GPU runs them on one context: the candidates and counts of the longest run lie behind
# the shorter ones; "same_cloud" cases run on the cloud the case before left (threshold 0 keeps all of it: the other slot)
BLOB_CASES = (
    ("max_iterations_1023", dict(max_iterations=1023)),
    ("max_iterations_0", dict(max_iterations=0)),
    ("defaults", dict()),
    ("max_iterations_1", dict(max_iterations=1)),
    ("probability_low", dict(probability=1e-9)),
    ("probability_high", dict(probability=1.0 - 1e-12)),
    ("optimize_off", dict(optimize=False)),
    ("threshold_0", dict(threshold=0.0)),
    ("seed_7", dict(seed=7)),
    ("threshold_10", dict(threshold=10.0)),
)
BLOB_ON_KEPT_CLOUD = ("seed_7",)  # runs without a set_cloud, on what threshold_0 kept
NONFINITE_SEED = 5
PROBE_CASES = {0.01: 2, 0.05: 0}  # threshold -> seed; float32(0.01) < 0.01, float32(0.05) > 0.05
REFUSALS = (dict(max_iterations=-1), dict(max_iterations=1024), dict(probability=0.0), dict(probability=1.0),
            dict(probability=float("nan")), dict(threshold=-1.0), dict(threshold=float("nan")))


def count_cloud(m, rough=False):
    """The m-inlier case.  With the patch at one exact z the refit's answer depends on the z sums alone (the covariance's z row is
    exactly zero); rough: the same cloud with COUNT_ROUGH of noise on the patch, where all nine sums and their order matter."""
    k, seed, zlo = COUNT_CASES[m]
    return patch_cloud(m, k, seed, zlo=zlo, noise=COUNT_ROUGH if rough else 0.0)


def point_cloud(n):
    """n points, 60 % of them a noisy table (sigma 2 mm) in every tile of the cloud; n = 3: the three points of a plane."""
    if n == 3:
        return patch_cloud(3, 0, 3)
    m = n * 6 // 10
    return patch_cloud(m, n - m, n, noise=0.002)


def blob_cloud():
    return blob(BLOB_N, BLOB_SEED)


def nonfinite_cloud():
    xyz, cam = blob_cloud()
    return nonfinite(xyz, NONFINITE_SEED), cam


def probe_cloud(t):
    return threshold_probe(t, PROBE_CASES[t])
