"""The plane-removal inputs (tests/plane_clouds.py) reach the regime each one names, on the restatement alone.

CPU only.  tests/test_gpu_plane_edges.py holds the GPU to the restatement on these cases bit for bit; what is asserted here is
that the restatement, and so a GPU that agrees with it, is then on the count, the branch or the float neighbour that the case
is there for.  A case that stops meeting its condition fails here and wants another seed in the case table.
"""
import functools
import os
import re

import numpy as np
import pytest

from tests import plane_clouds as pc
from tests import plane_ref_lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _blob(name):
    xyz, _ = pc.blob_cloud()
    return R.segment(xyz, **dict(pc.BLOB_CASES)[name])


def test_tables_sit_on_the_constants_of_plane_hip():
    with open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "plane.hip")) as f:
        src = f.read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))

    chunk, cand, per_thread = const("kPlaneChunk"), const("kPlaneMaxCand"), const("kPlaneScorePts")
    counts = set(pc.COUNT_CASES)
    assert {3, 4, 5, 6, 7} <= counts  # no refit below 4 inliers (counts[best] >= 4); tails of 1 to 3 behind one float4
    assert re.search(r"P\.counts\[\(size_t\) best\] >= 4\)", src)
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1} <= counts
    assert set(pc.COUNT_ORDER) == counts and len(pc.COUNT_ORDER) == len(counts)
    sizes = set(pc.POINT_COUNTS)
    assert pc.POINT_COUNTS[:2] == (262145, 3)
    assert {3, 255, 256, 257} <= sizes and re.search(r"const int64_t nblk = \(n \+ 255\) / 256;", src)
    assert {256 * per_thread - 1, 256 * per_thread, 256 * per_thread + 1} <= sizes
    assert re.search(r"const int per = \(nblk \+ 1023\) / 1024;", src) and {256 * 1024, 256 * 1024 + 1} <= sizes
    its = [p.get("max_iterations", 100) for _, p in pc.BLOB_CASES]
    assert its[:3] == [cand - 1, 0, 100] and 1 in its
    bad_its = [p["max_iterations"] for p in pc.REFUSALS if "max_iterations" in p]
    assert sorted(bad_its) == [-1, cand]
    for name in pc.BLOB_ON_KEPT_CLOUD:  # the case before it keeps the whole cloud
        names = [n for n, _ in pc.BLOB_CASES]
        assert names[names.index(name) - 1] == "threshold_0"


@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("m", sorted(pc.COUNT_CASES))
def test_inlier_count_cases(m, rough):
    xyz, cam = pc.count_cloud(m, rough)
    k = pc.COUNT_CASES[m][0]
    assert k == m // 3 + 5 and xyz.shape == (m + k, 3) and cam.shape == (m + k,) and set(cam.tolist()) == {0, 1}
    r = R.segment(xyz)
    assert r["found"] and r["counts"][r["best"]] == m and r["counts"].max() == m and len(r["inliers"]) == m
    if m >= 4:  # the refit ran, over the patch: its points in inlier order are the nine chains' input
        z = xyz[r["inliers"], 2]
        assert (np.abs(z - np.float32(0.25)) < 0.002).all() and (np.unique(z).size > 1) == rough
        if rough:
            assert not np.array_equal(pc.bits(r["coefficients"]), pc.bits(r["planes"][r["best"]]))
    else:
        assert np.array_equal(pc.bits(r["coefficients"]), pc.bits(r["planes"][r["best"]]))


@pytest.mark.parametrize("n", pc.POINT_COUNTS)
def test_point_count_cases(n):
    xyz, cam = pc.point_cloud(n)
    assert xyz.shape == (n, 3) and xyz.dtype == np.float32 and cam.shape == (n,)
    r = R.segment(xyz)
    assert r["found"]
    if n == 3:
        assert len(r["inliers"]) == 3
        return
    assert 0.5 * n < len(r["inliers"]) < 0.7 * n
    tiles = np.add.reduceat(r["mask"].astype(np.int64), np.arange(0, n, 256))
    assert (tiles[:-1] > 0).all() and (tiles[:-1] < 256).all()  # every full tile splits: inliers and kept points in each


def test_blob_runs_to_the_cap():
    r = _blob("defaults")
    assert r["found"] and r["iterations"] == 101 and len(r["counts"]) == 101
    assert r["counts"].max() < 0.05 * pc.BLOB_N
    r = _blob("max_iterations_1023")
    assert r["found"] and r["iterations"] == 1024 and len(r["counts"]) == 1024
    # 3 draws per candidate, 624 per generator state: the chosen plane was drawn after the second refill
    assert r["best"] > 208 and (r["samples"] >= 0).all()


def test_blob_parameter_cases():
    base = _blob("defaults")
    r = _blob("max_iterations_0")
    assert not r["found"] and len(r["counts"]) == 0 and r["iterations"] == 0
    assert _blob("max_iterations_1")["iterations"] == 2
    assert _blob("probability_low")["iterations"] == 1
    assert _blob("probability_high")["iterations"] == 101
    for name in ("seed_7", "optimize_off"):
        r = _blob(name)
        assert r["found"] and not np.array_equal(r["coefficients"], base["coefficients"])
    assert not np.array_equal(_blob("seed_7")["samples"], base["samples"])
    r = _blob("optimize_off")
    assert np.array_equal(r["samples"], base["samples"]) and not np.array_equal(r["mask"], base["mask"])
    r = _blob("threshold_0")
    assert r["found"] and r["iterations"] == 101 and not r["counts"].any() and len(r["inliers"]) == 0
    r = _blob("threshold_10")
    assert r["found"] and r["iterations"] == 1 and len(r["inliers"]) == pc.BLOB_N
    assert {n for n, _ in pc.BLOB_CASES} == {"defaults", "max_iterations_1023", "max_iterations_0", "max_iterations_1",
                                             "probability_low", "probability_high", "seed_7", "optimize_off", "threshold_0",
                                             "threshold_10"}


def test_nonfinite_blob():
    xyz, _ = pc.nonfinite_cloud()
    bad = ~np.isfinite(xyz).all(1)
    assert np.isnan(xyz[::7]).any(1).all() and np.isinf(xyz).any() and (xyz == -np.inf).any() and (xyz == np.inf).any()
    assert 0.1 * len(xyz) < bad.sum() < 0.25 * len(xyz)
    r = R.segment(xyz)
    nan_plane = np.isnan(r["planes"]).any(1)
    assert r["found"] and nan_plane[:r["best"]].any() and nan_plane[r["best"] + 1:].any()
    assert (r["counts"][nan_plane] == 0).all() and not r["mask"][bad].any() and len(r["inliers"]) >= 4
    assert np.isfinite(r["coefficients"]).all()


@pytest.mark.parametrize("t", sorted(pc.PROBE_CASES))
def test_threshold_probes(t):
    xyz, cam, probes = pc.probe_cloud(t)
    f = np.float32(t)
    assert (float(f) < t) == (t == 0.01) and float(f) != t
    for name, want in (("at", f), ("below", np.nextafter(f, np.float32(0))), ("above", np.nextafter(f, np.float32(1)))):
        z = xyz[probes[name], 2]
        assert np.array_equal(np.abs(z), np.full(z.size, want, np.float32)) and (z > 0).any() and (z < 0).any()
    r = R.segment(xyz, threshold=t, optimize=False)
    assert r["found"]
    c = r["planes"][r["best"]]
    assert (pc.bits(c) & 0x7fffffff).tolist() == [0, 0, 0x3f800000, 0]  # (0, 0, +-1, +-0): |dot| is |z| exactly
    assert np.array_equal(pc.bits(r["coefficients"]), pc.bits(c))
    m = r["mask"]
    assert m[probes["at"]].all() if float(f) < t else not m[probes["at"]].any()
    assert m[probes["below"]].all() and not m[probes["above"]].any()
    # threshold 0 on the same cloud: the z = 0 points lie ON candidate planes (dot = +-0) and still are no inliers
    r = R.segment(xyz, threshold=0.0)
    on_plane = ((pc.bits(r["planes"]) & 0x7fffffff) == np.array([0, 0, 0x3f800000, 0], np.uint32)).all(1)
    assert r["found"] and on_plane.any() and not r["counts"].any() and len(r["inliers"]) == 0


def test_padded_layout_keeps_the_points():
    xyz, _ = pc.count_cloud(513)
    p = pc.padded(xyz)
    assert p.shape == (len(xyz), 8) and p.flags["C_CONTIGUOUS"] and np.array_equal(p[:, :3], xyz) and (p[:, 3:] == 7.0).all()
    a, b = R.segment(p), R.segment(xyz)
    assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(pc.bits(a["coefficients"]), pc.bits(b["coefficients"]))
