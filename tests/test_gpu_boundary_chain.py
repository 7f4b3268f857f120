"""Localization::filterHands (localization.cpp:364-388) as a device stage of the fused localize chain: agh_localize* with
filters_boundaries = 1, the configuration the reference's nodes ship (grasp_localizer.cpp:21, nodes/test.cpp:72).  Every
result is held against the stage-wise calls with the filter restated in numpy, and every scene is one where the filter bites:
a workspace face cuts through it (as in tests/test_boundary.py), so that hypotheses, SVM-positive ones among them, are dropped."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT, _dump_raw, _preprocess_numpy, _raw_cloud
from tests.test_preprocess import HANDLE_FIELDS, HYP_FIELDS

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")
FIELDS = HYP_FIELDS + ("valid",)  # (the epoch stamps the context's own search)


def _scene():
    xyz, size_left, ws, cams = _raw_cloud()
    ws = ws.copy()
    ws[1] = 0.8  # cuts through the scene
    return xyz, size_left, ws, cams


def _near(hyps, ws):
    """Localization::filterHands' test, restated: within MIN_DIST = 0.02 of some face, strictly."""
    s = hyps["surface"]
    near = np.zeros(len(hyps), bool)
    for k in range(6):
        near |= np.abs(s[:, k // 2] - ws[k]) < 0.02
    return near


def _stagewise(ctx, xyz, size_left, ws, samples, classify):
    """find_hands -> classify -> filterHands (numpy) -> find_handles on the same samples: the hands the chain must return,
    its handles and inlier lists, and the numbers that say whether the filter bit."""
    ctx.preprocess(xyz, size_left, ws)
    hyps = ctx.find_hands(samples)
    keep = ctx.classify().astype(bool)
    hyps = hyps.copy()
    near = _near(hyps, ws)
    if classify:
        hyps["svm_keep"] = keep
        h = hyps[keep & ~near]
    else:
        h = hyps[~near]
    hd, idx = ctx.find_handles(h, 2, 0.005)
    bite = dict(n_hyp=len(hyps), near=int(near.sum()), kept_near=int((keep & near).sum()), survivors=len(h))
    return h, hd, idx, bite


def _assert_bites(bite):
    assert bite["near"] >= 3 and bite["kept_near"] >= 1 and bite["survivors"] >= 1, bite


def _assert_same(got, h, hd, idx):
    assert len(got["hands"]) == len(h)
    for f in FIELDS:
        assert np.array_equal(got["hands"][f], h[f]), f
    assert len(got["handles"]) == len(hd) and np.array_equal(got["inlier_idx"], idx)
    for f in HANDLE_FIELDS:
        assert np.array_equal(got["handles"][f], hd[f]), f


def _contexts(cams, svm_model, n=2, general=False):
    from agile_grasp_amd import binding

    out = []
    for _ in range(n):
        c = binding.Context(cams)
        if general:  # the same weights as two support vectors of a LINEAR model: the general path (descriptors, kernel rows)
            w, rho = svm_model
            c.load_svm_model(binding.SVM_LINEAR, np.stack([w, w]), np.array([0.5, 0.5]), rho)
        else:
            c.load_svm(*svm_model)
        out.append(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["linear", "general"])
def test_one_call_equals_search_classify_filter_handles(svm_model, model):
    xyz, size_left, ws, cams = _scene()
    one, chain = _contexts(cams, svm_model, general=model == "general")
    got = one.localize(xyz, size_left, ws, n_samples=600, sample_seed=3, classify=True, min_inliers=2, filters_boundaries=True)
    h, hd, idx, bite = _stagewise(chain, xyz, size_left, ws, got["samples"], True)
    _assert_bites(bite)
    assert got["n_hypotheses"] == bite["n_hyp"]  # the search's unfiltered count
    _assert_same(got, h, hd, idx)
    assert np.all(got["hands"]["svm_keep"] == 1)
    # the same capture unfiltered, on the same context: the flag is per call
    plain = one.localize(xyz, size_left, ws, n_samples=600, sample_seed=3, classify=True, min_inliers=2)
    assert len(plain["hands"]) == len(h) + bite["kept_near"]


@pytest.mark.gpu
def test_unclassified_chain_drops_the_filtered_hands(svm_model):
    xyz, size_left, ws, cams = _scene()
    one, chain = _contexts(cams, svm_model)
    vox, _ = _preprocess_numpy(xyz, size_left, ws)
    samples = np.sort(np.random.default_rng(5).permutation(len(vox))[:500]).astype(np.int32)
    got = one.localize(xyz, size_left, ws, samples=samples, classify=False, min_inliers=2, filters_boundaries=True)
    h, hd, idx, bite = _stagewise(chain, xyz, size_left, ws, samples, False)
    _assert_bites(bite)
    assert got["n_hypotheses"] == bite["n_hyp"] and bite["survivors"] == bite["n_hyp"] - bite["near"]
    _assert_same(got, h, hd, idx)


def _crop(xyz, size_left, lo, hi):
    """The points of a capture inside a box (NaN rows go: they compare false), camera split kept."""
    with np.errstate(invalid="ignore"):
        m = np.all((xyz >= lo) & (xyz <= hi), axis=1)
    return np.ascontiguousarray(xyz[m]), int(m[:size_left].sum())


def _captures():
    """Three captures, the first a small crop (its lattice sizes a context's voxel bitmap), the second the whole scene (its
    lattice outgrows that bitmap: the chain's speculative voxelisation fails and the whole call repeats), the third another
    draw of the scene."""
    xyz, size_left, ws, cams = _scene()
    fin = xyz[np.isfinite(xyz).all(1)]
    lo, hi = np.percentile(fin, 30, axis=0), np.percentile(fin, 70, axis=0)
    lo[0], hi[0] = 0.7, 0.85  # (across the cutting face)
    small = _crop(xyz, size_left, lo, hi)
    xyz2, size_left2, _, _ = _raw_cloud(seed=12)
    return [small, (xyz, size_left), (xyz2, size_left2)], ws, cams


@pytest.mark.gpu
def test_staged_stream_equals_the_one_call_per_capture(svm_model):
    caps, ws, cams = _captures()
    one, two, chain = _contexts(cams, svm_model, n=3)
    kw = [dict(n_samples=400, sample_seed=31 + i, classify=True, min_inliers=2, filters_boundaries=True) for i in range(3)]
    clouds = [c for c, _ in caps]
    got = []
    two.localize_begin(clouds[0], caps[0][1], ws, **kw[0])
    for i in range(3):
        if i + 1 < 3:
            two.localize_stage(clouds[i + 1])
        got.append(two.localize_end())
        if i + 1 < 3:
            two.localize_begin(clouds[i + 1], caps[i + 1][1], ws, **kw[i + 1])
    assert got[1]["n_voxels"] > 2 * got[0]["n_voxels"]
    for i, (xyz, size_left) in enumerate(caps):
        ref = one.localize(xyz, size_left, ws, **kw[i])
        g = got[i]
        assert g["n_voxels"] == ref["n_voxels"] and g["n_hypotheses"] == ref["n_hypotheses"] > 0
        assert np.array_equal(g["samples"], ref["samples"])
        _assert_same(g, ref["hands"], ref["handles"], ref["inlier_idx"])
        if i >= 1:  # the whole scene: the chain is the stage-wise one, and (second capture) the filter bites
            h, hd, idx, bite = _stagewise(chain, xyz, size_left, ws, g["samples"], True)
            _assert_same(g, h, hd, idx)
            if i == 1:
                _assert_bites(bite)


@pytest.mark.gpu
def test_invalid_flag_is_refused(svm_model):
    from agile_grasp_amd import binding

    xyz, size_left, ws, cams = _scene()
    (ctx,) = _contexts(cams, svm_model, n=1)
    for bad in (2, -1):
        with pytest.raises(binding.AghError) as e:
            ctx.localize(xyz, size_left, ws, n_samples=64, filters_boundaries=bad)
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "filters_boundaries" in str(e.value)
    # the context goes on working, filtered and not
    got = ctx.localize(xyz, size_left, ws, n_samples=200, sample_seed=9, min_inliers=2, filters_boundaries=True)
    assert got["n_hypotheses"] > 0


def _build(tmp_path):
    from agile_grasp_amd import build

    build.build()
    exe = str(tmp_path / "boundary_chain_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "boundary_chain_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _rows(lines, tag):
    return [l.split()[1:] for l in lines if l.startswith(tag + " ")]


@pytest.mark.gpu
def test_adapter_chain_equals_the_three_calls(tmp_path, svm_model):
    """Localization(4, true, 0): localizeHandles (the fused chain, filtered on the device) returns what the node's three calls
    return -- localizeHands (filtered on the host) -> predictAntipodalHands -> findHandles -- and stageNextCloud works."""
    exe = _build(tmp_path)
    xyz, size_left, ws, cams = _scene()
    vox, vcam = _preprocess_numpy(xyz, size_left, ws)
    idx = np.sort(np.random.default_rng(2).permutation(len(vox))[:400]).astype(np.int32)
    path = str(tmp_path / "raw.bin")
    _dump_raw(path, xyz, size_left, idx, ws, cams)
    out = subprocess.run([exe, "chain", SVM, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    (ctx,) = _contexts(cams, svm_model, n=1)
    ctx.set_cloud(vox, vcam)
    hyps = ctx.find_hands(idx)
    keep = ctx.classify().astype(bool)
    near = _near(hyps, ws)
    _assert_bites(dict(near=int(near.sum()), kept_near=int((keep & near).sum()), survivors=int((keep & ~near).sum())))
    assert _rows(lines, "HANDS") == [[str(int((~near).sum()))]]  # localizeHands' host filterHands
    c1 = _rows(lines, "CHAIN1")
    assert _rows(lines, "CHAIN3") == c1 and c1[0][0] == str(int((keep & ~near).sum()))
    k1 = [[float(v) for v in r[:4]] + [int(r[4])] for r in _rows(lines, "K1")]
    exp = [[float(h["surface"][0]), float(h["surface"][1]), float(h["surface"][2]), float(h["width"]), 1] for h in hyps[keep & ~near]]
    assert k1 == exp and _rows(lines, "K3") == _rows(lines, "K1")
    assert _rows(lines, "G3") == _rows(lines, "G1")
    assert len(_rows(lines, "G1")) == int(_rows(lines, "CHAIN1")[0][1])
    assert "SAME 1" in lines and "STAGE 1 1 1" in lines


@pytest.mark.gpu
def test_adapter_stream_equals_localize_handles_per_capture(tmp_path, svm_model):
    """Localization(4, true, 0): Begin / stageNextCloud / End over three captures (the second outgrows the first's voxel
    bitmap) return what localizeHandles returns, capture by capture; stageNextCloud no longer refuses."""
    exe = _build(tmp_path)
    caps, ws, cams = _captures()
    paths = []
    (ctx,) = _contexts(cams, svm_model, n=1)
    for k, (xyz, size_left) in enumerate(caps):
        vox, vcam = _preprocess_numpy(xyz, size_left, ws)
        idx = np.sort(np.random.default_rng(10 + k).permutation(len(vox))[:300]).astype(np.int32)
        paths.append(str(tmp_path / f"raw{k}.bin"))
        _dump_raw(paths[-1], xyz, size_left, idx, ws, cams)
        if k == 1:  # the whole scene: the filter bites
            ctx.set_cloud(vox, vcam)
            hyps = ctx.find_hands(idx)
            keep = ctx.classify().astype(bool)
            near = _near(hyps, ws)
            _assert_bites(dict(near=int(near.sum()), kept_near=int((keep & near).sum()), survivors=int((keep & ~near).sum())))
    out = subprocess.run([exe, "stream", SVM] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    st = _rows(out.stdout.splitlines(), "STREAM")
    assert len(st) == 3 and all(r[0] == str(k) and r[1] == "1" and r[4] == "1" for k, r in enumerate(st)), st
    assert sum(int(r[2]) for r in st) > 0
    lines = [l for l in out.stdout.splitlines() if "close to workspace boundaries" in l]
    assert len(lines) >= 3  # (every chain of a filtering object says so)
