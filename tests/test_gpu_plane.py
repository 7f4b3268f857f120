"""agh_remove_plane on the MI355X against the host restatement (tests/cpp/plane_ref.cpp): candidates, counts, the chosen
model, iterations, refined coefficients, inliers and the kept cloud with its camera ids agree bit for bit; the kept cloud
is searched like any other; Localization::localizeHands(..., uses_clustering = true) and train_pcd run the whole chain."""
import os
import subprocess

import numpy as np
import pytest

from tests import plane_clouds
from tests import plane_ref_lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIBDIR = os.path.join(ROOT, "agile_grasp_amd", "lib")


def _check(ctx, xyz, cam, by_position):
    """remove_plane with its defaults on the context's cloud (xyz, cam as read back) against the restatement (the shared check
    of tests/plane_clouds.py); returns the GPU result."""
    return plane_clouds.check(ctx, xyz, cam, by_position)


def _context(sc):
    from agile_grasp_amd import binding

    ctx = binding.Context(sc.cam_origins)
    ctx.set_cloud(sc.xyz, sc.cam)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "small", "C2", "C2u", "C4", "boxu"])
@pytest.mark.parametrize("by_position", [True, False])
def test_scene_bit_exact(name, by_position):
    from agile_grasp_amd import synthetic

    sc = synthetic.config(name)
    ctx = _context(sc)
    xyz, cam = ctx.cloud()
    res = _check(ctx, xyz, cam, by_position)
    assert res["found"] and res["n_inliers"] > 0.2 * sc.n


@pytest.mark.gpu
def test_kept_cloud_is_searched_like_a_fresh_one(small_scene):
    from agile_grasp_amd import binding

    ctx = _context(small_scene)
    res = ctx.remove_plane()
    kx, kc = ctx.cloud()
    samples = np.sort(np.random.default_rng(1).permutation(res["n_remaining"])[:150]).astype(np.int32)
    hyps = ctx.find_hands(samples)
    fresh = binding.Context(small_scene.cam_origins)
    fresh.set_cloud(kx, kc)
    ref = fresh.find_hands(samples)
    assert len(hyps) == len(ref) > 0
    for f in hyps.dtype.names:
        if f != "epoch":  # (the stamp of the call that made the record)
            assert np.array_equal(hyps[f], ref[f]), f
    # a second removal reads the first one's output (the other buffer set)
    xyz, cam = ctx.cloud()
    _check(ctx, xyz, cam, True)


@pytest.mark.gpu
def test_preprocessed_cloud():
    from agile_grasp_amd import binding, synthetic

    raw = synthetic.make_raw_cloud(120_000, seed=5)
    ctx = binding.Context(raw.cam_origins)
    ctx.preprocess(raw.xyz, raw.size_left, raw.workspace)
    xyz, cam = ctx.cloud()
    _check(ctx, xyz, cam, True)


@pytest.mark.gpu
def test_degenerate_clouds():
    from agile_grasp_amd import binding, synthetic

    sc = synthetic.config("tiny")
    ctx = binding.Context(sc.cam_origins)
    rng = np.random.default_rng(3)
    base = rng.uniform(-0.1, 0.1, (6, 3)).astype(np.float32)
    dup = np.ascontiguousarray(base[rng.integers(0, 6, 200)])
    cam = (np.arange(200) % 2).astype(np.int32)
    ctx.set_cloud(dup, cam)
    _check(ctx, dup, cam, True)
    assert np.isnan(ctx.plane_candidates()["planes"]).any()
    # fewer than 3 points, an all-collinear line: no model, the cloud stays
    for pts in (np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], np.float32),
                np.ascontiguousarray((np.arange(60, dtype=np.float32)[:, None] * np.float32(0.01)).repeat(3, 1))):
        c = np.zeros(len(pts), np.int32)
        ctx.set_cloud(pts, c)
        res = _check(ctx, pts, c, True)
        assert not res["found"] and ctx.plane_inliers().size == 0
    # a cloud that is only the plane: nothing remains
    g = np.arange(40, dtype=np.float32) * np.float32(0.003)
    u, v = np.meshgrid(g, g, indexing="ij")
    flat = np.ascontiguousarray(np.stack([u.ravel(), v.ravel(), np.full(u.size, 0.25, np.float32)], 1))
    ctx.set_cloud(flat, np.zeros(len(flat), np.int32))
    res = _check(ctx, flat, np.zeros(len(flat), np.int32), True)
    assert res["found"] and res["n_remaining"] == 0 and ctx.cloud()[0].shape[0] == 0


@pytest.mark.gpu
def test_state_errors(tiny_scene):
    from agile_grasp_amd import binding

    ctx = binding.Context(tiny_scene.cam_origins)
    with pytest.raises(binding.AghError) as e:
        ctx.remove_plane()
    assert e.value.code == binding.AGH_ERR_STATE
    ctx.set_cloud_batch([tiny_scene.xyz[:5000], tiny_scene.xyz[5000:]], [tiny_scene.cam[:5000], tiny_scene.cam[5000:]])
    with pytest.raises(binding.AghError) as e:
        ctx.remove_plane()
    assert e.value.code == binding.AGH_ERR_STATE
    from agile_grasp_amd import synthetic

    raw = synthetic.make_raw_cloud(40_000, seed=5)
    ctx.localize_begin(raw.xyz, raw.size_left, raw.workspace, n_samples=50, classify=False)
    with pytest.raises(binding.AghError) as e:
        ctx.remove_plane()
    assert e.value.code == binding.AGH_ERR_STATE
    ctx.localize_end()
    xyz, cam = ctx.cloud()
    _check(ctx, xyz, cam, True)


def _write_pcd(path, xyz):
    n = len(xyz)
    hdr = ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS x y z", "SIZE 4 4 4", "TYPE F F F",
           "COUNT 1 1 1", f"WIDTH {n}", "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0", f"POINTS {n}", "DATA binary"]
    with open(path, "wb") as f:
        f.write(("\n".join(hdr) + "\n").encode())
        f.write(np.ascontiguousarray(xyz, np.float32).tobytes())


def _compile(src, exe):
    from agile_grasp_amd import build

    build.build()
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           src, "-o", exe, "-L" + LIBDIR, "-lagile_grasp_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib"])


@pytest.mark.gpu
def test_localize_hands_with_clustering(tmp_path):
    """localizeHands(l.pcd, r.pcd, true, true): the hands equal ctx.find_hands on the restatement's kept cloud, with the
    reference's camera ids (those of the unsegmented cloud's first M points) and the samples the adapter drew over M."""
    from agile_grasp_amd import binding, synthetic

    exe = str(tmp_path / "plane_adapter_test")
    _compile(os.path.join(ROOT, "tests", "cpp", "plane_adapter_test.cpp"), exe)
    raw = synthetic.make_raw_cloud(150_000, seed=9)
    lp, rp = str(tmp_path / "l.pcd"), str(tmp_path / "r.pcd")
    _write_pcd(lp, raw.xyz[:raw.size_left])
    _write_pcd(rp, raw.xyz[raw.size_left:])
    co = raw.cam_origins
    args = [exe, lp, rp] + [repr(float(v)) for v in raw.workspace] + [repr(float(v)) for v in co.ravel()] + ["300", "7"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "Finding point cloud clusters ... " in lines
    ctx = binding.Context(co, normals_mode=binding.NORMALS_DETERMINISTIC)
    ctx.preprocess(raw.xyz, raw.size_left, raw.workspace)
    vox, vcam = ctx.cloud()
    ref = R.segment(vox)
    assert ref["found"]
    m = ref["mask"]
    M = int((~m).sum())
    assert any(l == f" PointCloud representing the planar component: {int(m.sum())} data points." for l in lines)
    cl = [l.split() for l in lines if l.startswith("P ")]
    assert len(cl) == M
    got = np.array([[float(v) for v in r[1:4]] for r in cl], np.float32)
    assert np.array_equal(got, vox[~m]) and np.array_equal(np.array([int(r[4]) for r in cl]), vcam[:M])
    samples = np.array([int(l.split()[1]) for l in lines if l.startswith("S ")], np.int32)
    assert len(samples) == 300 and samples.max() < M
    ctx.set_cloud(vox[~m], vcam[:M])
    hyps = ctx.find_hands(samples, calculates_antipodal=True)
    hl = [l.split()[1:] for l in lines if l.startswith("H ")]
    res = [l for l in lines if l.startswith("RESULT")][0].split()
    assert int(res[1]) == len(hyps) == len(hl) > 0
    for row, h in zip(hl, hyps):
        assert [float(v) for v in row[:4]] == [float(h["surface"][0]), float(h["surface"][1]), float(h["surface"][2]),
                                               float(h["width"])]
        assert int(row[4]) == h["cam_source"]


@pytest.mark.gpu
def test_train_example_with_clustering(tmp_path):
    from agile_grasp_amd import synthetic
    from oracle import oracle_py as O

    exe = str(tmp_path / "train_pcd")
    _compile(os.path.join(ROOT, "examples", "train_pcd.cpp"), exe)
    d = str(tmp_path) + os.sep
    with open(d + "workspace.txt", "w") as f:
        for k in range(2):
            raw = synthetic.make_raw_cloud(120_000, seed=11 + k)
            _write_pcd(d + f"{k}l_reg.pcd", raw.xyz[:raw.size_left])
            _write_pcd(d + f"{k}r_reg.pcd", raw.xyz[raw.size_left:])
            f.write(" ".join(repr(float(v)) for v in raw.workspace) + " \n")
    model = d + "trained.yaml"
    out = subprocess.run([exe, "2", d, model, "0", "400", "4", "1"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("PointCloud representing the planar component") == 2
    assert "Saved trained SVM as " + model in out.stdout
    kernel, sv, alpha, rho = O.load_svm_model(model)
    assert kernel == 1 and sv.shape[0] == alpha.shape[0] >= 2 and np.isfinite(rho)
