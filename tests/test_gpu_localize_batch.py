"""agh_localize_batch: the fused chain over a batch of captures in one call.  Every capture's results are held against
agh_localize on the same capture and samples, on a second context: every hand field but the epoch, handles, inlier lists,
samples, n_voxels and n_hypotheses."""
import numpy as np
import pytest

from agile_grasp_amd import synthetic
from tests.test_gpu_boundary_chain import _contexts, _near, _scene

HYP_NAMES = tuple(n for n in __import__("agile_grasp_amd.binding", fromlist=["HYP_DTYPE"]).HYP_DTYPE.names if n != "epoch")


def _same(got, ref, what=""):
    assert got["n_voxels"] == ref["n_voxels"], what
    assert got["n_hypotheses"] == ref["n_hypotheses"], what
    assert np.array_equal(got["samples"], ref["samples"]), what
    assert len(got["hands"]) == len(ref["hands"]), what
    for f in HYP_NAMES:
        assert np.array_equal(got["hands"][f], ref["hands"][f]), (what, f)
    assert len(got["handles"]) == len(ref["handles"]), what
    for f in got["handles"].dtype.names:
        assert np.array_equal(got["handles"][f], ref["handles"][f]), (what, f)
    assert np.array_equal(got["inlier_idx"], ref["inlier_idx"]), what


def _caps(n, seed0, sizes=(60000, 90000, 40000, 120000, 70000, 50000, 100000, 80000)):
    """n raw captures of different sizes, one with no non-finite point (it is passed as dense), the others with drop-outs."""
    out = []
    for k in range(n):
        rc = synthetic.make_raw_cloud(sizes[k % len(sizes)], seed0 + k, nan_frac=0.0 if k == 1 else 0.01)
        out.append(rc)
    return out


def _check(batch_ctx, ref_ctx, caps, ws_list, samples=None, n_samples=None, seeds=None, dense=None, **kw):
    C = len(caps)
    n_samples = n_samples if n_samples is not None else [300 + 50 * k for k in range(C)]
    seeds = seeds if seeds is not None else [7 + k for k in range(C)]
    dense = dense if dense is not None else [k == 1 for k in range(C)]
    got = batch_ctx.localize_batch([c.xyz for c in caps], [c.size_left for c in caps], ws_list, samples=samples,
                                   n_samples=n_samples, sample_seeds=seeds, dense=dense, **kw)
    assert len(got) == C
    for k, c in enumerate(caps):
        s = samples[k] if samples is not None else None
        ref = ref_ctx.localize(c.xyz, c.size_left, ws_list[k], samples=s, n_samples=n_samples[k], sample_seed=seeds[k],
                               dense=dense[k], **kw)
        _same(got[k], ref, f"capture {k}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("classify", [0, 1])
@pytest.mark.parametrize("filters", [0, 1])
def test_batch_equals_localize_per_capture(svm_model, classify, filters):
    caps = _caps(3, 40)
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    ws = [c.workspace for c in caps]
    got = _check(one, ref, caps, ws, classify=bool(classify), min_inliers=2, filters_boundaries=filters)
    assert all(g["n_hypotheses"] > 0 for g in got)
    if not classify:
        assert sum(len(g["handles"]) for g in got) > 0
    # the same context again: a batch of another size, other captures (kept bitmap and grid descriptors re-used)
    caps8 = _caps(8, 60)
    _check(one, ref, caps8, [c.workspace for c in caps8], classify=bool(classify), min_inliers=2, filters_boundaries=filters)
    caps1 = _caps(1, 90)
    _check(one, ref, caps1, [caps1[0].workspace], classify=bool(classify), min_inliers=2, filters_boundaries=filters)


@pytest.mark.gpu
def test_boundary_filter_bites_per_capture_workspace(svm_model):
    xyz, size_left, ws, cams = _scene()
    other = synthetic.make_raw_cloud(80000, 5)
    one, ref = _contexts(cams, svm_model)
    caps = [synthetic.RawCloud(xyz, size_left, ws, cams), other]
    got = _check(one, ref, caps, [ws, other.workspace], n_samples=[600, 300], classify=True, min_inliers=2,
                 filters_boundaries=1)
    plain = one.localize_batch([xyz, other.xyz], [size_left, other.size_left], [ws, other.workspace], n_samples=[600, 300],
                               sample_seeds=[7, 8], classify=True, min_inliers=2, filters_boundaries=0)
    assert len(plain[0]["hands"]) > len(got[0]["hands"])  # the filter bit
    assert not _near(got[0]["hands"], ws).any()


@pytest.mark.gpu
def test_explicit_samples_edge_cases_and_device_variant(svm_model):
    import torch

    caps = _caps(4, 120)
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    ws = [c.workspace for c in caps]
    ws[2] = np.array([10.0, 11.0, 10.0, 11.0, 10.0, 11.0])  # keeps no point
    vox = [ref.localize(c.xyz, c.size_left, w, n_samples=0, dense=(k == 1))["n_voxels"] for k, (c, w) in enumerate(zip(caps, ws))]
    assert vox[2] == 0
    rng = np.random.default_rng(3)
    samples = [np.sort(rng.permutation(v)[:min(v, 400)]).astype(np.int32) for v in vox]
    samples[3] = np.zeros(0, np.int32)  # n_samples = 0
    _check(one, ref, caps, ws, samples=samples, n_samples=[len(s) for s in samples], classify=True, min_inliers=2)
    # drawn on the device, the captures read in place as torch tensors with 12- and 32-byte rows
    dev = []
    for k, c in enumerate(caps):
        if k % 2:
            t = torch.zeros((c.xyz.shape[0], 8), dtype=torch.float32)
            t[:, :3] = torch.from_numpy(c.xyz)
            dev.append(t.cuda())
        else:
            dev.append(torch.from_numpy(c.xyz).cuda())
    n_s, seeds, dense = [250, 300, 200, 350], [1, 2, 3, 4], [False, True, False, False]
    got = one.localize_batch(dev, [c.size_left for c in caps], ws, n_samples=n_s, sample_seeds=seeds, dense=dense,
                             classify=True, min_inliers=2)
    for k, c in enumerate(caps):
        r = ref.localize(c.xyz, c.size_left, ws[k], n_samples=n_s[k], sample_seed=seeds[k], dense=dense[k], classify=True,
                         min_inliers=2)
        _same(got[k], r, f"device capture {k}")


@pytest.mark.gpu
def test_fresh_context_first_batch_repeats_the_capacity_class(svm_model):
    """A fresh context whose first batch holds a C2-style capture (700k raw points): about a tenth of its samples exceed the
    first Taubin capacity class, so the search's AGH_ERR_RETRY is repeated inside the call."""
    big = synthetic.make_raw_cloud(700000, 2)
    small = synthetic.make_raw_cloud(50000, 3)
    one, ref = _contexts(big.cam_origins, svm_model)
    _check(one, ref, [small, big], [small.workspace, big.workspace], n_samples=[300, 2000], dense=[False, False],
           classify=True, min_inliers=3)
    # the retry happened: the batch's own search has frames whose Taubin neighbourhoods exceed the first class (1152 points)
    nt, _ = one.neighbor_counts()
    assert len(nt) == 2300 and int((nt > 1152).sum()) > 20


@pytest.mark.gpu
def test_errors_leave_the_context_usable(svm_model):
    from agile_grasp_amd import binding

    caps = _caps(3, 200)
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    xyz = [c.xyz for c in caps]
    sl = [c.size_left for c in caps]
    ws = [c.workspace for c in caps]

    # shared fields must be equal (the binding writes them alike: the records are built by hand here), 1 <= n_captures <= 64
    import ctypes as C

    lps = (binding.AghLocalizeParams * 2)()
    for k in range(2):
        lps[k].size_left, lps[k].classify, lps[k].cell_size, lps[k].min_inliers, lps[k].min_length = sl[k], 0, 0.003, 2, 0.005
        for q in range(6):
            lps[k].workspace[q] = ws[k][q]
        lps[k].n_samples = 10
    ptrs = (C.c_void_p * 2)(xyz[0].ctypes.data, xyz[1].ctypes.data)
    strides = (C.c_int64 * 2)(12, 12)
    ns = (C.c_int64 * 2)(xyz[0].shape[0], xyz[1].shape[0])
    res = (binding.AghLocalizeBatchResult * 2)()

    def call(nc):
        return one.lib.agh_localize_batch(one._h, ptrs, strides, ns, lps, C.c_int32(nc), None, C.c_int64(0), None, C.c_int64(0),
                                          None, C.c_int64(0), None, res)

    for field, value in (("cell_size", 0.004), ("min_inliers", 3), ("min_length", 0.01), ("classify", 1),
                         ("filters_boundaries", 1)):
        old = getattr(lps[1], field)
        setattr(lps[1], field, value)
        assert call(2) == binding.AGH_ERR_INVALID_ARGUMENT, field
        setattr(lps[1], field, old)
    assert call(0) == binding.AGH_ERR_INVALID_ARGUMENT
    assert call(65) == binding.AGH_ERR_INVALID_ARGUMENT
    _check(one, ref, caps[:2], ws[:2], n_samples=[200, 200], dense=[False, False], classify=True, min_inliers=2)
    # too-small outputs: AGH_ERR_CAPACITY with every capture's counts filled
    good = one.localize_batch(xyz, sl, ws, n_samples=300, classify=True, min_inliers=2)
    assert sum(len(g["handles"]) for g in good) > 0
    with pytest.raises(binding.AghError) as e:
        one.localize_batch(xyz, sl, ws, n_samples=300, classify=True, min_inliers=2, caps=(0, 0, 0))
    assert e.value.code == binding.AGH_ERR_CAPACITY
    counts = one.last_batch_counts
    assert [c["n_handles"] for c in counts] == [len(g["handles"]) for g in good]
    assert [c["n_hands"] for c in counts] == [len(g["hands"]) for g in good]
    assert [c["n_voxels"] for c in counts] == [g["n_voxels"] for g in good]
    _check(one, ref, caps, ws, n_samples=[300] * 3, dense=[False] * 3, classify=True, min_inliers=2)
    # an out-of-range sample: the error names the capture
    bad = [np.array([0, 1], np.int32), np.array([0, 10 ** 8], np.int32), np.array([2], np.int32)]
    with pytest.raises(binding.AghError) as e:
        one.localize_batch(xyz, sl, ws, samples=bad, classify=True, min_inliers=2)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "capture 1" in str(e.value)
    _check(one, ref, caps, ws, n_samples=[300] * 3, dense=[False] * 3, classify=True, min_inliers=2)
    # no SVM
    plain = binding.Context(caps[0].cam_origins)
    with pytest.raises(binding.AghError) as e:
        plain.localize_batch(xyz, sl, ws, n_samples=100, classify=True)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    # a chain in flight: refused, the chain untouched
    one.localize_begin(xyz[0], sl[0], ws[0], n_samples=300, sample_seed=9, classify=True, min_inliers=2)
    with pytest.raises(binding.AghError) as e:
        one.localize_batch(xyz, sl, ws, n_samples=300, classify=True, min_inliers=2)
    assert e.value.code == binding.AGH_ERR_STATE
    staged = one.localize_end()
    _same(staged, ref.localize(xyz[0], sl[0], ws[0], n_samples=300, sample_seed=9, classify=True, min_inliers=2), "chain")
    # after every error the context still gives agh_localize's results, and the batch's
    _check(one, ref, caps, ws, n_samples=[300] * 3, dense=[False] * 3, classify=True, min_inliers=2)


@pytest.mark.gpu
def test_batch_capture_against_the_stage_wise_calls(svm_model):
    """One capture of a batch against the stage-wise calls on the same samples (preprocess -> find_hands -> classify ->
    find_handles, each held against the oracle by tests/test_preprocess.py and tests/test_handles.py)."""
    from tests.test_cpp_adapter import _preprocess_numpy, _raw_cloud

    xyz, size_left, ws, cams = _raw_cloud()
    other = synthetic.make_raw_cloud(60000, 8)
    one, chain = _contexts(cams, svm_model)
    vox, _ = _preprocess_numpy(xyz, size_left, ws)
    samples = np.sort(np.random.default_rng(1).permutation(len(vox))[:300]).astype(np.int32)
    got = one.localize_batch([other.xyz, xyz], [other.size_left, size_left], [other.workspace, ws],
                             samples=[None, samples], n_samples=[200, 300], classify=True, min_inliers=2)
    assert got[1]["n_voxels"] == len(vox)
    assert chain.preprocess(xyz, size_left, ws) == len(vox)
    hyps = chain.find_hands(samples)
    keep = chain.classify().astype(bool)
    h = hyps[keep].copy()
    h["svm_keep"] = 1
    hd, idx = chain.find_handles(h, 2, 0.005)
    assert got[1]["n_hypotheses"] == len(hyps) and len(got[1]["hands"]) == len(h)
    for f in HYP_NAMES:
        assert np.array_equal(got[1]["hands"][f], h[f]), f
    assert len(got[1]["handles"]) == len(hd) > 0 and np.array_equal(got[1]["inlier_idx"], idx)
    for f in hd.dtype.names:
        assert np.array_equal(got[1]["handles"][f], hd[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("filters", [0, 1])
def test_adapter_batch_equals_localize_handles_per_capture(tmp_path, svm_model, filters):
    """Localization::localizeHandlesBatch against localizeHandles per capture (tests/cpp/localize_batch_test.cpp), with a
    workspace per capture and with the object's own workspace; then localizeHandlesBatchBegin / stageNextBatch /
    localizeHandlesBatchEnd on the same object against the blocking call's results (the STREAM rows: Begin, a refused second
    Begin, the reversed batch staged, End, the staged batch adopted and collected, a plain localizeHandles afterwards)."""
    import os
    import subprocess

    from tests.test_cpp_adapter import ROOT, _dump_raw
    from tests.test_gpu_boundary_chain import SVM
    from agile_grasp_amd import build

    build.build()
    exe = str(tmp_path / "localize_batch_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "localize_batch_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    xyz, size_left, ws, cams = _scene()
    paths = []
    for k, rc in enumerate([synthetic.RawCloud(xyz, size_left, ws, cams), synthetic.make_raw_cloud(60000, 31),
                            synthetic.make_raw_cloud(90000, 32)]):
        idx = np.sort(np.random.default_rng(k).permutation(5000)[:300]).astype(np.int32)
        paths.append(str(tmp_path / f"raw{k}.bin"))
        _dump_raw(paths[-1], rc.xyz, rc.size_left, idx, rc.workspace, cams)
    out = subprocess.run([exe, str(filters), SVM] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines() if l.startswith(("BATCH ", "OWNWS "))]
    assert len(rows) == 6, out.stdout[-2000:]
    assert all(r[4] == "1" for r in rows), rows
    assert sum(int(r[3]) for r in rows if r[0] == "BATCH") > 0  # handles found
    stream = [l.split() for l in out.stdout.splitlines() if l.startswith("STREAM ")]
    assert len(stream) == 6, out.stdout[-2000:]
    assert all(r[2] == "1" for r in stream), stream
