"""Camera origins per cloud of a batch (agh_set_cloud_cam_origins): a context that holds a table {A, B, C} for a batch of
three clouds must give, cloud by cloud, exactly what a context CREATED with that cloud's origins gives on the same batch --
frames, normals, hypotheses, occupancy images, training images, SVM sums -- and what the oracle gives for that cloud alone
under those origins.  Origins B lie on the opposite side of the scene from A, so every origin site of the kernels shows: the
sign of the Taubin normals (K1c), the camera-side test of the orientations and source_to_center of the images (K2).
Everything is compared with np.array_equal: the table only changes WHERE the six doubles come from."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HYP_NAMES = ("sample", "orientation", "cam_source", "n_in_box", "half_antipodal", "full_antipodal", "svm_keep", "valid",
             "finger_index", "depth_index", "axis", "approach", "binormal", "bottom", "surface", "width")  # all but epoch
FRAME_NAMES = ("sample", "normal", "axis", "binormal", "params", "eigenvalue", "n_nb", "majority_cam", "max_index", "valid")
ORACLE_FIELDS = ("orientation", "cam_source", "n_in_box", "half_antipodal", "full_antipodal", "finger_index", "depth_index",
                 "axis", "approach", "binormal", "bottom", "surface", "width", "valid")


def _origins(sc_origins, centre):
    """A: the scene's own rig.  B: A mirrored through the scene's centre (the far side: every normal flips).  C: the two
    cameras swapped and moved sideways and up."""
    a = np.asarray(sc_origins, np.float64)
    b = 2.0 * np.asarray(centre, np.float64)[None, :] - a
    c = a[::-1] + np.array([0.10, 0.45, 0.30])
    return np.stack([a, b, c])


@pytest.fixture(scope="module")
def batch():
    """Three tiny_scene-sized clouds (12 000 points, 40 - 64 samples each), the origin pairs A, B, C and the oracle's lists,
    cloud k alone under origins k.  Asserts first, on the CPU, that the origins matter: cloud 1 under A against under B."""
    from agile_grasp_amd import synthetic
    from oracle import oracle_py as O

    scs = [synthetic.config("tiny"), synthetic.make_scene(12_000, 40, seed=33, two_view=True, n_objects=3, name="tiny33"),
           synthetic.make_scene(12_000, 48, seed=34, two_view=True, n_objects=3, name="tiny34")]
    tab = _origins(scs[0].cam_origins, np.concatenate([s.xyz for s in scs]).astype(np.float64).mean(0))
    refs = [O.find_hands(O.default_params(tab[k]), s.xyz, s.cam, s.samples, want_images=True) for k, s in enumerate(scs)]
    under_a = O.find_hands(O.default_params(tab[0]), scs[1].xyz, scs[1].cam, scs[1].samples)
    ha, hb = under_a["hyps"], refs[1]["hyps"]
    fa, fb = under_a["frames"], refs[1]["frames"]
    both = (fa["valid"] != 0) & (fb["valid"] != 0)
    assert both.sum() > 20 and not np.array_equal(fa["normal"][both], fb["normal"][both])  # normals flipped
    assert len(ha) != len(hb) or any(not np.array_equal(ha[f], hb[f]) for f in ORACLE_FIELDS)
    off = np.concatenate([[0], np.cumsum([s.n for s in scs])]).astype(np.int64)
    samples = np.concatenate([s.samples + off[k] for k, s in enumerate(scs)]).astype(np.int32)
    s_off = np.concatenate([[0], np.cumsum([s.samples.size for s in scs])])
    return dict(scs=scs, tab=tab, refs=refs, off=off, samples=samples, s_off=s_off)


def _bind(ctx, b):
    off = ctx.set_cloud_batch([s.xyz for s in b["scs"]], [s.cam for s in b["scs"]])
    assert np.array_equal(off, b["off"])


def _search(ctx, samples, svm_model, anti=True, train=True):
    """One search and everything the getters give for it."""
    if train:
        ctx.set_training_images(True)
    ctx.load_svm(*svm_model)
    hyps = ctx.find_hands(samples, calculates_antipodal=anti)
    out = dict(hyps=hyps, frames=ctx.frames(), images=ctx.images())
    if anti:
        out["normals"] = ctx.normals()
    if train:
        out["train"] = ctx.training_images()
    _, out["sums"] = ctx.hog()
    out["keep"] = ctx.classify()
    return out


def _span_equal(got, ref, s_lo, s_hi, p_lo=None, p_hi=None, what=""):
    """The records of the samples [s_lo, s_hi) of two searches of the same sample list, and the normals of the points
    [p_lo, p_hi)."""
    mg = (got["hyps"]["sample"] >= s_lo) & (got["hyps"]["sample"] < s_hi)
    mr = (ref["hyps"]["sample"] >= s_lo) & (ref["hyps"]["sample"] < s_hi)
    assert mg.sum() == mr.sum() > 0, what
    for f in HYP_NAMES:
        assert np.array_equal(got["hyps"][f][mg], ref["hyps"][f][mr]), (what, f)
    for f in FRAME_NAMES:
        assert np.array_equal(got["frames"][f][s_lo:s_hi], ref["frames"][f][s_lo:s_hi]), (what, f)
    assert np.array_equal(got["images"][mg], ref["images"][mr]), what
    if "train" in got:
        assert np.array_equal(got["train"][mg], ref["train"][mr]), what
    assert np.array_equal(got["sums"][mg], ref["sums"][mr]), what
    assert np.array_equal(got["keep"][mg], ref["keep"][mr]), what
    if p_lo is not None:
        assert np.array_equal(got["normals"][p_lo:p_hi], ref["normals"][p_lo:p_hi]), what
        assert np.abs(got["normals"][p_lo:p_hi]).sum() > 0
    return int(mg.sum())


# ---- 1. the table run against per-origin contexts on the same batch ------------------------------------------------
@pytest.mark.parametrize("mode", ["det", "rand50"])
def test_table_equals_contexts_created_with_each_origin_pair(batch, svm_model, mode):
    from agile_grasp_amd import binding

    kw = dict(normals_mode=binding.NORMALS_RAND50, rand_seed=3) if mode == "rand50" else {}
    b = batch
    T = binding.Context(b["tab"][0], **kw)
    _bind(T, b)
    T.set_cloud_cam_origins(b["tab"])
    got = _search(T, b["samples"], svm_model)
    assert got["hyps"]["half_antipodal"].sum() > 0 and got["keep"].sum() > 0
    spans = []
    for k in range(3):
        R = binding.Context(b["tab"][k], **kw)
        _bind(R, b)
        ref = _search(R, b["samples"], svm_model)
        spans.append(_span_equal(got, ref, b["s_off"][k], b["s_off"][k + 1], b["off"][k], b["off"][k + 1], f"cloud {k}"))
        if k == 0:  # ... and the origins show: cloud 1 under A (this context) is not cloud 1 under B (the table's row)
            m = (ref["hyps"]["sample"] >= b["s_off"][1]) & (ref["hyps"]["sample"] < b["s_off"][2])
            g = (got["hyps"]["sample"] >= b["s_off"][1]) & (got["hyps"]["sample"] < b["s_off"][2])
            assert m.sum() != g.sum() or not np.array_equal(ref["hyps"]["approach"][m], got["hyps"]["approach"][g])
            assert not np.array_equal(ref["normals"][b["off"][1]:b["off"][2]], got["normals"][b["off"][1]:b["off"][2]])
    assert sum(spans) == len(got["hyps"])


# ---- 2. against the oracle ------------------------------------------------------------------------------------------
def test_table_against_the_oracle_cloud_by_cloud(batch, svm_model):
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    b = batch
    w, rho = svm_model
    T = binding.Context(b["tab"][2])  # (the context's own origins are none of the first two rows)
    _bind(T, b)
    T.set_cloud_cam_origins(b["tab"])
    hyps = T.find_hands(b["samples"])
    T.load_svm(w, rho)
    keep = T.classify()
    frames, images = T.frames(), T.images()
    pos = 0
    for k, ref in enumerate(b["refs"]):
        n = len(ref["hyps"])
        part = hyps[pos:pos + n]
        assert np.array_equal(part["sample"], ref["hyps"]["sample"] + b["s_off"][k]), k
        for f in ORACLE_FIELDS:
            assert np.array_equal(part[f], ref["hyps"][f]), (k, f)
        assert np.array_equal(images[pos:pos + n], ref["images"]), k
        okeep, _ = O.classify(ref["images"], w, rho)
        assert np.array_equal(keep[pos:pos + n], okeep), k
        fr = frames[b["s_off"][k]:b["s_off"][k + 1]]
        for f in ("normal", "axis", "binormal", "params", "n_nb", "max_index", "majority_cam", "valid"):
            assert np.array_equal(fr[f], ref["frames"][f]), (k, f)
        pos += n
    assert pos == len(hyps) > 100


# ---- 3. the larger capacity classes -----------------------------------------------------------------------------------
def test_table_reaches_the_larger_capacity_classes_and_survives_the_retry(tiny_scene, svm_model):
    """Cloud 1 holds samples with 1153, 4097 and 6145 Taubin neighbours (tests/capacity_clouds.py): the smallest of the 4096
    class, of the 6144 class and of the pooled class beyond -- k_taubin_frame<4096>, <6144> and k_taubin_frame_huge -- under
    origins that are not the context's.  A fresh context meets them with the larger classes off: the AGH_ERR_RETRY repeats
    inside the call must search with the table too."""
    from agile_grasp_amd import binding
    from tests import capacity_clouds as cc

    targets = (1153, 4097, 6145)
    xyz, cam, s = cc.ball_cloud(targets, 0.03, seed=1, filler=500)
    sc = tiny_scene
    site = xyz[s].astype(np.float64).mean(0)
    blob_cams = 2.0 * site[None, :] - cc.cams()  # behind the patches, which face synthetic.camera_origins()
    tab = np.stack([np.asarray(sc.cam_origins, np.float64), blob_cams])
    samples = np.concatenate([sc.samples[:32], s + sc.n]).astype(np.int32)

    def run(origins, table):
        ctx = binding.Context(origins)
        ctx.set_cloud_batch([sc.xyz, xyz], [sc.cam, cam])
        if table is not None:
            ctx.set_cloud_cam_origins(table)
        out = _search(ctx, samples, svm_model)
        nt, _ = ctx.neighbor_counts()
        assert nt[32:].tolist() == list(targets)
        return out

    got = run(tab[0], tab)
    shared = run(tab[0], None)
    _span_equal(got, shared, 0, 32, 0, sc.n, "the scene")
    n = _span_equal(got, run(tab[1], None), 32, 35, sc.n, sc.n + len(xyz), "the blobs")
    assert n >= 3 and (got["frames"]["valid"][32:] != 0).all()
    # ... and the blobs' frames under the context's own origins are others
    assert not np.array_equal(shared["frames"]["normal"][32:], got["frames"]["normal"][32:])


# ---- 4. agh_localize_batch ----------------------------------------------------------------------------------------------
def test_localize_batch_with_a_table_equals_localize_per_rig(svm_model):
    from agile_grasp_amd import binding, synthetic
    from tests.test_gpu_localize_batch import _same

    caps = [synthetic.make_raw_cloud(n, 200 + k, nan_frac=0.01) for k, n in enumerate((40000, 60000, 50000))]
    centre = np.nanmean(np.concatenate([c.xyz for c in caps]).astype(np.float64), 0)
    tab = _origins(caps[0].cam_origins, centre)
    n_s, seeds = [300, 350, 250], [7, 8, 9]
    T = binding.Context(tab[2])
    T.load_svm(*svm_model)
    T.set_cloud_cam_origins(tab)
    kw = dict(classify=True, min_inliers=2, filters_boundaries=1)
    for _ in range(2):  # (the second call: kept bitmap slots and grid descriptors, the table still set)
        got = T.localize_batch([c.xyz for c in caps], [c.size_left for c in caps], [c.workspace for c in caps], n_samples=n_s,
                               sample_seeds=seeds, **kw)
    refs = []
    for k, c in enumerate(caps):
        R = binding.Context(tab[k])
        R.load_svm(*svm_model)
        refs.append(R.localize(c.xyz, c.size_left, c.workspace, n_samples=n_s[k], sample_seed=seeds[k], **kw))
        _same(got[k], refs[k], f"capture {k}")
    assert all(r["n_hypotheses"] > 0 for r in refs) and sum(len(r["hands"]) for r in refs) > 0
    # the origins show: capture 1 under the context's own origins is another result
    T.set_cloud_cam_origins(None)
    plain = T.localize_batch([c.xyz for c in caps], [c.size_left for c in caps], [c.workspace for c in caps], n_samples=n_s,
                             sample_seeds=seeds, **kw)
    assert plain[1]["n_hypotheses"] != got[1]["n_hypotheses"] or len(plain[1]["hands"]) != len(got[1]["hands"]) or \
        not np.array_equal(plain[1]["hands"]["approach"], got[1]["hands"]["approach"])
    # a table of the wrong size is refused before anything runs, by agh_localize too; one row is agh_localize's table
    T.set_cloud_cam_origins(tab[:2])
    with pytest.raises(binding.AghError) as e:
        T.localize_batch([c.xyz for c in caps], [c.size_left for c in caps], [c.workspace for c in caps], n_samples=n_s,
                         sample_seeds=seeds, **kw)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "2 rows" in str(e.value) and "3 clouds" in str(e.value)
    with pytest.raises(binding.AghError) as e:
        T.localize(caps[1].xyz, caps[1].size_left, caps[1].workspace, n_samples=n_s[1], sample_seed=seeds[1], **kw)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT
    T.set_cloud_cam_origins(tab[1:2])
    _same(T.localize(caps[1].xyz, caps[1].size_left, caps[1].workspace, n_samples=n_s[1], sample_seed=seeds[1], **kw), refs[1])


# ---- 5. sharded -----------------------------------------------------------------------------------------------------------
def test_sharded_search_with_the_table_on_both_ranks(batch):
    from agile_grasp_amd import binding
    from tests.test_gpu_sharding import _run_ranks

    b = batch
    one = binding.Context(b["tab"][0])
    _bind(one, b)
    one.set_cloud_cam_origins(b["tab"])
    ref = one.find_hands(b["samples"], calculates_antipodal=True)
    ctxs = [binding.Context(b["tab"][0]) for _ in range(2)]
    for c in ctxs:
        _bind(c, b)
        c.set_cloud_cam_origins(b["tab"])
    binding.comm_init_local(ctxs)  # (the parameter digest covers the tables: equal ones pass)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(b["samples"], calculates_antipodal=True)):
        assert len(hyps) == len(ref) > 100
        for f in HYP_NAMES:
            assert np.array_equal(hyps[f], ref[f]), f
    # a table that does not fit the batch on ONE rank: that rank takes part without searching, every rank returns an error
    ctxs[1].set_cloud_cam_origins(b["tab"][:2])
    codes = [None, None]

    def search(r, c):
        try:
            c.find_hands_sharded(b["samples"])
        except binding.AghError as e:
            codes[r] = e.code
            return str(e)
        return ""

    msgs = _run_ranks(ctxs, search)
    assert codes[1] == binding.AGH_ERR_INVALID_ARGUMENT and "2 rows" in msgs[1] and "3 clouds" in msgs[1]
    assert codes[0] == binding.AGH_ERR_STATE
    ctxs[1].set_cloud_cam_origins(b["tab"])
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(b["samples"], calculates_antipodal=True)):
        for f in HYP_NAMES:
            assert np.array_equal(hyps[f], ref[f]), f
    # contexts that hold different tables cannot form a communicator
    x, y = binding.Context(b["tab"][0]), binding.Context(b["tab"][0])
    x.set_cloud_cam_origins(b["tab"])
    y.set_cloud_cam_origins(b["tab"][::-1].copy())
    with pytest.raises(binding.AghError):
        binding.comm_init_local([x, y])


# ---- 6. neutrality and state ------------------------------------------------------------------------------------------------
def test_neutral_table_one_row_table_and_the_error_paths(batch, tiny_scene, svm_model):
    from agile_grasp_amd import binding

    b = batch
    a = b["tab"][0]
    plain = binding.Context(a)
    _bind(plain, b)
    ref = _search(plain, b["samples"], svm_model)
    T = binding.Context(a)
    _bind(T, b)
    assert T.get_cloud_cam_origins() is None
    T.set_cloud_cam_origins(np.stack([a, a, a]))
    got = _search(T, b["samples"], svm_model)
    # every row the context's own origins: byte-identical records (the epoch is the call's stamp)
    g, r = got["hyps"].copy(), ref["hyps"].copy()
    g["epoch"] = r["epoch"] = 0
    assert g.tobytes() == r.tobytes() and got["frames"].tobytes() == ref["frames"].tobytes()
    _span_equal(got, ref, 0, len(b["samples"]), 0, int(b["off"][-1]), "neutral table")
    # the getter returns what was set; the table is sticky over a new batch
    assert np.array_equal(T.get_cloud_cam_origins(), np.stack([a, a, a]))
    T.set_cloud_cam_origins(b["tab"])
    _bind(T, b)
    assert np.array_equal(T.get_cloud_cam_origins(), b["tab"])
    # a one-row table on a single cloud = a context created with that row
    sc = tiny_scene
    one = binding.Context(a)
    one.set_cloud(sc.xyz, sc.cam)
    one.set_cloud_cam_origins(b["tab"][1:2])
    made = binding.Context(b["tab"][1])
    made.set_cloud(sc.xyz, sc.cam)
    _span_equal(_search(one, sc.samples, svm_model), _search(made, sc.samples, svm_model), 0, sc.samples.size, 0, sc.n, "one row")
    # a wrong row count: AGH_ERR_INVALID_ARGUMENT naming both counts, for the host and the device entry point; cleared: fine
    one.set_cloud_cam_origins(b["tab"])
    with pytest.raises(binding.AghError) as e:
        one.find_hands(sc.samples)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "3 rows" in str(e.value) and "1 clouds" in str(e.value)
    import torch

    s_t = torch.from_numpy(np.ascontiguousarray(sc.samples)).cuda()
    out_t = torch.zeros(8 * sc.samples.size * 160, dtype=torch.uint8, device="cuda")
    n_t = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(binding.AghError) as e:
        one.find_hands_torch(s_t, out_t, n_t)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT
    one.synchronize()
    assert int(n_t.item()) == -7  # nothing ran
    one.set_cloud_cam_origins(None)
    assert one.get_cloud_cam_origins() is None
    again = one.find_hands(sc.samples)
    made_a = binding.Context(a)
    made_a.set_cloud(sc.xyz, sc.cam)
    exp = made_a.find_hands(sc.samples)
    for f in HYP_NAMES:
        assert np.array_equal(again[f], exp[f]), f
    # refused values: NaN / infinity, no rows, too many rows -- and the table held before stays
    one.set_cloud_cam_origins(b["tab"][1:2])
    for bad in (np.nan, np.inf):
        t = b["tab"].copy()
        t[2, 1, 0] = bad
        with pytest.raises(binding.AghError) as e:
            one.set_cloud_cam_origins(t)
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT
    for rows in (0, 65):
        assert one.lib.agh_set_cloud_cam_origins(one._h, np.zeros((65, 2, 3)).ctypes.data_as(C.POINTER(C.c_double)),
                                                 C.c_int32(rows)) == binding.AGH_ERR_INVALID_ARGUMENT
    assert np.array_equal(one.get_cloud_cam_origins(), b["tab"][1:2])
    small = np.zeros((1, 2, 3))
    one.set_cloud_cam_origins(b["tab"])
    assert one.lib.agh_get_cloud_cam_origins(one._h, small.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(1)) == binding.AGH_ERR_CAPACITY


def test_setter_is_refused_while_a_localize_chain_is_in_flight(svm_model):
    from agile_grasp_amd import binding, synthetic
    from tests.test_gpu_localize_batch import _same

    rc = synthetic.make_raw_cloud(50000, 77)
    tab = _origins(rc.cam_origins, np.nanmean(rc.xyz.astype(np.float64), 0))
    kw = dict(n_samples=300, sample_seed=5, classify=True, min_inliers=2)
    ref_ctx = binding.Context(tab[1])
    ref_ctx.load_svm(*svm_model)
    ref = ref_ctx.localize(rc.xyz, rc.size_left, rc.workspace, **kw)
    ctx = binding.Context(tab[0])
    ctx.load_svm(*svm_model)
    ctx.set_cloud_cam_origins(tab[1:2])
    ctx.localize_begin(rc.xyz, rc.size_left, rc.workspace, **kw)
    with pytest.raises(binding.AghError) as e:
        ctx.set_cloud_cam_origins(tab[2:3])
    assert e.value.code == binding.AGH_ERR_STATE
    with pytest.raises(binding.AghError) as e:
        ctx.set_cloud_cam_origins(None)
    assert e.value.code == binding.AGH_ERR_STATE
    assert np.array_equal(ctx.get_cloud_cam_origins(), tab[1:2])  # the getter is host-side and stays allowed
    _same(ctx.localize_end(), ref, "the chain in flight")
    ctx.set_cloud_cam_origins(tab[2:3])  # ... and after the end the setter works again
    assert np.array_equal(ctx.get_cloud_cam_origins(), tab[2:3])


# ---- 7. the C++ adapter -------------------------------------------------------------------------------------------------
def test_adapter_batch_with_transforms_per_capture(tmp_path):
    """Localization::localizeHandlesBatch(..., cams_left, cams_right) against localizeHandles on Localization objects set up
    with each capture's transforms (tests/cpp/cloud_cam_origins_test.cpp); the plain overload afterwards finds no table."""
    from agile_grasp_amd import build, synthetic
    from tests.test_cpp_adapter import ROOT, _dump_raw
    from tests.test_gpu_boundary_chain import SVM

    build.build()
    exe = str(tmp_path / "cloud_cam_origins_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cloud_cam_origins_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    caps = [synthetic.make_raw_cloud(n, 300 + k) for k, n in enumerate((50000, 60000, 40000))]
    tab = _origins(caps[0].cam_origins, np.nanmean(np.concatenate([c.xyz for c in caps]).astype(np.float64), 0))
    paths = []
    for k, rc in enumerate(caps):
        idx = np.sort(np.random.default_rng(k).permutation(4000)[:300]).astype(np.int32)
        paths.append(str(tmp_path / f"raw{k}.bin"))
        _dump_raw(paths[-1], rc.xyz, rc.size_left, idx, rc.workspace, tab[k])
    out = subprocess.run([exe, SVM] + paths, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines() if l.startswith(("MIXED ", "SHARED ", "SHORT "))]
    mixed = [r for r in rows if r[0] == "MIXED"]
    shared = [r for r in rows if r[0] == "SHARED"]
    assert len(mixed) == 6 and all(r[4] == "1" for r in mixed), rows
    assert sum(int(r[2]) for r in mixed) > 0  # kept hands
    assert [r[2] for r in shared] == ["1", "0", "0"], rows  # capture 0's rig is the object's own; the others' is not
    assert [r for r in rows if r[0] == "SHORT"] == [["SHORT", "3", "0"]]
    assert "one left and one right camera transform per cloud" in out.stdout
