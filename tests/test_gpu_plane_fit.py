"""agh_localize_clustered_fit* and agh_localize_depth_clustered_fit* (include/agh.h): the clustered chain with the support plane
found on the device.  The plane, the counts and every candidate are held against the numpy model of tests/plane_fit_cases.py on
the context's own cloud; the chain against agh_localize_clustered fed the reported plane -- exact equality throughout."""
import numpy as np
import pytest

from tests import cluster_cases as CC
from tests import plane_fit_cases as PF
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same
from tests.test_gpu_localize_clustered import _depth_scene

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
SKIP = -(1 << 31)
CASES = PF.cases()


def _fp(fields):
    from agile_grasp_amd import binding

    return binding.plane_fit_params(**fields)


def _cp(fields):
    from agile_grasp_amd import binding

    return binding.cluster_params(**fields)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _context(c):
    from agile_grasp_amd import binding

    ctx = binding.Context(c["origins"])
    if c["table"] is not None:
        ctx.set_cloud_cam_origins(c["table"][None])
    return ctx


def _check_fit(ctx, m, what=""):
    """agh_get_plane_fit and agh_get_plane_fit_candidates of the last call against the model `m`, bit for bit"""
    fit, cand = ctx.plane_fit(), ctx.plane_fit_candidates()
    print(what, "voxels", fit["n_voxels"], "best", fit["best_candidate"], "inliers", fit["n_inliers"], "refit", fit["n_refit"], "found",
          fit["found"], "refined", fit["refined"], "plane", list(fit["plane"]))
    assert np.array_equal(cand["idx"], m["idx"]), what
    assert np.array_equal(_bits(cand["planes"]), _bits(m["planes"])), what
    assert np.array_equal(cand["counts"], m["counts"]), what
    for f in ("n_voxels", "best_candidate", "n_inliers", "n_refit", "found", "refined"):
        assert fit[f] == m[f], (what, f, fit[f], m[f])
    assert np.array_equal(_bits(fit["plane"]), _bits(m["plane"])), (what, list(fit["plane"]), list(m["plane"]))
    return fit


def _run_case(ctx, c, S=7, seed=11, **kw):
    return ctx.localize_clustered_fit(c["points"], c["size_left"], c["workspace"], _fp(c["fp"]), _cp(c["cp"]), n_samples=S,
                                      sample_seed=seed, **dict(dict(classify=False, dense=c["dense"], cell_size=c["cell"]), **kw))


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_model(name):
    c = CASES[name]
    ctx = _context(c)
    got = _run_case(ctx, c)
    want_xyz, want_cams = PF.voxel_cloud(c)
    if len(want_xyz):
        xyz, cams = ctx.cloud()
        assert np.array_equal(xyz, want_xyz) and np.array_equal(cams, want_cams)
    m = PF.fit_model(want_xyz, c["fp"], PF.origin_of(c))
    fit = _check_fit(ctx, m, name)
    info = ctx.cluster_info()
    assert len(got) == c["cp"]["max_objects"] and all(g["n_voxels"] == len(want_xyz) for g in got)
    if fit["found"]:
        cm = CC.cluster_model(want_xyz, dict(c["cp"], plane=tuple(fit["plane"])))
        assert np.array_equal(ctx.cluster_labels(), cm["labels"])
        assert (info["n_foreground"], info["n_objects"]) == (cm["n_foreground"], cm["n_objects"])
        assert np.array_equal(info["n_voxels"], cm["sizes"])
    else:  # no plane: AGH_OK, K empty objects, no foreground
        assert (info["n_foreground"], info["n_components"], info["n_objects"]) == (0, 0, 0)
        assert all((g["samples"] == SKIP).all() and g["n_hypotheses"] == 0 and len(g["hands"]) == 0 for g in got)
        assert not ctx.cluster_labels().any()
    ctx.close()


@pytest.mark.parametrize("name", PF.CHAIN_CASES)
def test_lattice_chain_equals_the_clustered_call_with_the_reported_plane(name):
    import torch

    c = CASES[name]
    one, ref = _context(c), _context(c)
    got = _run_case(one, c)
    fit = one.plane_fit()
    assert fit["found"]
    info, labels = one.cluster_info(), one.cluster_labels()
    assert info["n_objects"] == 2
    want = ref.localize_clustered(c["points"], c["size_left"], c["workspace"], _cp(dict(c["cp"], plane=tuple(fit["plane"]))), n_samples=7,
                                  sample_seed=11, classify=False, dense=c["dense"], cell_size=c["cell"])
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (name, j))
    winfo = ref.cluster_info()
    assert all(np.array_equal(info[k], winfo[k]) for k in info) and np.array_equal(labels, ref.cluster_labels())
    # device points, read in place
    d_pts = torch.from_numpy(c["points"]).cuda()
    dev = one.localize_clustered_fit(d_pts, c["size_left"], c["workspace"], _fp(c["fp"]), _cp(c["cp"]), n_samples=7, sample_seed=11,
                                     classify=False, dense=c["dense"], cell_size=c["cell"])
    for j, (g, w) in enumerate(zip(dev, want)):
        _same(g, w, (name, "device", j))
    assert np.array_equal(_bits(one.plane_fit()["plane"]), _bits(fit["plane"]))
    one.close()
    ref.close()


@pytest.fixture(scope="module")
def scene():
    pts, size_left, ws, origins, cp, centre = PF.rotated_scene()
    pts.setflags(write=False)
    small = np.array([centre[0] - 0.05, centre[0] + 0.05, centre[1] - 0.05, centre[1] + 0.05, centre[2] - 0.05, centre[2] + 0.05])
    return dict(xyz=pts, size_left=size_left, ws=ws, small=small, origins=origins, cp=cp, fp=dict(distance_threshold=0.004, seed=2))


def _scene_call(ctx, scene, fp=None, ws=None, **kw):
    return ctx.localize_clustered_fit(np.array(scene["xyz"]), scene["size_left"], scene["ws"] if ws is None else ws,
                                      _fp(scene["fp"] if fp is None else fp), _cp(dict(scene["cp"], plane=(1.0, 0.0, 0.0, 0.0))),
                                      **dict(dict(KW, n_samples=60, sample_seed=7, dense=True), **kw))


def test_scene_chain_equality_repeatability_and_no_sticky_state(svm_model, scene):
    """The rotated table with three cubes, S = 60 per object, the classifier on.  The fitted call against the model and against
    agh_localize_clustered fed the reported plane; the same call again on the same context and on a fresh one; with the library's
    default parameters; and a plain clustered call on the context that made fitted ones against a fresh context's."""
    import torch

    one, ref, fresh = _contexts(scene["origins"], svm_model, n=3)
    xyz = np.array(scene["xyz"])
    got = _scene_call(one, scene)
    cloud, _ = one.cloud()
    fit = _check_fit(one, PF.fit_model(cloud, scene["fp"], scene["origins"][0]), "scene")
    assert fit["found"] and fit["refined"] and len(cloud) == 26399
    info, labels = one.cluster_info(), one.cluster_labels()
    assert info["n_objects"] == 3 and sum(g["n_hypotheses"] for g in got) > 0
    kw = dict(KW, n_samples=60, sample_seed=7, dense=True)
    given = _cp(dict(scene["cp"], plane=tuple(fit["plane"])))
    want = ref.localize_clustered(xyz, scene["size_left"], scene["ws"], given, **kw)
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("scene", j))
    winfo = ref.cluster_info()
    assert all(np.array_equal(info[k], winfo[k]) for k in info) and np.array_equal(labels, ref.cluster_labels())
    # the same call twice on one context, on a fresh one, and from device memory
    for ctx, what in ((one, "again"), (fresh, "fresh")):
        for j, (g, w) in enumerate(zip(_scene_call(ctx, scene), got)):
            _same(g, w, (what, j))
        again = ctx.plane_fit()
        assert all(np.array_equal(_bits(again[k]), _bits(fit[k])) if k == "plane" else again[k] == fit[k] for k in fit), what
        assert np.array_equal(ctx.cluster_labels(), labels), what
    d_xyz = torch.from_numpy(xyz).cuda()
    dev = one.localize_clustered_fit(d_xyz, scene["size_left"], scene["ws"], _fp(scene["fp"]), _cp(scene["cp"]), **kw)
    for j, (g, w) in enumerate(zip(dev, got)):
        _same(g, w, ("device", j))
    assert np.array_equal(_bits(one.plane_fit()["plane"]), _bits(fit["plane"]))
    # the defaults: 128 candidates, 1 cm, seed 1
    _scene_call(one, scene, fp={})
    _check_fit(one, PF.fit_model(cloud, {}, scene["origins"][0]), "defaults")
    # a plain clustered call after fitted ones gives what it gives on a fresh context
    for j, (g, w) in enumerate(zip(one.localize_clustered(xyz, scene["size_left"], scene["ws"], given, **kw), want)):
        _same(g, w, ("clustered after fitted", j))
    for c in (one, ref, fresh):
        c.close()


def test_the_outgrown_bitmap_repeat_holds_the_fit_parameters(svm_model, scene):
    """A context's FIRST fitted call, on a small workspace, sizes the bitmap; the wide one's lattice outgrows it and the chain runs
    once more inside the call, with the fit parameters held by the chain."""
    one, ref = _contexts(scene["origins"], svm_model)
    kw = dict(n_samples=40, sample_seed=6)
    want = _scene_call(ref, scene, **kw)
    want_fit = ref.plane_fit()
    first = _scene_call(one, scene, ws=scene["small"], **kw)
    assert first[0]["n_voxels"] > 100 and one.plane_fit()["n_voxels"] == first[0]["n_voxels"]
    builds = one.grid_stats()["builds"]
    got = _scene_call(one, scene, **kw)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the chain twice)
    fit = one.plane_fit()
    assert all(np.array_equal(_bits(fit[k]), _bits(want_fit[k])) if k == "plane" else fit[k] == want_fit[k] for k in fit)
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("repeat", j))
    one.close()
    ref.close()


def test_depth_forms_equal_the_points_form(svm_model):
    import torch

    xyz, size_left, ws, origins, cp = CC.table_scene()
    base = dict(xyz=xyz, size_left=size_left, cp=cp)
    one, ref = _contexts(origins, svm_model)
    images, dcp = _depth_scene(base)
    fp = dict(distance_threshold=0.006, seed=5, n_candidates=64)
    kw = dict(KW, n_samples=20, sample_seed=3)
    got = one.localize_depth_clustered_fit(images, ws, _fp(fp), _cp(dcp), **kw)
    cloud, _ = one.cloud()
    fit = _check_fit(one, PF.fit_model(cloud, fp, origins[0]), "depth")
    assert fit["found"] and one.cluster_info()["n_objects"] >= 1
    pts = ref.deproject(images)
    want = ref.localize_clustered_fit(pts, images[0]["data"].size, ws, _fp(fp), _cp(dcp), dense=True, **kw)
    assert np.array_equal(_bits(ref.plane_fit()["plane"]), _bits(fit["plane"]))
    assert np.array_equal(one.cluster_labels(), ref.cluster_labels())
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("depth", j))
    dev, keep = [], []
    for im in images:  # device images: rows padded, read in place
        d = im["data"]
        full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
        full[:, :d.shape[1]] = d
        t = torch.from_numpy(full.view(np.int16)).cuda()
        dev.append(dict(im, data=t[:, :d.shape[1]]))
        keep.append(t)
    for j, (g, w) in enumerate(zip(one.localize_depth_clustered_fit(dev, ws, _fp(fp), _cp(dcp), **kw), want)):
        _same(g, w, ("device depth", j))
    assert np.array_equal(_bits(one.plane_fit()["plane"]), _bits(fit["plane"]))
    one.close()
    ref.close()


def test_refusals_and_state(svm_model):
    from agile_grasp_amd import binding

    c = CASES["floor_blocks_small"]
    one = _context(c)
    bad, state, cap = binding.AGH_ERR_INVALID_ARGUMENT, binding.AGH_ERR_STATE, binding.AGH_ERR_CAPACITY
    getters = {"agh_get_plane_fit": one.plane_fit, "agh_get_plane_fit_candidates": one.plane_fit_candidates}

    def refused(call, code, text):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (text, str(e.value))

    for name, g in getters.items():  # no chain yet
        refused(g, state, name + ": ")
    got = _run_case(one, c)
    fit, cand = one.plane_fit(), one.plane_fit_candidates()
    call = lambda fp=None, cp=None, **k: _run_case(one, dict(c, fp=dict(c["fp"], **(fp or {})), cp=dict(c["cp"], **(cp or {}))), **k)
    fields = [
        ("n_candidates", dict(n_candidates=0)), ("n_candidates must be 1 .. 256", dict(n_candidates=257)),
        ("refine", dict(refine=2)), ("refine must be 0 or 1", dict(refine=-1)),
        ("min_inliers", dict(min_inliers=2)), ("reserved", dict(reserved=1)),
        ("distance_threshold", dict(distance_threshold=0.0)), ("distance_threshold", dict(distance_threshold=float("nan"))),
        ("distance_threshold", dict(distance_threshold=float("inf"))), ("distance_threshold", dict(distance_threshold=0.0500001)),
        ("distance_threshold", dict(distance_threshold=-0.01)),
    ]
    for what, fp in fields:
        refused(lambda: call(fp), bad, what)
        refused(one.localize_end, state, "")  # nothing queued
        now = one.plane_fit()  # ... and nothing changed
        assert all(now[k] == fit[k] for k in now if k != "plane") and np.array_equal(now["plane"], fit["plane"]), what
    refused(lambda: one.localize_clustered_fit(c["points"], c["size_left"], c["workspace"], None, _cp(c["cp"])), bad, "fp is NULL")
    refused(lambda: one.localize_clustered_fit(c["points"], c["size_left"], c["workspace"], _fp(c["fp"]), None), bad, "cp is NULL")
    # the clustered call's own rules hold for every field but the plane, which is neither read nor validated
    refused(lambda: call(cp=dict(tolerance=0.0)), bad, "tolerance must be in")
    refused(lambda: call(cp=dict(max_objects=65)), bad, "max_objects must be")
    refused(lambda: call(samples=np.arange(4, dtype=np.int32)), bad, "sample_idx must be NULL")
    for plane in ((np.nan, 0.0, 0.0, 0.0), (3.0, 4.0, 0.0, np.inf)):
        for j, (g, w) in enumerate(zip(call(cp=dict(plane=plane)), got)):
            _same(g, w, ("plane ignored", j))
    # a threshold of exactly 0.05, 256 candidates and min_inliers 3 are accepted
    call(dict(distance_threshold=0.05, n_candidates=256, min_inliers=3))
    refused(lambda: one.plane_fit_candidates(cap=255), cap, "agh_get_plane_fit_candidates")
    assert len(one.plane_fit_candidates(cap=256)["counts"]) == 256
    refused(lambda: call(classify=True), binding.AGH_ERR_NO_SVM, "")
    # the getters after a chain of another kind, and mid-chain
    one.load_svm(*svm_model)
    kw = dict(classify=False, dense=c["dense"], cell_size=c["cell"], n_samples=7, sample_seed=11)
    one.localize_clustered(c["points"], c["size_left"], c["workspace"], _cp(c["cp"]), **kw)
    one.cluster_info()
    for name, g in getters.items():
        refused(g, state, name + ": ")
    one.localize(c["points"], c["size_left"], c["workspace"], **kw)
    for name, g in getters.items():
        refused(g, state, name + ": ")
    call()
    assert np.array_equal(one.plane_fit_candidates()["counts"], cand["counts"])
    refused(one.label_counts, state, "")
    refused(one.sample_mask_count, state, "")
    one.localize(c["points"], c["size_left"], c["workspace"], phase="begin", **kw)
    refused(call, state, "agh_localize_clustered_fit: ")
    for name, g in getters.items():
        refused(g, state, name + ": ")
    one.localize_end()
    one.localize_batch_begin([c["points"]], [c["size_left"]], [c["workspace"]], **{k: v for k, v in kw.items() if k != "sample_seed"})
    refused(call, state, "agh_localize_clustered_fit: ")
    one.localize_batch_end()
    for j, (g, w) in enumerate(zip(call(), got)):
        _same(g, w, ("at the end", j))
    assert np.array_equal(_bits(one.plane_fit()["plane"]), _bits(fit["plane"]))
    one.close()
