"""agh_localize_clustered* and agh_localize_depth_clustered* (include/agh.h): the labelled chain with the connected components of
the voxels above a support plane as its objects.  Labels, counts, ids and sample lists are held against the numpy model of
tests/cluster_cases.py applied to the cloud agh_get_cloud returns; every object's span of every output against agh_localize with
that object's list as explicit indices, and against agh_localize_labeled fed the label image the clusters imply -- exact equality
throughout."""
import numpy as np
import pytest

from tests import cluster_cases as CC
from tests import depth_captures as D
from tests import mask_cases as M
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
SKIP = -(1 << 31)
CASES = CC.cases()


def _cp(fields):
    from agile_grasp_amd import binding

    return binding.cluster_params(**fields)


def _check_model(ctx, got, cp, S, seed, vox=None):
    """labels, info and samples of the last clustered call against the model on the context's own cloud; returns the model"""
    from agile_grasp_amd.binding import labeled_samples

    xyz, cams = ctx.cloud()
    if vox is not None:
        assert np.array_equal(xyz, vox[0]) and np.array_equal(cams, vox[1])
    m = CC.cluster_model(xyz, cp)
    info = ctx.cluster_info()
    labels = ctx.cluster_labels()
    print("voxels", len(xyz), "foreground", info["n_foreground"], "components", info["n_components"], "objects", info["n_objects"],
          "M", list(info["n_voxels"]), "hypotheses", [g["n_hypotheses"] for g in got])
    assert len(labels) == len(xyz) and np.array_equal(labels, m["labels"])
    assert (info["n_foreground"], info["n_components"], info["n_objects"]) == (m["n_foreground"], m["n_components"], m["n_objects"])
    assert np.array_equal(info["n_voxels"], m["sizes"]) and np.array_equal(info["ids"], m["ids"])
    assert len(got) == cp["max_objects"] and all(g["n_voxels"] == len(xyz) for g in got)
    want = labeled_samples(m["lists"], S, seed)
    assert np.array_equal(np.concatenate([g["samples"] for g in got]) if S else np.zeros(0, np.int32), want)
    return m


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_model(name):
    from agile_grasp_amd import binding

    c = CASES[name]
    ctx = binding.Context(np.zeros((2, 3)))
    S = {"snake": 40, "seventy_components": 5}.get(name, 7)
    kw = dict(classify=False, dense=c["dense"], cell_size=c["cell"])
    got = ctx.localize_clustered(c["points"], c["size_left"], c["workspace"], _cp(c["cp"]), n_samples=S, sample_seed=11, **kw)
    m = _check_model(ctx, got, c["cp"], S, 11, CC.voxel_cloud(c))
    for j in range(c["cp"]["max_objects"]):
        if m["sizes"][j] == 0:
            assert (got[j]["samples"] == SKIP).all() and got[j]["n_hypotheses"] == 0 and len(got[j]["hands"]) == 0
    # the stage runs for n_samples = 0 too
    got = ctx.localize_clustered(c["points"], c["size_left"], c["workspace"], _cp(c["cp"]), n_samples=0, **kw)
    _check_model(ctx, got, c["cp"], 0, 1)
    ctx.close()


@pytest.fixture(scope="module")
def scene():
    xyz, size_left, ws, origins, cp = CC.table_scene()
    xyz.setflags(write=False)
    ws_cut = ws.copy()
    ws_cut[1] = 0.75 + 25 * 0.003 + 0.004  # the +x face through the second cube
    return dict(xyz=xyz, size_left=size_left, ws=ws, ws_cut=ws_cut, origins=origins, cp=cp)


def _raw_labels(xyz, size_left, ws, vox_labels):
    """the label image the clusters imply: every kept raw point gets the byte of its voxel (mask_cases.bit_positions: a
    camera's voxels are its distinct bit positions in ascending order, camera 0's block first)"""
    cams = M.camera_ids(xyz, size_left, True)
    out, base = np.zeros(len(xyz), np.uint8), 0
    for sel, _c, pos, _dim in M.bit_positions(xyz, cams, ws):
        uniq = np.unique(pos)
        out[sel] = vox_labels[base + np.searchsorted(uniq, pos)]
        base += len(uniq)
    assert base == len(vox_labels)
    return out


@pytest.mark.parametrize("mode", ["classified", "boundaries"])
def test_chain_equality(svm_model, scene, mode):
    """A table with three cubes, S = 60 per object, seed 7, the classifier on, min_inliers = 2; K = 4, so the last object is empty.
    Every object's span against agh_localize with the object's reported list as explicit indices, and against agh_localize_labeled
    with the clusters' labels mapped back to the raw points -- then with filters_boundaries on a workspace cut through a cube."""
    one, ref = _contexts(scene["origins"], svm_model)
    ws = scene["ws"] if mode == "classified" else scene["ws_cut"]
    kw = dict(KW, n_samples=60, sample_seed=7, filters_boundaries=mode == "boundaries", dense=True)
    xyz = np.array(scene["xyz"])
    got = one.localize_clustered(xyz, scene["size_left"], ws, _cp(scene["cp"]), **kw)
    m = _check_model(one, got, scene["cp"], 60, 7)
    print(mode, "hands", [len(g["hands"]) for g in got], "handles", [len(g["handles"]) for g in got])
    assert m["n_objects"] == 3 and m["sizes"][3] == 0 and got[3]["n_hypotheses"] == 0
    assert sum(g["n_hypotheses"] for g in got) > 0
    labels = one.cluster_labels()
    for j in range(4):
        want = ref.localize(xyz, scene["size_left"], ws, samples=got[j]["samples"], **dict(kw, n_samples=0))
        _same(got[j], want, (mode, "explicit", j))
    lab = ref.localize_labeled(xyz, scene["size_left"], ws, _raw_labels(xyz, scene["size_left"], ws, labels), 4, **kw)
    assert np.array_equal(ref.label_counts(), m["sizes"])
    for j in range(4):
        _same(got[j], lab[j], (mode, "labelled", j))
    one.close()
    ref.close()


def _depth_scene(scene):
    images = [D.render_depth(scene["xyz"][:scene["size_left"]] if k == 0 else scene["xyz"][scene["size_left"]:], k, 64, 48, D.U16,
                             52.0, pad=1 + 2 * k) for k in range(2)]
    cp = dict(scene["cp"], min_height=0.015, tolerance=0.03, min_voxels=5)
    return images, cp


def test_depth_form_equals_points_form(svm_model, scene):
    import torch

    one, ref = _contexts(scene["origins"], svm_model)
    images, cp = _depth_scene(scene)
    kw = dict(KW, n_samples=20, sample_seed=3)
    got = one.localize_depth_clustered(images, scene["ws"], _cp(cp), **kw)
    m = _check_model(one, got, cp, 20, 3)
    assert m["n_objects"] >= 1
    pts = ref.deproject(images)
    want = ref.localize_clustered(pts, images[0]["data"].size, scene["ws"], _cp(cp), dense=True, **kw)
    assert np.array_equal(one.cluster_labels(), ref.cluster_labels())
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("depth", j))
    # device images: rows padded, read in place
    dev, keep = [], []
    for im in images:
        d = im["data"]
        full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
        full[:, :d.shape[1]] = d
        t = torch.from_numpy(full.view(np.int16)).cuda()
        dev.append(dict(im, data=t[:, :d.shape[1]]))
        keep.append(t)
    for j, (g, w) in enumerate(zip(one.localize_depth_clustered(dev, scene["ws"], _cp(cp), **kw), want)):
        _same(g, w, ("device depth", j))
    one.close()
    ref.close()


def test_device_points_with_an_odd_stride_and_an_odd_base(svm_model, scene):
    import torch

    one, ref = _contexts(scene["origins"], svm_model)
    kw = dict(KW, n_samples=40, sample_seed=9, dense=True)
    xyz = np.array(scene["xyz"])
    want = ref.localize_clustered(xyz, scene["size_left"], scene["ws"], _cp(scene["cp"]), **kw)
    # records of five floats, the first one a float into the allocation
    flat = torch.full((1 + 5 * len(xyz),), 7.0, dtype=torch.float32)
    rec = flat[1:].view(len(xyz), 5)
    rec[:, :3] = torch.from_numpy(xyz)
    d_flat = flat.cuda()
    view = d_flat[1:].view(len(xyz), 5)
    assert view.data_ptr() == d_flat.data_ptr() + 4 and view.stride(0) == 5
    got = one.localize_clustered(view, scene["size_left"], scene["ws"], _cp(scene["cp"]), **kw)
    assert np.array_equal(one.cluster_labels(), ref.cluster_labels())
    assert one.cluster_info()["n_objects"] == 3
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("device", j))
    one.close()
    ref.close()


def test_the_outgrown_bitmap_repeat_inside_a_clustered_call(svm_model, scene):
    """A small workspace sizes the context's bitmap; the wide one's lattice outgrows it and the chain is run once more inside the
    call, with the cluster parameters held by the chain."""
    one, ref = _contexts(scene["origins"], svm_model)
    kw = dict(KW, n_samples=40, sample_seed=6, dense=True)
    xyz = np.array(scene["xyz"])
    small = np.array([0.70, 0.80, -0.05, 0.05, -0.2, 0.2])
    want = ref.localize_clustered(xyz, scene["size_left"], scene["ws"], _cp(scene["cp"]), **kw)
    first = one.localize_clustered(xyz, scene["size_left"], small, _cp(scene["cp"]), **kw)
    assert first[0]["n_voxels"] > 100
    builds = one.grid_stats()["builds"]
    got = one.localize_clustered(xyz, scene["size_left"], scene["ws"], _cp(scene["cp"]), **kw)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the chain twice)
    _check_model(one, got, scene["cp"], 40, 6)
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("repeat", j))
    one.close()
    ref.close()


def test_no_sticky_state(svm_model, scene):
    from agile_grasp_amd import binding

    one, fresh = _contexts(scene["origins"], svm_model)
    kw = dict(KW, n_samples=50, sample_seed=5, dense=True)
    xyz, n0, ws = np.array(scene["xyz"]), scene["size_left"], scene["ws"]
    raw = (np.arange(len(xyz)) % 3).astype(np.uint8)
    want_c = fresh.localize_clustered(xyz, n0, ws, _cp(scene["cp"]), **kw)
    info_c = fresh.cluster_info()

    def state(call):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE

    def clustered():
        for j, (g, w) in enumerate(zip(one.localize_clustered(xyz, n0, ws, _cp(scene["cp"]), **kw), want_c)):
            _same(g, w, ("clustered", j))
        assert np.array_equal(one.cluster_info()["n_voxels"], info_c["n_voxels"])
        state(one.label_counts)
        state(one.sample_mask_count)

    others = {
        "plain": lambda c: [c.localize(xyz, n0, ws, **kw)],
        "masked": lambda c: [c.localize_masked(xyz, n0, ws, (raw == 1).astype(np.uint8), **kw)],
        "labelled": lambda c: c.localize_labeled(xyz, n0, ws, raw, 2, **kw),
    }
    want_o = {k: f(fresh) for k, f in others.items()}
    for name, f in others.items():  # both orders: clustered, other, clustered
        clustered()
        for j, (g, w) in enumerate(zip(f(one), want_o[name])):
            _same(g, w, (name, "after clustered", j))
        state(one.cluster_info)
        state(one.cluster_labels)
    clustered()
    one.close()
    fresh.close()


def test_refusals(svm_model, scene):
    from agile_grasp_amd import binding

    one, ref = _contexts(scene["origins"], svm_model)
    kw = dict(KW, n_samples=40, sample_seed=8, dense=True)
    xyz, n0, ws = np.array(scene["xyz"]), scene["size_left"], scene["ws"]
    images, dcp = _depth_scene(scene)
    want = ref.localize_clustered(xyz, n0, ws, _cp(scene["cp"]), **kw)
    got = one.localize_clustered(xyz, n0, ws, _cp(scene["cp"]), **kw)
    sizes = one.cluster_info()["n_voxels"]
    assert [g["n_hypotheses"] for g in got] == [w["n_hypotheses"] for w in want]
    bad, state, cap = binding.AGH_ERR_INVALID_ARGUMENT, binding.AGH_ERR_STATE, binding.AGH_ERR_CAPACITY
    points = lambda cp=None, **k: one.localize_clustered(xyz, n0, ws, _cp(dict(scene["cp"], **(cp or {}))), **dict(kw, **k))
    dkw = {a: b for a, b in kw.items() if a != "dense"}
    depth = lambda cp=None, **k: one.localize_depth_clustered(images, ws, _cp(dict(dcp, **(cp or {}))), **dict(dkw, **k))
    calls = [
        ("plane[1]", lambda: points(dict(plane=(0.0, np.nan, 1.0, 0.1)))),
        ("plane[3]", lambda: points(dict(plane=(0.0, 0.0, 1.0, np.inf)))),
        ("min_height", lambda: points(dict(min_height=-np.inf))),
        ("max_height", lambda: depth(dict(max_height=np.nan))),
        ("tolerance", lambda: points(dict(tolerance=np.nan))),
        ("unit vector", lambda: points(dict(plane=(0.0, 0.0, 1.0 + 2e-6, 0.1)))),
        ("unit vector", lambda: depth(dict(plane=(0.0, 0.6, 0.7, 0.1)))),
        ("min_height must be below max_height", lambda: points(dict(min_height=0.5, max_height=0.5))),
        ("tolerance must be in", lambda: points(dict(tolerance=0.0))),
        ("tolerance must be in (0, 0.05]", lambda: depth(dict(tolerance=0.0500001))),
        ("min_voxels", lambda: points(dict(min_voxels=0))),
        ("max_objects must be 1 .. 64", lambda: points(dict(max_objects=0))),
        ("max_objects must be", lambda: depth(dict(max_objects=65))),
        ("max_objects x n_samples", lambda: points(dict(max_objects=64), n_samples=(1 << 18) + 1, caps=(1, 1, 1))),
        ("sample_idx", lambda: points(samples=np.arange(10, dtype=np.int32))),
        ("sample_idx must be NULL", lambda: depth(samples=np.arange(10, dtype=np.int32))),
        ("cp is NULL", lambda: one.localize_clustered(xyz, n0, ws, None, **kw)),
        ("agh_localize", lambda: points(n_samples=-1)),  # (a twin's validation)
    ]
    for what, call in calls:
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == bad and what in str(e.value), (what, str(e.value))
        # nothing queued, nothing bound or changed
        with pytest.raises(binding.AghError) as e:
            one.localize_end()
        assert e.value.code == state, what
        assert np.array_equal(one.cluster_info()["n_voxels"], sizes), what
    # (a tolerance of exactly 0.05 and a unit vector within 1e-6 are accepted)
    points(dict(tolerance=0.05, plane=(0.0, 0.0, 1.0 + 4e-7, 0.099)), n_samples=2)
    for j, (g, w) in enumerate(zip(points(), want)):
        _same(g, w, ("after the refusals", j))
    plain = binding.Context(scene["origins"])
    with pytest.raises(binding.AghError) as e:
        plain.localize_clustered(xyz, n0, ws, _cp(scene["cp"]), **kw)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    # buffers that are too small: every results[j] filled, and the repeat sized from them succeeds
    with pytest.raises(binding.AghError) as e:
        points(caps=(1, 1, 1))
    assert e.value.code == cap and "agh_localize_clustered" in str(e.value)
    counts = one.last_batch_counts
    assert [r["n_hypotheses"] for r in counts] == [w["n_hypotheses"] for w in want]
    assert [r["first_sample"] for r in counts] == [40 * j for j in range(4)]
    sized = (sum(r["n_handles"] for r in counts), sum(r["n_inlier_idx"] for r in counts), sum(r["n_hands"] for r in counts))
    for j, (g, w) in enumerate(zip(points(caps=sized), want)):
        _same(g, w, ("sized from the counts", j))
    with pytest.raises(binding.AghError) as e:
        one.cluster_info(cap_objects=3)
    assert e.value.code == cap
    with pytest.raises(binding.AghError) as e:
        one.cluster_labels(cap=10)
    assert e.value.code == cap
    # mid-chain and mid-batch: the four calls and the two getters are refused, the chain in flight is untouched
    import torch

    d_xyz = torch.from_numpy(xyz).cuda()
    d_images = [dict(im, data=torch.from_numpy(np.ascontiguousarray(im["data"]).view(np.int16)).cuda()) for im in images]
    clustered_calls = {
        "agh_localize_clustered": points,
        "agh_localize_clustered_device": lambda: one.localize_clustered(d_xyz, n0, ws, _cp(scene["cp"]), **kw),
        "agh_localize_depth_clustered": depth,
        "agh_localize_depth_clustered_device": lambda: one.localize_depth_clustered(d_images, ws, _cp(dcp), n_samples=20, **KW),
        "agh_get_cluster_info": one.cluster_info,
        "agh_get_cluster_labels": one.cluster_labels,
    }
    ckw = dict(KW, n_samples=50, sample_seed=8, dense=True)
    chain_want = ref.localize(xyz, n0, ws, **ckw)
    one.localize(xyz, n0, ws, phase="begin", **ckw)
    for name, call in clustered_calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == state and name + ": " in str(e.value), (name, str(e.value))
    _same(one.localize_end(), chain_want, "after the mid-chain refusals")
    batch_want = ref.localize_batch([xyz], [n0], [ws], n_samples=50, dense=True, **KW)
    one.localize_batch_begin([xyz], [n0], [ws], n_samples=50, dense=True, **KW)
    for name, call in clustered_calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == state and name + ": " in str(e.value), (name, str(e.value))
    _same(one.localize_batch_end()[0], batch_want[0], "after the mid-batch refusals")
    for j, (g, w) in enumerate(zip(points(), want)):
        _same(g, w, ("at the end", j))
    one.close()
    ref.close()
