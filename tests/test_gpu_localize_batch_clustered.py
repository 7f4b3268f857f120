"""agh_localize_batch_clustered* and agh_localize_depth_batch_clustered* (include/agh.h): the labelled batch chain with every
capture's own connected components as its objects.  Per capture, labels, counts, ids and sample lists are held against the numpy
model of tests/cluster_cases.py applied to that capture's slice of the cloud agh_get_cloud returns; every capture's spans against
agh_localize_clustered on it alone, and the whole call against agh_localize_batch_labeled fed the label bytes the clusters imply
-- exact equality throughout."""
import numpy as np
import pytest

from tests import cluster_batch_cases as B
from tests import cluster_cases as CC
from tests import cluster_grid_cases as G
from tests import grid_scale_clouds as gs
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same
from tests.test_gpu_localize_clustered import _depth_scene, _raw_labels

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
SKIP = -(1 << 31)


def _cps(fields):
    from agile_grasp_amd import binding

    return [binding.cluster_params(**f) for f in fields]


def _slices(got):
    """capture k's voxels in the bound batch, from the counts the call reported"""
    off = np.concatenate([[0], np.cumsum([objs[0]["n_voxels"] for objs in got])]).astype(np.int64)
    return [slice(int(off[k]), int(off[k + 1])) for k in range(len(got))]


def _check_models(ctx, got, cps, S, seeds, models=None, clouds=None):
    """Per capture: labels, info, M, capture-local ids and samples of the last clustered batch against the model of the capture's
    own slice of the context's cloud (models[k]: a model computed beforehand, of clouds[k]); returns the models."""
    from agile_grasp_amd.binding import labeled_samples

    xyz, cams = ctx.cloud()
    info, labels = ctx.batch_cluster_info(), ctx.batch_cluster_labels()
    sl = _slices(got)
    assert len(got) == len(cps) and len(labels) == len(xyz) == sl[-1].stop
    first = np.concatenate([[0], np.cumsum([cp["max_objects"] for cp in cps])])
    assert len(info["n_voxels"]) == len(info["ids"]) == first[-1] and len(info["n_foreground"]) == len(cps)
    out = []
    for k, cp in enumerate(cps):
        if clouds is not None:
            assert np.array_equal(xyz[sl[k]], clouds[k][0]) and np.array_equal(cams[sl[k]], clouds[k][1]), k
        m = models[k] if models is not None else CC.cluster_model(xyz[sl[k]], cp)
        l0, l1 = first[k], first[k + 1]
        print("capture", k, "voxels", sl[k].stop - sl[k].start, "foreground", info["n_foreground"][k], "components",
              info["n_components"][k], "objects", info["n_objects"][k], "M", list(info["n_voxels"][l0:l1][:8]), "hypotheses",
              [g["n_hypotheses"] for g in got[k]][:8])
        assert np.array_equal(labels[sl[k]], m["labels"]), k
        assert (info["n_foreground"][k], info["n_components"][k], info["n_objects"][k]) == (m["n_foreground"], m["n_components"],
                                                                                           m["n_objects"]), k
        assert np.array_equal(info["n_voxels"][l0:l1], m["sizes"]) and np.array_equal(info["ids"][l0:l1], m["ids"]), k
        assert len(got[k]) == cp["max_objects"] and all(g["n_voxels"] == sl[k].stop - sl[k].start for g in got[k]), k
        want = labeled_samples(m["lists"], S[k], seeds[k])
        assert np.array_equal(np.concatenate([g["samples"] for g in got[k]]) if S[k] else np.zeros(0, np.int32), want), k
        for j in range(cp["max_objects"]):  # every empty list is all INT32_MIN with zero hypotheses
            if m["sizes"][j] == 0:
                g = got[k][j]
                assert (g["samples"] == SKIP).all() and g["n_hypotheses"] == 0 and len(g["hands"]) == 0 and len(g["handles"]) == 0
        out.append(m)
    return out


def _call_cases(ctx, batch, S, seeds, **kw):
    a = B.args(batch)
    return ctx.localize_batch_clustered(a["captures"], a["sizes_left"], a["workspaces"], _cps(a["cp"]), n_samples=list(S),
                                        sample_seeds=list(seeds), classify=False, dense=a["dense"], cell_size=a["cell"], **kw)


def test_all_twelve_small_cases_as_one_batch():
    """L = 64 lists, classifier off, S = 7 (snake: 40), seed 11; then S = 0.  no_foreground sits in the middle; the two threshold
    captures occupy the same coordinates under two tolerances and keep 1 and 2 components."""
    from agile_grasp_amd import binding

    batch = B.small_batch()
    cps = [c["cp"] for _, c in batch]
    clouds = [CC.voxel_cloud(c) for _, c in batch]
    ctx = binding.Context(np.zeros((2, 3)))
    S, seeds = B.small_samples(batch), [11] * len(batch)
    got = _call_cases(ctx, batch, S, seeds)
    assert sum(len(objs) for objs in got) == 64
    models = _check_models(ctx, got, cps, S, seeds, clouds=clouds)
    names = [n for n, _ in batch]
    a, b, none = names.index("threshold_neighbours"), names.index("threshold_neighbours_above"), names.index("no_foreground")
    assert np.array_equal(clouds[a][0], clouds[b][0])  # the same coordinates ...
    assert models[a]["n_components"] == 1 and models[b]["n_components"] == 2  # ... and each its own components, under its own cp
    assert models[none]["n_foreground"] == 0 and models[none - 1]["n_objects"] > 0 and models[none + 1]["n_objects"] > 0
    assert models[names.index("seventy_components")]["n_objects"] == 22
    # the stage runs for S_k = 0 too
    zero = [0] * len(batch)
    got = _call_cases(ctx, batch, zero, seeds)
    _check_models(ctx, got, cps, zero, seeds, models=models)
    ctx.close()


def test_uneven_sizes_and_grids_forwards_and_in_reverse():
    """Four captures of 1 cm voxels whose grids have cells of 0.04 / 0.02 / 0.08 / 0.02 m (reach 2 / 3 / 1 / 1) and 5332 / 620 /
    5332 / 16 voxels: every capture against its model and its descriptor against the grid model; then the reversed batch on the
    same context, on the descriptors the first build kept per cloud slot."""
    from agile_grasp_amd import binding

    ctx, g = binding.Context(np.zeros((2, 3))), gs.GridModel()
    fwd = B.grid_batch()
    for step, batch in enumerate((fwd, fwd[::-1])):
        cps = [c["cp"] for _, c in batch]
        clouds = [CC.voxel_cloud(c) for _, c in batch]
        models = [G.model(n)["m"] if n in G.cases() else CC.cluster_model(x, cp) for (n, _), (x, _c), cp in zip(batch, clouds, cps)]
        S, seeds = [3, 5, 3, 5][::1 - 2 * step], [20 + step] * 4
        got = _call_cases(ctx, batch, S, seeds)
        _check_models(ctx, got, cps, S, seeds, models=models, clouds=clouds)
        descs = g.build([x for x, _c in clouds])
        for k, (d, regime) in enumerate(descs):
            print(step, k, regime, ctx.grid_desc(k))
            assert ctx.grid_desc(k) == d.as_dict(), (step, k)
            if step == 0:  # (the reversed batch runs on whatever descriptor its cloud slot kept: the grid model says which)
                assert (d.cell, G.reach_of(cps[k]["tolerance"], d.cell)) == (B.GRID_CELLS[k], B.GRID_REACH[k])
        assert ctx.grid_stats() == g.stats
    ctx.close()


def _table_kw(scenes, mode):
    return dict(KW, n_samples=[s["S"] for s in scenes], sample_seeds=[7, 8, 9], filters_boundaries=mode == "boundaries", dense=True)


def _table_call(ctx, scenes, mode, begin=False, **over):
    ws = [s["ws_cut" if mode == "boundaries" else "ws"] for s in scenes]
    f = ctx.localize_batch_clustered_begin if begin else ctx.localize_batch_clustered
    return f([np.array(s["xyz"]) for s in scenes], [s["size_left"] for s in scenes], ws, _cps([s["cp"] for s in scenes]),
             **dict(_table_kw(scenes, mode), **over))


def _table_twins(ref, scenes, mode):
    """agh_localize_clustered on every capture alone: (results, infos, label bytes)"""
    kw = _table_kw(scenes, mode)
    out, infos, labels = [], [], []
    for k, s in enumerate(scenes):
        out.append(ref.localize_clustered(np.array(s["xyz"]), s["size_left"], s["ws_cut" if mode == "boundaries" else "ws"],
                                          _cps([s["cp"]])[0], n_samples=s["S"], sample_seed=kw["sample_seeds"][k], dense=True,
                                          filters_boundaries=kw["filters_boundaries"], **KW))
        infos.append(ref.cluster_info())
        labels.append(ref.cluster_labels())
    return out, infos, labels


def _same_batch(got, want, what):
    assert len(got) == len(want), what
    for k, (objs, w) in enumerate(zip(got, want)):
        assert len(objs) == len(w), (what, k)
        for j, (a, b) in enumerate(zip(objs, w)):
            _same(a, b, (what, "capture", k, "object", j))


@pytest.mark.parametrize("mode", ["classified", "boundaries"])
def test_chain_equality(svm_model, mode):
    """table_scene(5), (6), (7) with K = 4, 3, 5 and S = 60, 45, 60, the classifier on, min_inliers = 2: every capture's spans
    against agh_localize_clustered on it alone, the whole call against agh_localize_batch_labeled with the reported label bytes
    mapped back to the raw points -- then with filters_boundaries on a workspace cut through a cube."""
    scenes = B.table_scenes()
    one, ref = _contexts(scenes[0]["origins"], svm_model)
    got = _table_call(one, scenes, mode)
    cps = [s["cp"] for s in scenes]
    kw = _table_kw(scenes, mode)
    models = _check_models(one, got, cps, kw["n_samples"], kw["sample_seeds"])
    assert [m["n_objects"] for m in models] == [3, 3, 3]
    info, labels, sl = one.batch_cluster_info(), one.batch_cluster_labels(), _slices(got)
    want, infos, twin_labels = _table_twins(ref, scenes, mode)
    print(mode, "handles of the twins", [[len(g["handles"]) for g in w] for w in want], "hands", [[len(g["hands"]) for g in w] for w in want])
    if mode == "classified":  # (the condition of the batch, on the twin: at least two objects with a handle in every capture)
        assert all(sum(len(g["handles"]) >= 1 for g in w) >= 2 for w in want)
    assert all(sum(g["n_hypotheses"] for g in w) > 0 for w in want)
    _same_batch(got, want, (mode, "twin"))
    first = B.first_lists([(k, dict(cp=cp)) for k, cp in enumerate(cps)])
    for k, (ti, tl) in enumerate(zip(infos, twin_labels)):
        assert np.array_equal(labels[sl[k]], tl), k
        assert (info["n_foreground"][k], info["n_components"][k], info["n_objects"][k]) == (ti["n_foreground"], ti["n_components"],
                                                                                           ti["n_objects"])
        assert np.array_equal(info["n_voxels"][first[k]:first[k + 1]], ti["n_voxels"])
        assert np.array_equal(info["ids"][first[k]:first[k + 1]], ti["ids"])
    ws = [s["ws_cut" if mode == "boundaries" else "ws"] for s in scenes]
    raw = [_raw_labels(np.asarray(s["xyz"]), s["size_left"], w, labels[sl[k]]) for k, (s, w) in enumerate(zip(scenes, ws))]
    lab = ref.localize_batch_labeled([np.array(s["xyz"]) for s in scenes], [s["size_left"] for s in scenes], ws, raw,
                                     [cp["max_objects"] for cp in cps], **kw)
    assert np.array_equal(ref.batch_label_counts(), info["n_voxels"])
    _same_batch(got, lab, (mode, "labelled batch"))
    one.close()
    ref.close()


def _depth_batch(scenes):
    """two captures of two 64 x 48 images each, with the cluster parameters of the depth scene"""
    caps, cps = [], []
    for s in scenes[:2]:
        images, cp = _depth_scene(s)
        caps.append(images)
        cps.append(cp)
    return caps, cps


def test_depth_forms_equal_the_points_forms(svm_model):
    """host and device images against the points form on agh_deproject_batch's arrays; device points at an odd stride and an
    odd base; a camera-origin table of n_captures rows, row k the rig of capture k, against the single call with that row"""
    import torch

    scenes = B.table_scenes()
    one, ref = _contexts(scenes[0]["origins"], svm_model)
    caps, cps = _depth_batch(scenes)
    ws = [s["ws"] for s in scenes[:2]]
    kw = dict(KW, n_samples=[20, 16], sample_seeds=[3, 4])
    got = one.localize_depth_batch_clustered(caps, ws, _cps(cps), **kw)
    models = _check_models(one, got, cps, kw["n_samples"], kw["sample_seeds"])
    assert all(m["n_objects"] >= 1 for m in models)
    labels = one.batch_cluster_labels()
    pts = ref.deproject_batch(caps)
    counts = [sum(im["data"].size for im in images) for images in caps]
    split = [pts[:counts[0]], pts[counts[0]:]]
    sizes_left = [images[0]["data"].size for images in caps]
    want = ref.localize_batch_clustered(split, sizes_left, ws, _cps(cps), dense=True, **kw)
    assert np.array_equal(labels, ref.batch_cluster_labels())
    _same_batch(got, want, "depth")
    for k in range(2):  # ... and the depth form's twin, capture by capture
        twin = ref.localize_depth_clustered(caps[k], ws[k], _cps(cps)[k], n_samples=kw["n_samples"][k], sample_seed=kw["sample_seeds"][k],
                                            **KW)
        _same_batch([got[k]], [twin], ("depth twin", k))
    # device images: rows padded, read in place
    dev, keep = [], []
    for images in caps:
        dev.append([])
        for im in images:
            d = im["data"]
            full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
            full[:, :d.shape[1]] = d
            t = torch.from_numpy(full.view(np.int16)).cuda()
            dev[-1].append(dict(im, data=t[:, :d.shape[1]]))
            keep.append(t)
    _same_batch(one.localize_depth_batch_clustered(dev, ws, _cps(cps), **kw), want, "device depth")
    # device points: records of five floats, the first one a float into the allocation
    views = []
    for p in split:
        flat = torch.full((1 + 5 * len(p),), 7.0, dtype=torch.float32)
        flat[1:].view(len(p), 5)[:, :3] = torch.from_numpy(p)
        d_flat = flat.cuda()
        keep.append(d_flat)
        views.append(d_flat[1:].view(len(p), 5))
        assert views[-1].data_ptr() == d_flat.data_ptr() + 4 and views[-1].stride(0) == 5
    _same_batch(one.localize_batch_clustered(views, sizes_left, ws, _cps(cps), dense=True, **kw), want, "device points")
    assert np.array_equal(one.batch_cluster_labels(), labels)
    # a per-capture camera-origin table: n_captures rows, not one per list
    o = np.asarray(scenes[0]["origins"], np.float64)
    table = np.stack([o, o + np.array([[0.0, 0.01, 0.0], [0.0, -0.01, 0.02]])])
    one.set_cloud_cam_origins(table)
    tabled = one.localize_depth_batch_clustered(caps, ws, _cps(cps), **kw)
    for k in range(2):
        ref.set_cloud_cam_origins(table[k:k + 1])
        twin = ref.localize_depth_clustered(caps[k], ws[k], _cps(cps)[k], n_samples=kw["n_samples"][k], sample_seed=kw["sample_seeds"][k],
                                            **KW)
        _same_batch([tabled[k]], [twin], ("origin table", k))
    one.close()
    ref.close()


def _state(call, name=None):
    from agile_grasp_amd import binding

    with pytest.raises(binding.AghError) as e:
        call()
    assert e.value.code == binding.AGH_ERR_STATE and (name is None or name + ": " in str(e.value)), (name, str(e.value))


def test_begin_and_end(svm_model):
    """begin + end equals the blocking form; mid-chain the new calls and getters are refused and the chain is untouched; a batch
    whose lattices outgrow the kept slots is run once more inside the call, with the cp records the chain holds"""
    import torch

    scenes = B.table_scenes()
    one, ref = _contexts(scenes[0]["origins"], svm_model)
    want = _table_call(ref, scenes, "classified")
    want_labels = ref.batch_cluster_labels()
    caps, dcps = _depth_batch(scenes)
    # a first small batch sizes the kept slots
    small = np.array([0.70, 0.80, -0.05, 0.05, -0.2, 0.2])
    first = one.localize_batch_clustered([np.array(s["xyz"]) for s in scenes], [s["size_left"] for s in scenes], [small] * 3,
                                         _cps([s["cp"] for s in scenes]), **_table_kw(scenes, "classified"))
    assert all(objs[0]["n_voxels"] > 100 for objs in first)
    builds = one.grid_stats()["builds"]
    _table_call(one, scenes, "classified", begin=True)
    assert one.grid_stats()["builds"] - builds == 1
    d_xyz = [torch.from_numpy(np.array(s["xyz"])).cuda() for s in scenes]
    d_caps = [[dict(im, data=torch.from_numpy(np.ascontiguousarray(im["data"]).view(np.int16)).cuda()) for im in images] for images in caps]
    pkw = _table_kw(scenes, "classified")
    dkw = dict(KW, n_samples=10)
    n0, ws, cps = [s["size_left"] for s in scenes], [s["ws"] for s in scenes], [s["cp"] for s in scenes]
    dws = ws[:2]
    refused = {
        "agh_localize_batch_clustered": lambda: _table_call(one, scenes, "classified"),
        "agh_localize_batch_clustered_device": lambda: one.localize_batch_clustered(d_xyz, n0, ws, _cps(cps), **pkw),
        "agh_localize_batch_clustered_begin": lambda: _table_call(one, scenes, "classified", begin=True),
        "agh_localize_batch_clustered_begin_device": lambda: one.localize_batch_clustered_begin(d_xyz, n0, ws, _cps(cps), **pkw),
        "agh_localize_depth_batch_clustered": lambda: one.localize_depth_batch_clustered(caps, dws, _cps(dcps), **dkw),
        "agh_localize_depth_batch_clustered_device": lambda: one.localize_depth_batch_clustered(d_caps, dws, _cps(dcps), **dkw),
        "agh_localize_depth_batch_clustered_begin": lambda: one.localize_depth_batch_clustered_begin(caps, dws, _cps(dcps), **dkw),
        "agh_localize_depth_batch_clustered_begin_device": lambda: one.localize_depth_batch_clustered_begin(d_caps, dws, _cps(dcps), **dkw),
        "agh_get_batch_cluster_info": one.batch_cluster_info,
        "agh_get_batch_cluster_labels": lambda: one.batch_cluster_labels(cap=1 << 20),
    }
    pending = one._batch_pending
    for name, call in refused.items():
        _state(call, name)
        one._batch_pending = pending  # (a refused begin of the binding leaves its own note of the chain alone)
    got = one.localize_batch_end()
    assert one.grid_stats()["builds"] - builds == 2  # (the slots were outgrown: the call ran the chain twice)
    _same_batch(got, want, "begin / end after the outgrown-slot repeat")
    assert np.array_equal(one.batch_cluster_labels(), want_labels)
    # ... and in the steady state: one pass
    _table_call(one, scenes, "classified", begin=True)
    _same_batch(one.localize_batch_end(), want, "begin / end")
    assert one.grid_stats()["builds"] - builds == 3
    # a chain of another kind in flight refuses the new calls too, and is collected untouched
    chain_want = ref.localize(np.array(scenes[0]["xyz"]), n0[0], ws[0], n_samples=50, sample_seed=8, dense=True, **KW)
    one.localize(np.array(scenes[0]["xyz"]), n0[0], ws[0], phase="begin", n_samples=50, sample_seed=8, dense=True, **KW)
    for name in ("agh_localize_batch_clustered", "agh_localize_depth_batch_clustered_begin", "agh_get_batch_cluster_info"):
        _state(refused[name], name)
    one._batch_pending = None
    _same(one.localize_end(), chain_want, "after the mid-chain refusals")
    one.close()
    ref.close()


def test_no_sticky_state(svm_model):
    """clustered batch -> single clustered -> labelled batch -> clustered batch on one context: each equals its result on a fresh
    context, and every getter answers only for its own kind"""
    scenes = B.table_scenes()
    one, fresh = _contexts(scenes[0]["origins"], svm_model)
    s0 = scenes[0]
    xyzs, n0, ws = [np.array(s["xyz"]) for s in scenes], [s["size_left"] for s in scenes], [s["ws"] for s in scenes]
    raw = [(np.arange(len(x)) % 3).astype(np.uint8) for x in xyzs]
    skw = dict(KW, n_samples=50, sample_seed=5, dense=True)
    lkw = dict(KW, n_samples=[30, 20, 30], sample_seeds=[1, 2, 3], dense=True)
    want_b = _table_call(fresh, scenes, "classified")
    info_b, labels_b = fresh.batch_cluster_info(), fresh.batch_cluster_labels()
    want_s = fresh.localize_clustered(xyzs[0], n0[0], ws[0], _cps([s0["cp"]])[0], **skw)
    info_s = fresh.cluster_info()
    want_l = fresh.localize_batch_labeled(xyzs, n0, ws, raw, [2, 2, 2], **lkw)
    counts_l = fresh.batch_label_counts()
    others = (one.sample_mask_count, one.label_counts, one.cluster_info, one.cluster_labels, one.batch_mask_counts, one.batch_label_counts)

    def clustered_batch():
        _same_batch(_table_call(one, scenes, "classified"), want_b, "clustered batch")
        info = one.batch_cluster_info()
        assert all(np.array_equal(info[f], info_b[f]) for f in info_b) and np.array_equal(one.batch_cluster_labels(), labels_b)
        for getter in others:  # the six existing count / info getters
            _state(getter)

    clustered_batch()
    _same_batch([one.localize_clustered(xyzs[0], n0[0], ws[0], _cps([s0["cp"]])[0], **skw)], [want_s], "single clustered")
    assert np.array_equal(one.cluster_info()["n_voxels"], info_s["n_voxels"])
    _state(one.batch_cluster_info, "agh_get_batch_cluster_info")
    _state(one.batch_cluster_labels, "agh_get_batch_cluster_labels")
    _same_batch(one.localize_batch_labeled(xyzs, n0, ws, raw, [2, 2, 2], **lkw), want_l, "labelled batch")
    assert np.array_equal(one.batch_label_counts(), counts_l)
    _state(one.batch_cluster_info)
    _state(one.batch_cluster_labels)
    _state(one.cluster_info)
    clustered_batch()
    one.close()
    fresh.close()
    from agile_grasp_amd import binding

    none = binding.Context(np.zeros((2, 3)))  # (no chain collected at all)
    _state(none.batch_cluster_info, "agh_get_batch_cluster_info")
    _state(lambda: none.batch_cluster_labels(cap=16), "agh_get_batch_cluster_labels")
    none.close()


def test_refusals(svm_model):
    """Rule 4 of the contract: AGH_ERR_INVALID_ARGUMENT with the text naming the capture and the field, nothing launched."""
    from agile_grasp_amd import binding

    scenes = B.table_scenes()
    one, ref = _contexts(scenes[0]["origins"], svm_model)
    want = _table_call(ref, scenes, "classified")
    got = _table_call(one, scenes, "classified")
    sizes = one.batch_cluster_info()["n_voxels"]
    stats = one.grid_stats()
    bad, cap = binding.AGH_ERR_INVALID_ARGUMENT, binding.AGH_ERR_CAPACITY
    xyzs, n0, ws = [np.array(s["xyz"]) for s in scenes], [s["size_left"] for s in scenes], [s["ws"] for s in scenes]
    base = [s["cp"] for s in scenes]
    caps, dcps = _depth_batch(scenes)

    def points(k=None, cp=None, **over):
        fields = [dict(f, **(cp or {})) if q == k else f for q, f in enumerate(base)]
        return one.localize_batch_clustered(xyzs, n0, ws, _cps(fields), **dict(_table_kw(scenes, "classified"), **over))

    def depth(k=None, cp=None, **over):
        fields = [dict(f, **(cp or {})) if q == k else f for q, f in enumerate(dcps)]
        return one.localize_depth_batch_clustered(caps, ws[:2], _cps(fields), **dict(KW, n_samples=10, **over))

    twelve = B.args(B.small_batch(23))
    per = lambda k, v, d: [v if q == k else d for q in range(3)]
    calls = [
        ("cp is NULL", lambda: one.localize_batch_clustered(xyzs, n0, ws, None, **_table_kw(scenes, "classified"))),
        ("cp is NULL", lambda: one.localize_depth_batch_clustered(caps, ws[:2], None, **KW)),
        ("capture 1: plane[1] is not finite", lambda: points(1, dict(plane=(0.0, np.nan, 1.0, 0.1)))),
        ("capture 2: plane[3] is not finite", lambda: points(2, dict(plane=(0.0, 0.0, 1.0, np.inf)))),
        ("capture 0: min_height is not finite", lambda: points(0, dict(min_height=-np.inf))),
        ("capture 1: max_height is not finite", lambda: depth(1, dict(max_height=np.nan))),
        ("capture 2: tolerance is not finite", lambda: points(2, dict(tolerance=np.nan))),
        ("capture 1: plane: (a, b, c) must be a unit vector", lambda: points(1, dict(plane=(0.0, 0.0, 1.0 + 2e-6, 0.1)))),
        ("capture 0: plane: (a, b, c) must be a unit vector", lambda: depth(0, dict(plane=(0.0, 0.6, 0.7, 0.1)))),
        ("capture 2: min_height must be below max_height", lambda: points(2, dict(min_height=0.5, max_height=0.5))),
        ("capture 1: tolerance must be in (0, 0.05]", lambda: points(1, dict(tolerance=0.0))),
        ("capture 1: tolerance must be in (0, 0.05]", lambda: depth(1, dict(tolerance=0.0500001))),
        ("capture 2: min_voxels must be >= 1", lambda: points(2, dict(min_voxels=0))),
        ("capture 0: max_objects must be 1 .. 64", lambda: points(0, dict(max_objects=0))),
        ("capture 1: max_objects must be 1 .. 64", lambda: depth(1, dict(max_objects=65))),
        ("capture 2: more than 64 lists in all", lambda: points(2, dict(max_objects=58))),  # 4 + 3 + 58
        ("capture 11: more than 64 lists in all",  # the twelve cases with seventy_components at 23: L = 65
         lambda: one.localize_batch_clustered(twelve["captures"], twelve["sizes_left"], twelve["workspaces"], _cps(twelve["cp"]),
                                              n_samples=7, classify=False, dense=twelve["dense"], cell_size=twelve["cell"])),
        ("capture 1: more than 2^24 samples in all",  # 32 x 2^19 = 2^24 is the limit itself; capture 1's 3 x 1 go beyond it
         lambda: points(0, dict(max_objects=32), n_samples=[1 << 19, 1, 1], caps=(1, 1, 1))),
        ("capture 1: sample_idx must be NULL", lambda: points(samples=[None, np.arange(10, dtype=np.int32), None])),
        ("capture 0: sample_idx must be NULL", lambda: depth(samples=[np.arange(10, dtype=np.int32), None])),
        # the unclustered batch twin's validations
        ("bad arguments for capture 2", lambda: points(n_samples=[10, 10, -1])),
        ("must be equal across the batch (capture 1 differs", lambda: _unequal(one, xyzs, n0, ws, base)),
        ("1 <= n_captures <= 64", lambda: one.localize_batch_clustered([], [], [], [], n_samples=10)),
    ]
    for what, call in calls:
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == bad and what in str(e.value) and "agh_localize" in str(e.value), (what, str(e.value))
        # nothing queued, nothing launched, nothing bound or changed
        _state(one.localize_batch_end)
        assert one.grid_stats() == stats, what
        assert np.array_equal(one.batch_cluster_info()["n_voxels"], sizes), what
    # a camera-origin table needs n_captures rows: origins are per capture, not per list
    o = np.asarray(scenes[0]["origins"], np.float64)
    one.set_cloud_cam_origins(np.stack([o] * 12))  # (a row per LIST is refused)
    with pytest.raises(binding.AghError) as e:
        points()
    assert e.value.code == bad and "12 rows" in str(e.value) and "3 clouds" in str(e.value)
    one.set_cloud_cam_origins(None)
    assert one.grid_stats() == stats
    plain = binding.Context(scenes[0]["origins"])
    with pytest.raises(binding.AghError) as e:
        _table_call(plain, scenes, "classified")
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    # buffers that are too small: every results[l] filled, and the repeat sized from them succeeds
    with pytest.raises(binding.AghError) as e:
        points(caps=(1, 1, 1))
    assert e.value.code == cap and "agh_localize_batch_clustered" in str(e.value)
    counts = one.last_batch_counts
    flat = [g for objs in want for g in objs]
    assert len(counts) == 12 and [r["n_hypotheses"] for r in counts] == [g["n_hypotheses"] for g in flat]
    assert [r["first_sample"] for r in counts] == np.concatenate([[0], np.cumsum([60] * 4 + [45] * 3 + [60] * 5)])[:-1].tolist()
    sized = (sum(r["n_handles"] for r in counts), sum(r["n_inlier_idx"] for r in counts), sum(r["n_hands"] for r in counts))
    _same_batch(points(caps=sized), want, "sized from the counts")
    for kw in (dict(cap_captures=2), dict(cap_lists=11)):
        with pytest.raises(binding.AghError) as e:
            one.batch_cluster_info(**kw)
        assert e.value.code == cap
    with pytest.raises(binding.AghError) as e:
        one.batch_cluster_labels(cap=10)
    assert e.value.code == cap
    _same_batch(got, want, "the first call")
    one.close()
    ref.close()


def _unequal(ctx, xyzs, n0, ws, base):
    """min_inliers differs in capture 1: through the raw records, which the binding fills with one value"""
    a = ctx._batch_cluster_lists(ctx._batch_masked_args(xyzs, n0, ws, None, dict(KW, n_samples=10, dense=True)), _cps(base))
    a["lps"][1].min_inliers = 3
    import ctypes as C

    return ctx._batch_labeled_collect(a, None, lambda *out: ctx.lib.agh_localize_batch_clustered(
        ctx._h, a["ptrs"], a["strides"], a["ns"], a["cps"], a["lps"], C.c_int32(a["n_captures"]), *out))
