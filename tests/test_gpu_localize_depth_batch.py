"""agh_localize_depth_batch* and agh_deproject_batch (include/agh.h): depth captures through the batch chain.
k_deproject_batch is held against the float32 model of tests/depth_captures.py word for word; every chain result is held, by
exact equality, against agh_localize_depth per capture on a second context (and once against agh_localize_batch on the model's
points)."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_batch_captures as DB
from tests import depth_captures as D
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same
from tests.test_gpu_localize_depth import _bits

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)


@pytest.fixture(scope="module")
def main():
    """main_batch with each capture's voxel model and explicit sample list (read-only)"""
    caps, ws, origins = DB.main_batch()
    vox = [DB.voxels_of(c, ws) for c in caps]
    return dict(caps=caps, ws=ws, origins=origins, vox=vox, samples=[DB.samples_for(k, len(v[0])) for k, v in enumerate(vox)])


def _singles(ref, caps, ws_list, kws):
    """agh_localize_depth, capture after capture"""
    return [ref.localize_depth(c, ws, **kw) for c, ws, kw in zip(caps, ws_list, kws)]


def _spans_consistent(counts):
    h = i = k = 0
    for c in counts:
        assert (c["first_handle"], c["first_inlier_idx"], c["first_hand"]) == (h, i, k)
        h, i, k = h + c["n_handles"], i + c["n_inlier_idx"], k + c["n_hands"]


def _floors(want):
    """the floors of tests/test_depth_batch_captures.py on the reference context's results"""
    assert all(w["n_hypotheses"] >= 20 for w in want), [w["n_hypotheses"] for w in want]


@pytest.mark.parametrize("name", ["edge", "max_views", "one"])
def test_kernel_equals_the_float32_model(name):
    from agile_grasp_amd import binding

    caps = {"edge": DB.edge_batch, "max_views": DB.max_views, "one": lambda: [D.edge_cases()["total_1025"]]}[name]()
    ctx = binding.Context(np.zeros((2, 3)))
    got = ctx.deproject_batch(caps)
    want = DB.deproject_ref(caps)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    diff = _bits(got) != _bits(want)
    print(name, "captures", len(caps), "points", len(want), "differing words", int(diff.sum()))
    assert not diff.any()
    recs, n_images, _keep, _ = ctx.depth_batch_records(caps)
    small = np.zeros((len(want), 3), np.float32)
    rc = ctx.lib.agh_deproject_batch(ctx._h, recs, n_images, C.c_int32(len(caps)), small.ctypes.data_as(C.POINTER(C.c_float)),
                                     C.c_int64(len(want) - 1))
    assert rc == binding.AGH_ERR_CAPACITY
    assert np.array_equal(_bits(ctx.deproject_batch(caps)), _bits(want))  # ... and the context still works
    ctx.close()


@pytest.mark.parametrize("mode", ["explicit", "drawn", "boundaries", "unclassified"])
def test_batch_equals_single_calls(svm_model, main, mode):
    caps, ws = main["caps"], main["ws"]
    one, ref = _contexts(main["origins"], svm_model)
    n = len(caps)
    kw = dict(KW)
    if mode == "explicit":
        kw.update(samples=main["samples"])
        kws = [dict(KW, samples=s) for s in main["samples"]]
    elif mode == "drawn":
        kw.update(n_samples=[200 + 20 * k for k in range(n)], sample_seeds=[7 + k for k in range(n)])
        kws = [dict(KW, n_samples=200 + 20 * k, sample_seed=7 + k) for k in range(n)]
    elif mode == "boundaries":
        ws = ws.copy()
        ws[1] = 0.5 * (ws[0] + ws[1])  # a face through the scene: the filter bites
        kw.update(n_samples=300, sample_seeds=[3 + k for k in range(n)], filters_boundaries=True)
        kws = [dict(KW, n_samples=300, sample_seed=3 + k, filters_boundaries=True) for k in range(n)]
    else:
        kw.update(samples=main["samples"], classify=False)
        kws = [dict(KW, samples=s, classify=False) for s in main["samples"]]
    want = _singles(ref, caps, [ws] * n, kws)
    got = one.localize_depth_batch(caps, ws, **kw)
    print(mode, [(w["n_voxels"], w["n_hypotheses"], len(w["hands"]), len(w["handles"])) for w in want])
    _floors(want)
    if mode == "unclassified":
        assert sum(len(w["handles"]) for w in want) >= 1
    assert len(got) == n
    for k in range(n):
        _same(got[k], want[k], f"{mode}, capture {k}")
    _spans_consistent(one.last_batch_counts)
    assert [c["first_sample"] for c in one.last_batch_counts] == list(np.cumsum([0] + [len(w["samples"]) for w in want])[:-1])
    if mode == "boundaries":
        plain = one.localize_depth_batch(caps, ws, **dict(kw, filters_boundaries=False))
        assert sum(len(p["hands"]) for p in plain) > sum(len(g["hands"]) for g in got)
        assert [p["n_hypotheses"] for p in plain] == [g["n_hypotheses"] for g in got]
    if mode == "explicit":
        # ... and agh_localize_batch on the model's points: stride 12, size_left = W0 x H0, dense = 1
        pts = [D.deproject_ref(c) for c in caps]
        by_points = ref.localize_batch(pts, [c[0]["data"].size for c in caps], ws, samples=main["samples"], dense=True, **KW)
        for k in range(n):
            _same(got[k], by_points[k], f"points batch, capture {k}")


def test_bound_batch_afterwards_is_the_voxelised_batch(svm_model, main):
    (one,) = _contexts(main["origins"], svm_model, n=1)
    got = one.localize_depth_batch(main["caps"], main["ws"], samples=main["samples"], **KW)
    assert [g["n_voxels"] for g in got] == [len(v[0]) for v in main["vox"]]
    gx, gc = one.cloud()
    assert np.array_equal(gx, np.concatenate([v[0] for v in main["vox"]]))
    assert np.array_equal(gc, np.concatenate([v[1] for v in main["vox"]]))
    for c, (_, cam) in zip(main["caps"], main["vox"]):
        if len(c) == 2:
            assert np.bincount(cam, minlength=2).min() > 1000  # both ids present
        else:
            assert not cam.any()


def _on_device(images, offset):
    """the images in device memory, rows with their padding, the base `offset` elements into an allocation"""
    import torch

    out = []
    for im in images:
        d = im["data"]
        full = np.full((d.shape[0], d.strides[0] // d.itemsize), 9, d.dtype)
        full[:, :d.shape[1]] = d
        flat = np.concatenate([np.full(offset, 9, d.dtype), full.reshape(-1)])
        t = torch.from_numpy(flat.view(np.int16) if d.dtype == np.uint16 else flat).cuda()
        view = t[offset:].view(full.shape)[:, :d.shape[1]]
        assert view.stride(0) * d.itemsize == d.strides[0] and view.data_ptr() == t.data_ptr() + offset * d.itemsize
        out.append(dict(im, data=view, keep=t))
    return out


def test_device_form_equals_host_form(svm_model, main):
    """Device images are read in place with their strides: padded rows (image 1's stride is an odd number of uint16 elements),
    bases 1 and 3 elements into their allocations, both formats, a capture of one image."""
    one, ref = _contexts(main["origins"], svm_model)
    pick = [0, 1, 4, 5]
    caps = [main["caps"][k] for k in pick]
    strides = [im["data"].strides[0] // im["data"].itemsize for c in caps for im in c]
    assert all(s > D.MAIN_W for s in strides) and any(s % 2 == 1 for s in strides)
    dev = [_on_device(c, (1, 3, 3, 1)[j]) for j, c in enumerate(caps)]
    kw = dict(KW, samples=[main["samples"][k] for k in pick])
    want = ref.localize_depth_batch(caps, main["ws"], **kw)
    got = one.localize_depth_batch(dev, main["ws"], **kw)
    for j in range(len(pick)):
        _same(got[j], want[j], f"device, capture {pick[j]}")
    _floors(want)
    gx, gc = one.cloud()
    assert np.array_equal(gx, np.concatenate([main["vox"][k][0] for k in pick]))
    assert np.array_equal(gc, np.concatenate([main["vox"][k][1] for k in pick]))
    # ... and through the two halves
    one.localize_depth_batch_begin(dev, main["ws"], **kw)
    got = one.localize_batch_end()
    for j in range(len(pick)):
        _same(got[j], want[j], f"device begin + end, capture {pick[j]}")


def test_begin_and_end_equal_the_blocking_call_and_staged_sets_are_dropped(svm_model, main):
    from agile_grasp_amd import synthetic

    one, ref = _contexts(main["origins"], svm_model)
    caps, ws = main["caps"][:3], main["ws"]
    kw = dict(KW, n_samples=[200, 220, 240], sample_seeds=[1, 2, 3])
    want = ref.localize_depth_batch(caps, ws, **kw)
    _floors(want)
    singles = _singles(ref, caps, [ws] * 3, [dict(KW, n_samples=200 + 20 * k, sample_seed=1 + k) for k in range(3)])

    def begin_end(what):
        one.localize_depth_batch_begin(caps, ws, **kw)
        got = one.localize_batch_end()
        for k in range(3):
            _same(got[k], want[k], f"{what}, capture {k}")
            _same(got[k], singles[k], f"{what}, capture {k} against the single call")
        _spans_consistent(one.last_batch_counts)

    begin_end("begin + end")
    # a pending staged set of each kind is dropped by the depth-batch begin
    pts = [D.deproject_ref(c) for c in main["caps"][3:5]]
    one.localize_stage(pts[0])
    begin_end("after agh_localize_stage")
    one.localize_depth_stage(main["caps"][3])
    begin_end("after agh_localize_depth_stage")
    one.localize_batch_stage(pts)
    begin_end("after agh_localize_batch_stage")
    # ... and dropped it is: the next points batch of the same arrays is uploaded and right
    sizes = [c[0]["data"].size for c in main["caps"][3:5]]
    pkw = dict(KW, n_samples=150, sample_seeds=[4, 5], dense=True)
    want_pts = ref.localize_batch(pts, sizes, ws, **pkw)
    got_pts = one.localize_batch(pts, sizes, ws, **pkw)
    for k in range(2):
        _same(got_pts[k], want_pts[k], f"points batch after a depth batch, capture {k}")
    assert all(w["n_hypotheses"] >= 20 for w in want_pts)
    begin_end("depth batch after a points batch")
    # a larger points batch (the raw buffer grows), then the depth batch again
    raw = synthetic.make_raw_cloud(600_000, 300)
    big = ref.localize(raw.xyz, raw.size_left, raw.workspace, n_samples=100, sample_seed=5, **KW)
    _same(one.localize_batch([raw.xyz], raw.size_left, raw.workspace, n_samples=100, sample_seeds=[5], **KW)[0], big, "large points batch")
    begin_end("depth batch after a larger points batch")


def test_the_outgrown_bitmap_repeat_inside_a_depth_batch(svm_model, main):
    """A small-extent batch sizes the context's bitmap slots; the wide one's lattices outgrow them, and the batch is run once
    more inside the call, from the points k_deproject_batch left in the raw buffer."""
    one, ref, fresh = _contexts(main["origins"], svm_model, n=3)
    caps, ws = main["caps"][:3], main["ws"]
    kw = dict(KW, n_samples=200, sample_seeds=[6, 7, 8])
    mid = 0.5 * (ws[0::2] + ws[1::2])
    half = 0.08 * (ws[1::2] - ws[0::2])
    small = np.stack([mid - half, mid + half], axis=1).reshape(6)
    want_small = ref.localize_depth_batch(caps, small, **kw)
    assert all(w["n_voxels"] > 100 for w in want_small)
    got = one.localize_depth_batch(caps, small, **kw)
    for k in range(3):
        _same(got[k], want_small[k], f"small extent, capture {k}")
    builds = one.grid_stats()["builds"]
    got = one.localize_depth_batch(caps, ws, **kw)
    print("grid builds of the wide call", one.grid_stats()["builds"] - builds)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the batch twice: the lattices outgrew the kept slots)
    want = fresh.localize_depth_batch(caps, ws, **kw)
    singles = _singles(ref, caps, [ws] * 3, [dict(KW, n_samples=200, sample_seed=6 + k) for k in range(3)])
    for k in range(3):
        _same(got[k], want[k], f"wide extent, capture {k}")
        _same(got[k], singles[k], f"wide extent, capture {k} against the single call")
    _floors(want)


def test_per_capture_rigs(svm_model, main):
    from agile_grasp_amd import binding

    # capture k seen by a rig moved by d_k: poses, points and workspace move with it, and so must the camera origins
    shifts = [np.zeros(3), np.array([0.25, -0.1, 0.05]), np.array([-0.3, 0.2, 0.1])]
    caps, wss, tab = [], [], []
    for k, d in enumerate(shifts):
        images = []
        for im in main["caps"][k]:
            pose = np.array(im["pose"], np.float64)
            pose[:, 3] += d
            images.append(dict(im, pose=pose))
        caps.append(images)
        wss.append(main["ws"] + np.repeat(d, 2))
        tab.append(np.stack([im["pose"][:, 3] for im in images]))
    tab = np.stack(tab)
    assert not np.array_equal(tab[0], tab[1]) and not np.array_equal(tab[1], tab[2])
    (one,) = _contexts(np.zeros((2, 3)), svm_model, n=1)  # (its own origins are not any capture's)
    kw = dict(KW, n_samples=200, sample_seeds=[1, 2, 3])
    one.set_cloud_cam_origins(tab)
    got = one.localize_depth_batch(caps, np.stack(wss), **kw)
    for k in range(3):
        (ref,) = _contexts(tab[k], svm_model, n=1)
        want = ref.localize_depth(caps[k], wss[k], n_samples=200, sample_seed=1 + k, **KW)
        assert want["n_hypotheses"] >= 20
        _same(got[k], want, f"rig {k}")
        ref.close()
    one.set_cloud_cam_origins(tab[:2])  # two rows, three captures
    with pytest.raises(binding.AghError) as e:
        one.localize_depth_batch(caps, np.stack(wss), **kw)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT
    one.set_cloud_cam_origins(tab)
    _same(one.localize_depth_batch(caps, np.stack(wss), **kw)[1], got[1], "after the refusal")


def test_refusals(svm_model, main):
    from agile_grasp_amd import binding

    one, ref = _contexts(main["origins"], svm_model)
    caps, ws = main["caps"][:3], main["ws"]
    kw = dict(KW, n_samples=150, sample_seeds=[1, 2, 3])
    want = ref.localize_depth_batch(caps, ws, **kw)
    _floors(want)
    bad = binding.AGH_ERR_INVALID_ARGUMENT

    def still_works(what):
        with pytest.raises(binding.AghError) as e:  # nothing was queued
            one.localize_batch_end()
        assert e.value.code == binding.AGH_ERR_STATE, what
        got = one.localize_depth_batch(caps, ws, **kw)
        for k in range(3):
            _same(got[k], want[k], f"after {what}, capture {k}")

    def refused(what, code, text=(), n_captures=3, mutate=None, fn="agh_localize_depth_batch"):
        a = one._depth_batch_args(caps, ws, dict(kw))
        if mutate:
            mutate(a)
        with pytest.raises(binding.AghError) as e:
            one._batch_collect(a, None, lambda *out: getattr(one.lib, fn)(one._h, a["recs"], a["n_images"], a["lps"],
                                                                          C.c_int32(n_captures), *out))
        assert e.value.code == code, (what, str(e.value))
        for t in (fn + ": ",) + tuple(text):
            assert t in str(e.value), (what, t, str(e.value))
        still_works(what)

    def n_images(k, v):
        def f(a):
            a["n_images"][k] = v
        return f

    def field(j, name, v):
        def f(a):
            setattr(a["recs"][j], name, v)
        return f

    def classify_differs(a):
        a["lps"][1].classify = 0

    refused("n_images 0", bad, ("capture 1", "n_images"), mutate=n_images(1, 0))
    refused("n_images 3", bad, ("capture 2", "n_images"), mutate=n_images(2, 3))
    refused("n_captures 0", bad, ("n_captures",), n_captures=0)
    refused("n_captures 65", bad, ("n_captures",), n_captures=65)
    refused("fx", bad, ("capture 2, image 1: fx must be finite and not zero",), mutate=field(5, "fx", 0.0))
    refused("width", bad, ("capture 2, image 1: width",), mutate=field(5, "width", 8193), fn="agh_localize_depth_batch_device")
    refused("stride", bad, ("capture 0, image 1: row_stride_bytes",), mutate=field(1, "row_stride_bytes", 2 * D.MAIN_W + 1))
    refused("classify", bad, ("capture 1 differs",), mutate=classify_differs)
    # the same rules for the introspection call and the begin
    recs, nim, _keep, _ = one.depth_batch_records(caps)
    recs[5].fy = float("nan")
    out = np.zeros((sum(DB.points_of(c) for c in caps), 3), np.float32)
    assert one.lib.agh_deproject_batch(one._h, recs, nim, C.c_int32(3), out.ctypes.data_as(C.c_void_p), C.c_int64(len(out))) == bad
    assert "agh_deproject_batch: capture 2, image 1: fy" in one.lib.agh_last_error(one._h).decode()
    lps = one._depth_batch_args(caps, ws, dict(kw))["lps"]
    assert one.lib.agh_localize_depth_batch_begin(one._h, recs, nim, lps, C.c_int32(3)) == bad
    assert "agh_localize_depth_batch_begin: capture 2, image 1: fy" in one.lib.agh_last_error(one._h).decode()
    still_works("the begin and the introspection call")
    # mid-chain: AGH_ERR_STATE, the chain untouched
    one.localize_depth_batch_begin(caps, ws, **kw)
    pending = one._batch_pending
    for name, call in (("agh_localize_depth_batch", lambda: one.localize_depth_batch(caps, ws, **kw)),
                       ("agh_localize_depth_batch_begin", lambda: one.localize_depth_batch_begin(caps, ws, **kw)),
                       ("agh_deproject_batch", lambda: one.deproject_batch(caps)),
                       ("agh_localize_depth_begin", lambda: one.localize_depth_begin(caps[0], ws, n_samples=8))):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE and name + ": " in str(e.value), (name, str(e.value))
        one._batch_pending = pending
    got = one.localize_batch_end()
    for k in range(3):
        _same(got[k], want[k], f"after the mid-chain refusals, capture {k}")
    # ... and a depth batch is refused while a single chain is in flight
    one.localize_depth_begin(caps[0], ws, n_samples=150, sample_seed=1, **KW)
    with pytest.raises(binding.AghError) as e:
        one.localize_depth_batch(caps, ws, **kw)
    assert e.value.code == binding.AGH_ERR_STATE
    _same(one.localize_end(), want[0], "the single chain")
    # output buffers too small: AGH_ERR_CAPACITY with results filled; a repeat sized from them succeeds
    assert sum(len(w["handles"]) for w in want) >= 1
    with pytest.raises(binding.AghError) as e:
        one.localize_depth_batch(caps, ws, caps=(0, 0, 0), **kw)
    assert e.value.code == binding.AGH_ERR_CAPACITY
    counts = one.last_batch_counts
    assert [c["n_handles"] for c in counts] == [len(w["handles"]) for w in want]
    assert [c["n_hands"] for c in counts] == [len(w["hands"]) for w in want]
    assert [c["n_voxels"] for c in counts] == [w["n_voxels"] for w in want]
    sized = tuple(sum(c[f] for c in counts) for f in ("n_handles", "n_inlier_idx", "n_hands"))
    got = one.localize_depth_batch(caps, ws, caps=sized, **kw)
    for k in range(3):
        _same(got[k], want[k], f"sized from the counts, capture {k}")
    # classification without an SVM
    plain = binding.Context(main["origins"])
    with pytest.raises(binding.AghError) as e:
        plain.localize_depth_batch(caps, ws, **kw)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    nokw = dict(kw, classify=False)
    got, unclassified = plain.localize_depth_batch(caps, ws, **nokw), ref.localize_depth_batch(caps, ws, **nokw)
    for k in range(3):
        _same(got[k], unclassified[k], f"after AGH_ERR_NO_SVM, capture {k}")
    plain.close()
    still_works("everything")
