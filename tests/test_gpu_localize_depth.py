"""agh_localize_depth* and agh_deproject (include/agh.h): the localize chain straight from depth images.  k_deproject is held
against the float32 model of tests/depth_captures.py bit for bit; every chain result is held, by exact equality, against
agh_localize on the model's points (stride 12, size_left = W0 x H0, dense = 1) on a second context."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_captures as D
from tests.test_depth_captures import samples_for
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
CASES = D.edge_cases()


def _bits(a):
    """the uint32 view with every NaN made one value"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


@pytest.fixture(scope="module")
def main():
    """the main case, its model points and the explicit sample list (read-only)"""
    images, ws, origins = D.main_case()
    pts = D.deproject_ref(images)
    pts.setflags(write=False)
    vox = D.voxel_model(pts, D.image_index(images), ws)
    return dict(images=images, ws=ws, origins=origins, pts=pts, size_left=images[0]["data"].size, vox=vox,
                samples=samples_for(len(vox[0])))


def _shifted(images, k):
    """another capture of the same layout: every reading 4 k mm further away"""
    out = []
    for im in images:
        d = im["data"]
        wide = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
        wide[:, :d.shape[1]] = np.where(d > 0, d + 4 * k, 0)
        out.append(dict(im, data=wide[:, :d.shape[1]]))
    return out


def _points_call(ctx, images, ws, **kw):
    pts = D.deproject_ref(images)
    return ctx.localize(pts, images[0]["data"].size, ws, dense=True, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_deprojection_equals_the_float32_model(name):
    from agile_grasp_amd import binding

    images = CASES[name]
    ctx = binding.Context(np.zeros((2, 3)))
    got = ctx.deproject(images)
    want = D.deproject_ref(images)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    diff = _bits(got) != _bits(want)
    print(name, "points", len(want), "differing words", int(diff.sum()))
    assert not diff.any()
    small = np.zeros((max(len(want) - 1, 1), 3), np.float32)
    rc = ctx.lib.agh_deproject(ctx._h, binding.depth_image_records(images)[0], C.c_int32(len(images)),
                               small.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(len(want) - 1))
    assert rc == binding.AGH_ERR_CAPACITY
    ctx.close()


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("name", ["u16_odd_stride", "f32_padded", "f32_special_unaligned", "total_1025", "u16_63x3", "main"])
def test_device_images_are_read_in_place_with_their_strides(name, offset, svm_model):
    """agh_localize_depth_device on padded device rows (unaligned ones among them) that start `offset` elements into an
    allocation, so that the base is aligned to the element only: the context's cloud afterwards is the voxelised model of the
    same images -- k_deproject read the right pixels."""
    import torch

    from agile_grasp_amd import binding

    images = CASES[name]
    dev = []
    for im in images:
        d = im["data"]
        full = np.full((d.shape[0], d.strides[0] // d.itemsize), 9, d.dtype)
        full[:, :d.shape[1]] = d
        flat = np.concatenate([np.full(offset, 9, d.dtype), full.reshape(-1)])
        t = torch.from_numpy(flat.view(np.int16) if d.dtype == np.uint16 else flat).cuda()
        view = t[offset:].view(full.shape)[:, :d.shape[1]]
        dev.append(dict(im, data=view, keep=t))
        assert view.stride(0) * d.itemsize == d.strides[0] and view.data_ptr() == t.data_ptr() + offset * d.itemsize
    pts = D.deproject_ref(images)
    fin = pts[np.isfinite(pts).all(1)]
    ws = np.array([fin[:, 0].min(), fin[:, 0].max(), fin[:, 1].min(), fin[:, 1].max(), fin[:, 2].min(), fin[:, 2].max()], np.float64)
    ctx = binding.Context(np.zeros((2, 3)))
    got = ctx.localize_depth(dev, ws, n_samples=0, classify=False)
    vox, cam = D.voxel_model(pts, D.image_index(images), ws)
    assert got["n_voxels"] == len(vox)
    gx, gc = ctx.cloud()
    assert np.array_equal(gx, vox) and np.array_equal(gc, cam)
    ctx.close()


@pytest.mark.parametrize("mode", ["explicit", "drawn", "boundaries", "one_image", "unclassified"])
def test_depth_chain_equals_points_chain(svm_model, main, mode):
    images, ws = main["images"], main["ws"]
    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW)
    if mode == "explicit":
        kw.update(samples=main["samples"])
    elif mode == "drawn":
        kw.update(n_samples=500, sample_seed=9)
    elif mode == "boundaries":
        ws = ws.copy()
        ws[1] = 0.5 * (ws[0] + ws[1])  # a face through the scene: the filter bites
        kw.update(n_samples=600, sample_seed=3, filters_boundaries=True)
    elif mode == "one_image":
        images = images[:1]
        kw.update(n_samples=300, sample_seed=4)
    else:
        kw.update(samples=main["samples"], classify=False)
    want = _points_call(ref, images, ws, **kw)
    got = one.localize_depth(images, ws, **kw)
    print(mode, "voxels", want["n_voxels"], "hypotheses", want["n_hypotheses"], "hands", len(want["hands"]), "handles", len(want["handles"]))
    assert want["n_hypotheses"] >= 20
    if mode in ("explicit", "unclassified"):
        assert len(want["hands"]) >= 1
    if mode == "unclassified":
        assert len(want["handles"]) >= 1
    _same(got, want, mode)
    gx, gc = one.cloud()
    rx, rc = ref.cloud()
    assert np.array_equal(gx, rx) and np.array_equal(gc, rc)
    if mode == "boundaries":
        plain = one.localize_depth(images, ws, **dict(kw, filters_boundaries=False))
        assert len(plain["hands"]) >= len(got["hands"]) and plain["n_hypotheses"] == got["n_hypotheses"]


def test_voxelised_cloud_keeps_the_image_index_as_camera_id(svm_model, main):
    (one,) = _contexts(main["origins"], svm_model, n=1)
    got = one.localize_depth(main["images"], main["ws"], samples=main["samples"], **KW)
    vox, cam = main["vox"]
    assert got["n_voxels"] == len(vox)
    gx, gc = one.cloud()
    assert np.array_equal(gx, vox) and np.array_equal(gc, cam)
    assert np.bincount(gc, minlength=2).min() > 1000


def test_device_form_equals_host_form(svm_model, main):
    import torch

    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, samples=main["samples"])
    want = ref.localize_depth(main["images"], main["ws"], **kw)
    dev = [dict(im, data=torch.from_numpy(np.ascontiguousarray(im["data"]).view(np.int16)).cuda()) for im in main["images"]]
    _same(one.localize_depth(dev, main["ws"], **kw), want, "device")
    assert len(want["hands"]) >= 1


def test_staged_stream_equals_blocking_calls(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    caps = [_shifted(main["images"], k) for k in range(3)]
    kws = [dict(KW, n_samples=300 + 50 * k, sample_seed=k + 1) for k in range(3)]
    want = [ref.localize_depth(caps[k], main["ws"], **kws[k]) for k in range(3)]
    assert all(w["n_hypotheses"] >= 20 for w in want)
    one.localize_depth_begin(caps[0], main["ws"], **kws[0])
    one.localize_depth_stage(caps[1])
    _same(one.localize_end(), want[0], "capture 0")
    one.localize_depth_begin(caps[1], main["ws"], **kws[1])  # adopted: same pixel arrays
    one.localize_depth_stage(caps[2])
    _same(one.localize_end(), want[1], "capture 1")
    saved = [im["data"].copy() for im in caps[2]]
    for im in caps[2]:
        im["data"][:] = 0  # (pageable images have been read when the stage call returns; an adopted set is not read again)
    one.localize_depth_begin(caps[2], main["ws"], **kws[2])
    _same(one.localize_end(), want[2], "capture 2")
    for im, d in zip(caps[2], saved):
        im["data"][:] = d
    # a staged set the next begin does not name (a copy of the pixels is another capture) is dropped
    one.localize_depth_stage(caps[1])
    other = [dict(im, data=np.array(im["data"])) for im in caps[0]]
    one.localize_depth_begin(other, main["ws"], **kws[0])
    _same(one.localize_end(), want[0], "not adopted")
    # one staged set of any kind: a newer stage replaces an older one
    one.localize_depth_stage(caps[0])
    one.localize_depth_stage(caps[2])
    one.localize_depth_begin(caps[2], main["ws"], **kws[2])
    _same(one.localize_end(), want[2], "replaced")


def test_staged_sets_of_the_other_kind_are_dropped(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    images, ws = main["images"], main["ws"]
    kw = dict(KW, n_samples=300, sample_seed=2)
    pts = np.array(main["pts"])
    want_depth = ref.localize_depth(images, ws, **kw)
    want_pts = ref.localize(pts, main["size_left"], ws, dense=True, **kw)
    _same(want_depth, want_pts, "the two kinds")
    staged = one.localize_stage(pts)  # points staged, depth begun
    one.localize_depth_begin(images, ws, **kw)
    _same(one.localize_end(), want_depth, "points stage, depth begin")
    one.localize_depth_stage(images)  # depth staged, points begun
    one.localize_begin(staged, main["size_left"], ws, dense=True, **kw)
    _same(one.localize_end(), want_pts, "depth stage, points begin")
    # ... and each kind still adopts its own
    one.localize_depth_stage(images)
    one.localize_depth_begin(images, ws, **kw)
    _same(one.localize_end(), want_depth, "depth stage, depth begin")
    staged = one.localize_stage(pts)
    one.localize_begin(staged, main["size_left"], ws, dense=True, **kw)
    _same(one.localize_end(), want_pts, "points stage, points begin")


def test_the_outgrown_bitmap_repeat_inside_a_depth_call(svm_model, main):
    """A small-extent capture sizes the context's voxel bitmap; the wide one's lattice outgrows it, and the chain is run once
    more inside the call, from the points k_deproject left in the raw buffer."""
    one, ref, fresh = _contexts(main["origins"], svm_model, n=3)
    images, ws = main["images"], main["ws"]
    kw = dict(KW, n_samples=300, sample_seed=6)
    mid = 0.5 * (ws[0::2] + ws[1::2])
    half = 0.08 * (ws[1::2] - ws[0::2])
    small = np.stack([mid - half, mid + half], axis=1).reshape(6)
    want_small = ref.localize_depth(images, small, **kw)
    assert want_small["n_voxels"] > 100
    _same(one.localize_depth(images, small, **kw), want_small, "small extent")
    builds = one.grid_stats()["builds"]
    got = one.localize_depth(images, ws, **kw)
    print("grid builds of the wide call", one.grid_stats()["builds"] - builds)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the chain twice: the lattice outgrew the kept bitmap)
    _same(got, fresh.localize_depth(images, ws, **kw), "wide extent")
    assert got["n_hypotheses"] >= 20


def test_points_call_after_a_depth_call_shares_the_raw_buffer_safely(svm_model, main):
    from agile_grasp_amd import synthetic

    one, fresh = _contexts(main["origins"], svm_model)
    one.localize_depth(main["images"], main["ws"], samples=main["samples"], **KW)
    raw = synthetic.make_raw_cloud(60_000, 300)
    kw = dict(KW, n_samples=200, sample_seed=5)
    want = fresh.localize(raw.xyz, raw.size_left, raw.workspace, **kw)
    _same(one.localize(raw.xyz, raw.size_left, raw.workspace, **kw), want, "points after depth")
    assert want["n_hypotheses"] > 0
    # ... and a depth call after a larger points call
    _same(one.localize_depth(main["images"], main["ws"], samples=main["samples"], **KW),
          fresh.localize_depth(main["images"], main["ws"], samples=main["samples"], **KW), "depth after points")


def test_refusals(svm_model, main):
    from agile_grasp_amd import binding

    one, ref = _contexts(main["origins"], svm_model)
    images, ws = main["images"], main["ws"]
    kw = dict(KW, n_samples=200, sample_seed=8)
    want = ref.localize_depth(images, ws, **kw)
    lp, _, S, hcap = one._localize_params(0, ws, None, 200, 8, True, 2, 0.005, 0.003, False, False)
    out = np.zeros((sum(im["data"].size for im in images), 3), np.float32)
    bad = binding.AGH_ERR_INVALID_ARGUMENT

    def check(field, k, mutate, n=2, only=None):
        recs = binding.depth_image_records(images)[0]
        if mutate:
            mutate(recs[k])
        h, idx, hands, sout = one._loc_bufs
        res = binding.AghLocalizeResult()
        outs = (h.ctypes.data_as(C.c_void_p), C.c_int64(hcap), idx.ctypes.data_as(C.c_void_p), C.c_int64(hcap),
                hands.ctypes.data_as(C.c_void_p), C.c_int64(hcap), sout.ctypes.data_as(C.c_void_p), C.byref(res))
        nn = C.c_int32(n)
        fns = {"agh_deproject": lambda: one.lib.agh_deproject(one._h, recs, nn, out.ctypes.data_as(C.c_void_p), C.c_int64(len(out))),
               "agh_localize_depth": lambda: one.lib.agh_localize_depth(one._h, recs, nn, C.byref(lp), *outs),
               "agh_localize_depth_device": lambda: one.lib.agh_localize_depth_device(one._h, recs, nn, C.byref(lp), *outs),
               "agh_localize_depth_begin": lambda: one.lib.agh_localize_depth_begin(one._h, recs, nn, C.byref(lp)),
               "agh_localize_depth_stage": lambda: one.lib.agh_localize_depth_stage(one._h, recs, nn)}
        for name in only or fns:
            rc = fns[name]()
            text = one.lib.agh_last_error(one._h).decode()
            assert rc == bad, (field, name, rc, text)
            assert text.startswith(name + ": ") and field in text, (field, name, text)
            if k is not None:
                assert f"image {k}" in text, (field, name, text)
            # the context still works, and nothing was queued or staged: a chain, and a stream that adopts its own staged set
            with pytest.raises(binding.AghError) as e:
                one.localize_end()
            assert e.value.code == binding.AGH_ERR_STATE
            _same(one.localize_depth(images, ws, **kw), want, f"after {name} refused {field}")

    def setter(name, value):
        return lambda r: setattr(r, name, value)

    def pose_nan(r):
        r.pose[7] = float("inf")

    nan, inf = float("nan"), float("inf")
    check("n_images", None, None, n=0)
    check("n_images", None, None, n=3)
    check("data", 1, setter("data", None))
    for field, values in (("width", (0, 8193)), ("height", (0, -4, 8193)), ("format", (2, -1)),
                          ("row_stride_bytes", (2 * D.MAIN_W - 2, 2 * D.MAIN_W + 1)), ("fx", (0.0, nan, inf)), ("fy", (0.0, -inf)),
                          ("cx", (nan,)), ("cy", (inf,)), ("depth_scale", (0.0, -0.001, nan, inf))):
        for k, v in enumerate(values):
            check(field, k % 2, setter(field, v))
    check("pose", 0, pose_nan)

    def odd(r):  # a device image is read in place, an element at a time at the least: an odd pointer is refused
        r.data += 1

    check("data", 1, odd, only=("agh_localize_depth_device",))
    h, idx, hands, sout = one._loc_bufs
    res = binding.AghLocalizeResult()
    rc = one.lib.agh_localize_depth(one._h, None, C.c_int32(2), C.byref(lp), h.ctypes.data_as(C.c_void_p), C.c_int64(hcap),
                                    idx.ctypes.data_as(C.c_void_p), C.c_int64(hcap), hands.ctypes.data_as(C.c_void_p), C.c_int64(hcap),
                                    sout.ctypes.data_as(C.c_void_p), C.byref(res))
    assert rc == bad and "images" in one.lib.agh_last_error(one._h).decode()
    # nothing was queued or staged by any of them
    with pytest.raises(binding.AghError) as e:
        one.localize_end()
    assert e.value.code == binding.AGH_ERR_STATE
    _same(one.localize_depth(images, ws, **kw), want, "after the refusals")
    # mid-chain: AGH_ERR_STATE, the chain untouched
    one.localize_depth_begin(images, ws, **kw)
    keep = one._loc_keep
    for name, call in (("agh_deproject", lambda: one.deproject(images)), ("agh_localize_depth", lambda: one.localize_depth(images, ws, **kw)),
                       ("agh_localize_depth_begin", lambda: one.localize_depth_begin(images, ws, **kw)),
                       ("agh_localize_begin", lambda: one.localize(np.array(main["pts"]), 1, ws, n_samples=8))):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE and name + ": " in str(e.value), (name, str(e.value))
        one._loc_keep = keep
    _same(one.localize_end(), want, "after the mid-chain refusals")
    # a camera-origin table must have one row
    one.set_cloud_cam_origins(np.zeros((2, 2, 3)))
    with pytest.raises(binding.AghError) as e:
        one.localize_depth(images, ws, **kw)
    assert e.value.code == bad
    one.set_cloud_cam_origins(None)
    # classification without an SVM
    plain = binding.Context(main["origins"])
    with pytest.raises(binding.AghError) as e:
        plain.localize_depth(images, ws, **kw)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    _same(plain.localize_depth(images, ws, **dict(kw, classify=False)), ref.localize_depth(images, ws, **dict(kw, classify=False)),
          "after AGH_ERR_NO_SVM")
    plain.close()
    _same(one.localize_depth(images, ws, **kw), want, "at the end")
