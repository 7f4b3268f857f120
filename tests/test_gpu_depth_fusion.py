"""agh_fuse_depth (include/agh.h, "DEPTH FUSION"): a burst of depth frames of one camera fused on the device.  k_depth_fuse is
held byte for byte -- the image (a float32 image by its uint32 view, so that NaNs compare) and the six counts -- against the numpy
model of tests/depth_fusion_cases.py at the launch's wave and row boundaries, on one image in which every pixel is a case, and in
the device form; the fused records then go through the depth chains with no synchronisation in between and must give, bit for bit
(epoch aside), what the host forms give for fused_depth()'s copies of the same slots.  The regimes are those
tests/test_depth_fusion_cases.py proves on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_captures as D
from tests import depth_fusion_cases as FU
from tests import hand_filter_cases as HF
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)


@pytest.fixture(scope="module")
def ctx():
    from agile_grasp_amd import binding

    c = binding.Context(np.zeros((2, 3)))
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain_ctx(svm_model):
    (c,) = _contexts(HF.box_scene(2)["origins"], svm_model, n=1)
    yield c
    c.close()


def _counts(ctx, slot=0):
    rec = ctx.depth_fusion_counts(slot)
    return None if rec is None else [getattr(rec, f) for f in FU.COUNT_FIELDS]


def _check(ctx, frames, fp, slot=0, what=""):
    """fuse `frames` into `slot`: the image and the counts are the model's"""
    want = FU.fuse([f["data"] for f in frames], frames[0]["depth_scale"], **fp)
    fused = ctx.fuse_depth(frames, slot=slot, **fp)
    got = ctx.fused_depth(slot)
    assert FU.same_image(got, want["image"]), (what, got, want["image"])
    assert _counts(ctx, slot) == want["counts"], (what, _counts(ctx, slot), want["counts"])
    return fused, want


def _device(frames, extra=3):
    """the frames as column slices of wider torch CUDA tensors (frame t's rows are extra + t elements longer)"""
    import torch

    out = []
    for t, f in enumerate(frames):
        d = np.asarray(f["data"])
        wide = np.full((d.shape[0], d.shape[1] + extra + t), 9, d.dtype)
        wide[:, :d.shape[1]] = d
        tt = torch.from_numpy(wide.view(np.int16) if d.dtype == np.uint16 else wide).cuda()
        out.append(dict(f, data=tt[:, :d.shape[1]], keep=tt))
    return out


@pytest.mark.parametrize("n_frames", FU.FRAME_COUNTS)
@pytest.mark.parametrize("fmt", [D.U16, D.F32], ids=["u16", "f32"])
def test_fused_image_and_counts_equal_the_model(ctx, fmt, n_frames):
    classes = np.zeros(4, np.int64)
    for k, (w, h) in enumerate(FU.SIZES):
        for pad in (0, 3):
            frames = FU.random_burst(w, h, n_frames, fmt, seed=100 * n_frames + 10 * k + pad, pad=pad)
            if pad and n_frames > 1:
                assert len({f["data"].strides[0] for f in frames}) == n_frames  # (a different row stride per frame)
            for mv in sorted({1, n_frames}):
                _, want = _check(ctx, frames, dict(min_valid=mv), what=(w, h, pad, mv))
                classes += np.array(want["counts"][1:5])
    print(np.dtype(fmt).name, n_frames, "empty, unsupported, inconsistent, fused:", classes.tolist())
    assert classes[3] > 0 and classes[0] + classes[1] + classes[2] > 0


@pytest.mark.parametrize("fmt", [D.U16, D.F32], ids=["u16", "f32"])
def test_constructed_pixels(ctx, fmt):
    frames, fp, cases = FU.constructed(fmt)
    _, want = _check(ctx, frames, fp, what="constructed")
    got = ctx.fused_depth(0)
    for name, (px, cls, value) in cases.items():
        assert want["cls"][0, px] == cls, name  # (the model's class is the one the pixel was built for; the image equals the model's)
        if cls != FU.FUSED:
            assert got[0, px] == 0 if fmt == D.U16 else np.isnan(got[0, px]), name
        elif value is not None:
            assert got[0, px] == value, (name, got[0, px], value)
    assert want["filled"][0, cases["last frame invalid"][0]] and not want["filled"][0, cases["last frame valid"][0]]
    frames, fp, value = FU.zero_spread(fmt)
    _check(ctx, frames, fp, what="zero spread")
    assert FU.same_image(ctx.fused_depth(0), value)  # (the median itself)


def test_float_sum_runs_in_frame_order(ctx):
    frames, fp, value = FU.order_of_the_sum()
    assert value[0, 0] != value[0, 1]
    _check(ctx, frames, fp, what="order")
    assert FU.same_image(ctx.fused_depth(0), value)


@pytest.mark.parametrize("fmt", [D.U16, D.F32], ids=["u16", "f32"])
def test_device_form_equals_the_host_form(ctx, fmt):
    frames = FU.random_burst(130, 7, 5, fmt, seed=5)
    fp = dict(min_valid=2)
    _, want = _check(ctx, frames, fp, slot=2, what="host")
    host = ctx.fused_depth(2)
    dev = _device(frames)
    assert len({int(f["data"].stride(0)) for f in dev}) == 5 and all(int(f["data"].stride(0)) > 130 for f in dev)
    fused = ctx.fuse_depth(dev, slot=3, **fp)
    assert FU.same_image(ctx.fused_depth(3), host) and _counts(ctx, 3) == want["counts"] == _counts(ctx, 2)
    assert fused["data"].is_cuda and fused["data"].shape == (7, 130)


def test_slots(ctx):
    from agile_grasp_amd import binding

    a = FU.random_burst(65, 3, 4, D.U16, seed=1)
    b = FU.random_burst(64, 1, 3, D.F32, seed=2)
    assert ctx.depth_fusion_counts(77) is None and ctx.fused_depth(77) is None  # never fused
    rec = binding.AghDepthFusionCounts()
    assert ctx.lib.agh_get_depth_fusion_counts(ctx._h, C.c_int32(77), C.byref(rec)) == 0
    fa, wa = _check(ctx, a, dict(min_valid=2), slot=10, what="a")
    fb, wb = _check(ctx, b, dict(min_valid=1), slot=127, what="b")  # (the last slot)
    # both are held at once
    assert FU.same_image(ctx.fused_depth(10), wa["image"]) and FU.same_image(ctx.fused_depth(127), wb["image"])
    assert _counts(ctx, 10) == wa["counts"] and _counts(ctx, 127) == wb["counts"]
    # a larger image into a used slot regrows it, a smaller one then fits
    big = FU.random_burst(257, 5, 2, D.F32, seed=3)
    _check(ctx, big, dict(min_valid=1), slot=10, what="regrown")
    _check(ctx, a, dict(min_valid=2), slot=10, what="smaller again")
    assert FU.same_image(ctx.fused_depth(127), wb["image"])
    # the record: frame 0's intrinsics, scale and pose, the tight stride, a device pointer
    recs, _keep, _ = binding.depth_image_records(a)
    out = binding.AghDepthImage()
    fp = binding.depth_fusion_params()
    assert ctx.lib.agh_fuse_depth(ctx._h, recs, C.c_int32(len(recs)), C.byref(fp), C.c_int32(11), C.byref(out)) == 0
    r0 = recs[0]
    assert (out.width, out.height, out.format, out.row_stride_bytes) == (65, 3, binding.DEPTH_U16, 65 * 2)
    assert (out.depth_scale, out.fx, out.fy, out.cx, out.cy) == (r0.depth_scale, r0.fx, r0.fy, r0.cx, r0.cy)
    assert list(out.pose) == list(r0.pose) and out.data not in (None, 0) and out.data != r0.data
    back = binding.AghDepthImage()
    pixels = np.empty((3, 65), np.uint16)
    assert ctx.lib.agh_get_fused_depth(ctx._h, C.c_int32(11), pixels.ctypes.data_as(C.c_void_p), C.c_int64(pixels.nbytes), C.byref(back)) == pixels.nbytes
    assert bytes(back) == bytes(out)
    short = np.empty(pixels.size - 1, np.uint16)
    assert ctx.lib.agh_get_fused_depth(ctx._h, C.c_int32(11), short.ctypes.data_as(C.c_void_p), C.c_int64(short.nbytes), None) == binding.AGH_ERR_CAPACITY
    sized = binding.AghDepthImage()  # (a short buffer still gets the record, which says what is needed)
    assert ctx.lib.agh_get_fused_depth(ctx._h, C.c_int32(11), None, C.c_int64(0), C.byref(sized)) == binding.AGH_ERR_CAPACITY
    assert bytes(sized) == bytes(out)
    assert fa["fx"] == a[0]["fx"] and fb["data"].element_size() == 4


# ---- through the chains, with no synchronisation between the fuse and the chain ----
@pytest.fixture(scope="module")
def bursts():
    return FU.box_bursts()


def _fuse_pair(ctx, bursts, first_slot=0, device=False, **fp):
    return [ctx.fuse_depth(_device(b["frames"]) if device else b["frames"], slot=first_slot + k, **fp) for k, b in enumerate(bursts)]


def _copies(ctx, bursts, first_slot=0):
    """the host images of the same slots: fused_depth()'s copies under frame 0's intrinsics and pose"""
    return [dict(b["frames"][0], data=ctx.fused_depth(first_slot + k)) for k, b in enumerate(bursts)]


@pytest.mark.parametrize("setting", ["plain", "depth filter", "hand filter and clearance"])
def test_single_chain_on_the_fused_records(chain_ctx, bursts, setting):
    one = chain_ctx
    sc = HF.box_scene(2)
    kw = dict(KW, n_samples=200, sample_seed=4)
    if setting == "depth filter":
        one.set_depth_filter(max_jump_abs=0.02)
    elif setting != "plain":
        one.set_hand_filter(**HF.scene_filters(sc)["view"])
        one.set_hand_clearance(max_points=40)
    try:
        fused = _fuse_pair(one, bursts, min_valid=3)
        got = one.localize_depth(fused, sc["ws"], **kw)  # (behind the two fuses on the context's stream)
        counts = one.hand_filter_counts() if setting not in ("plain", "depth filter") else None
        want = one.localize_depth(_copies(one, bursts), sc["ws"], **kw)
        print(setting, "voxels", want["n_voxels"], "hypotheses", want["n_hypotheses"], "hands", len(want["hands"]),
              "handles", len(want["handles"]), "" if counts is None else counts.tolist())
        _same(got, want, setting)
        assert len(want["hands"]) >= 1
        if counts is not None:
            assert counts.tolist() == one.hand_filter_counts().tolist() and counts[0, 3] >= 1  # (the view test read the fused image)
    finally:
        one.clear_depth_filter()
        one.clear_hand_filter()
        one.clear_hand_clearance()


def test_batch_chain_on_the_fused_records(chain_ctx, bursts):
    one = chain_ctx
    sc = HF.box_scene(2)
    second = [FU.burst(im, 5, seed=31 + cam) for cam, im in enumerate(sc["images"])]
    f0 = _fuse_pair(one, bursts, 0, min_valid=3)
    f1 = _fuse_pair(one, second, 2, device=True, min_valid=2)
    kw = dict(KW, n_samples=[150, 120], sample_seeds=[3, 4])
    got = one.localize_depth_batch([f0, f1], [sc["ws"]] * 2, **kw)
    want = one.localize_depth_batch([_copies(one, bursts, 0), _copies(one, second, 2)], [sc["ws"]] * 2, **kw)
    for k in range(2):
        _same(got[k], want[k], f"capture {k}")
        assert len(want[k]["hands"]) >= 1
    assert not FU.same_image(one.fused_depth(0), one.fused_depth(2))


def test_labelled_chain_on_the_fused_records(chain_ctx, bursts):
    import torch

    one = chain_ctx
    sc = HF.box_scene(2)
    labels = HF.label_images(sc)
    fused = _fuse_pair(one, bursts, min_valid=3)
    kw = dict(KW, n_samples=80, sample_seed=6)
    got = one.localize_depth_labeled(fused, [torch.from_numpy(m).cuda() for m in labels], sc["ws"], 2, **kw)
    want = one.localize_depth_labeled(_copies(one, bursts), labels, sc["ws"], 2, **kw)
    assert len(got) == len(want) == 2
    for j in range(2):
        _same(got[j], want[j], f"object {j}")
    assert sum(len(w["hands"]) for w in want) >= 1


# ---- refusals ----
def _raw(ctx, recs, n, fp, slot, out=None, device=False):
    from agile_grasp_amd import binding

    out = binding.AghDepthImage() if out is None else out
    fn = ctx.lib.agh_fuse_depth_device if device else ctx.lib.agh_fuse_depth
    rc = fn(ctx._h, recs, C.c_int32(n), None if fp is None else C.byref(fp), C.c_int32(slot), None if out is False else C.byref(out))
    return rc, ctx.lib.agh_last_error(ctx._h).decode()


def test_refusals_leave_the_slot_alone(ctx):
    from agile_grasp_amd import binding

    bad = binding.AGH_ERR_INVALID_ARGUMENT
    frames = FU.random_burst(65, 3, 4, D.U16, seed=8, pad=2)
    _, want = _check(ctx, frames, dict(min_valid=2), slot=5, what="before")
    before = ctx.fused_depth(5)

    def recs_with(t=None, **fields):
        recs, keep, _ = binding.depth_image_records(frames)
        for k, v in fields.items():
            if k.startswith("pose"):
                recs[t].pose[int(k[4:])] = v
            else:
                setattr(recs[t], k, v)
        return recs, keep

    fp = binding.depth_fusion_params()
    recs, keep = recs_with()
    for args, text in (((None, 4, fp, 5), "frames is NULL"), ((recs, 4, None, 5), "params is NULL"), ((recs, 4, fp, 5, False), "fused_out is NULL"),
                       ((recs, 0, fp, 5), "n_frames must be 1..16"), ((recs, 17, fp, 5), "n_frames must be 1..16"),
                       ((recs, 4, fp, -1), "slot must be 0..127"), ((recs, 4, fp, 128), "slot must be 0..127"),
                       ((recs, 1, fp, 5), "min_valid must be 1..n_frames")):  # (the default of 2 with one frame)
        rc, err = _raw(ctx, *args)
        assert rc == bad and text in err and "agh_fuse_depth" in err, (text, rc, err)
    for fields, text in ((dict(min_valid=0), "min_valid must be 1..n_frames"), (dict(min_valid=5), "min_valid must be 1..n_frames"),
                         (dict(max_spread_abs=-1e-9), "max_spread_abs"), (dict(max_spread_abs=float("nan")), "max_spread_abs"),
                         (dict(max_spread_rel=float("inf")), "max_spread_rel"), (dict(max_spread_rel=-1.0), "max_spread_rel"),
                         (dict(reserved=1), "reserved must be 0")):
        rc, err = _raw(ctx, recs, 4, binding.depth_fusion_params(**fields), 5)
        assert rc == bad and text in err, (fields, rc, err)
    # per frame: depth_check's rules and wording, under the frame's name
    for t, fields, text in ((2, dict(data=None), "frame 2: data is NULL"), (1, dict(width=0), "frame 1: width must be 1..8192"),
                            (3, dict(height=8193), "frame 3: height must be 1..8192"),
                            (0, dict(format=2), "frame 0: format must be AGH_DEPTH_U16 or AGH_DEPTH_F32"),
                            (1, dict(row_stride_bytes=65 * 2 - 2), "frame 1: row_stride_bytes must be at least width x element size"),
                            (2, dict(row_stride_bytes=65 * 2 + 1), "frame 2: row_stride_bytes must be at least width x element size"),
                            (0, dict(depth_scale=0.0), "frame 0: depth_scale must be finite and positive"),
                            (3, dict(fx=0.0), "frame 3: fx must be finite and not zero"), (1, dict(fy=float("nan")), "frame 1: fy must be finite and not zero"),
                            (2, dict(cx=float("inf")), "frame 2: cx must be finite"), (0, dict(cy=float("nan")), "frame 0: cy must be finite"),
                            (3, dict(pose7=float("nan")), "frame 3: pose[7] must be finite")):
        r, keep = recs_with(t, **fields)
        rc, err = _raw(ctx, r, 4, fp, 5)
        assert rc == bad and text in err, (text, rc, err)
    # a frame that differs from frame 0
    for t, fields, text in ((1, dict(width=64), "frame 1: width differs from frame 0"), (2, dict(height=2), "frame 2: height differs from frame 0"),
                            (3, dict(format=binding.DEPTH_F32, row_stride_bytes=65 * 4), "frame 3: format differs from frame 0"),
                            (1, dict(depth_scale=0.002), "frame 1: depth_scale differs from frame 0"),
                            (2, dict(fx=frames[0]["fx"] * (1 + 2.0 ** -52)), "frame 2: fx differs from frame 0"),
                            (3, dict(fy=1.0), "frame 3: fy differs from frame 0"), (1, dict(cx=1.0), "frame 1: cx differs from frame 0"),
                            (2, dict(cy=-0.5), "frame 2: cy differs from frame 0"), (3, dict(pose11=0.25), "frame 3: pose[11] differs from frame 0")):
        r, keep = recs_with(t, **fields)
        rc, err = _raw(ctx, r, 4, fp, 5)
        assert rc == bad and text in err, (text, rc, err)
    # the device form: a pointer that is no multiple of the element size
    dev = _device(frames)
    r, keep, on_device = binding.depth_image_records(dev)
    assert on_device
    r[2].data = r[2].data + 1
    rc, err = _raw(ctx, r, 4, fp, 5, device=True)
    assert rc == bad and "frame 2: data (a device pointer) must be aligned to the element size" in err
    # nothing was launched: the slot holds what it held
    assert FU.same_image(ctx.fused_depth(5), before) and _counts(ctx, 5) == want["counts"]
    for rc in (ctx.lib.agh_get_depth_fusion_counts(ctx._h, C.c_int32(128), C.byref(binding.AghDepthFusionCounts())),
               ctx.lib.agh_get_fused_depth(ctx._h, C.c_int32(-1), before.ctypes.data_as(C.c_void_p), C.c_int64(before.nbytes), None)):
        assert rc == bad


def test_mid_chain_calls_are_refused_and_the_chain_is_unharmed(chain_ctx, bursts):
    from agile_grasp_amd import binding

    one = chain_ctx
    sc = HF.box_scene(2)
    frames = bursts[0]["frames"]
    one.fuse_depth(frames, slot=9, min_valid=3)
    before = one.fused_depth(9)
    counts = _counts(one, 9)
    kw = dict(KW, n_samples=150, sample_seed=2)
    want = one.localize_depth(sc["images"], sc["ws"], **kw)
    calls = (lambda: one.fuse_depth(frames, slot=9, min_valid=1), lambda: one.fuse_depth(_device(frames[:2]), slot=9),
             lambda: one.depth_fusion_counts(9), lambda: one.fused_depth(9))
    one.localize_depth_begin(sc["images"], sc["ws"], **kw)
    for call in calls:
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    _same(one.localize_end(), want, "single chain")
    bkw = dict(KW, n_samples=[150, 100], sample_seeds=[2, 3])
    want_b = one.localize_depth_batch([sc["images"]] * 2, [sc["ws"]] * 2, **bkw)
    one.localize_depth_batch_begin([sc["images"]] * 2, [sc["ws"]] * 2, **bkw)
    for call in calls:
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    got_b = one.localize_batch_end()
    for k in range(2):
        _same(got_b[k], want_b[k], f"batch chain, capture {k}")
    assert FU.same_image(one.fused_depth(9), before) and _counts(one, 9) == counts
