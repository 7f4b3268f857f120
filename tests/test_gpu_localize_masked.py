"""agh_localize_masked* and agh_localize_depth_masked* (include/agh.h): the chain with its samples drawn under a mask.  The sample
list, the count of eligible voxels and the voxelised cloud are held against the numpy model of tests/mask_cases.py, every chain
result against agh_localize with the reported list as explicit sample_idx on a second context -- exact equality throughout.

An explicit list may carry INT32_MIN slots (k_taubin_moments skips them like those of a drawn list), so the reference takes the
masked call's samples_out as it is."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_captures as D
from tests import mask_cases as M
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
SKIP = -(1 << 31)
POINTS = M.point_cases()
DEPTH = M.depth_cases()
RECT = (slice(80, 160), slice(120, 200))  # rows, columns of image 0 of the main case: over one object (see test_chain_equality)


def _point_kw(c):
    return dict(dense=c["dense"], cell_size=c["cell"])


def _point_model(c):
    cams = M.camera_ids(c["points"], c["size_left"], c["dense"])
    keep = cams >= 0
    vox = D.voxel_model(c["points"][keep, :3], cams[keep], c["workspace"], c["cell"])
    return M.eligible_model(c["points"], cams, c["mask"], c["workspace"], c["cell"]), vox


def _check_model(ctx, got, E, vox, S, seed):
    from agile_grasp_amd.binding import masked_samples

    want = masked_samples(E, S, seed)
    print("M", len(E), "S", S, "voxels", len(vox[0]), "skips", int((want == SKIP).sum()), "hypotheses", got["n_hypotheses"])
    assert np.array_equal(got["samples"], want)
    assert ctx.sample_mask_count() == len(E)
    assert got["n_voxels"] == len(vox[0])
    gx, gc = ctx.cloud()
    assert np.array_equal(gx, vox[0]) and np.array_equal(gc, vox[1])


@pytest.fixture(scope="module")
def main():
    """the main case with a rectangular mask over one object of image 0, image 1's mask NULL; the model's points (read-only)"""
    images, ws, origins = D.main_case()
    pts = D.deproject_ref(images)
    pts.setflags(write=False)
    m0 = np.zeros(images[0]["data"].shape, np.uint8)
    m0[RECT] = 1
    masks = [m0, None]
    packed = M.packed_masks(images, masks)
    obj = pts[(packed != 0) & np.isfinite(pts).all(1)]
    ws_cut = ws.copy()
    ws_cut[1] = np.median(obj[:, 0]) + 0.01  # a face of the workspace through the object: hypotheses within 2 cm of it
    return dict(images=images, ws=ws, ws_cut=ws_cut, origins=origins, pts=pts, size_left=images[0]["data"].size, masks=masks,
                packed=packed, cams=D.image_index(images))


@pytest.mark.parametrize("name", sorted(POINTS))
def test_points_cases_equal_the_model(name):
    from agile_grasp_amd import binding

    c = POINTS[name]
    E, vox = _point_model(c)
    ctx = binding.Context(np.zeros((2, 3)))
    S = min(len(E) + 2, 24) if name != "dense_block" else 200
    got = ctx.localize_masked(c["points"], c["size_left"], c["workspace"], c["mask"], n_samples=S, sample_seed=11, classify=False,
                              **_point_kw(c))
    _check_model(ctx, got, E, vox, S, 11)
    if name == "all_dropped":
        assert len(E) == 0 and (got["samples"] == SKIP).all() and got["n_hypotheses"] == 0 and len(got["hands"]) == 0
        assert len(got["handles"]) == 0
    # the mask stage runs for n_samples = 0 too
    got = ctx.localize_masked(c["points"], c["size_left"], c["workspace"], c["mask"], n_samples=0, classify=False, **_point_kw(c))
    assert ctx.sample_mask_count() == len(E) and got["n_voxels"] == len(vox[0]) and len(got["samples"]) == 0
    ctx.close()


def test_strata_of_width_one_and_two_and_the_skip_slots():
    from agile_grasp_amd import binding

    c = POINTS["stride32"]
    E, vox = _point_model(c)
    m = len(E)
    assert m > 20
    ctx = binding.Context(np.zeros((2, 3)))
    for S in (m - 1, m, m + 1, 2 * m - 1, 2 * m + 3, 1, m // 2):
        got = ctx.localize_masked(c["points"], c["size_left"], c["workspace"], c["mask"], n_samples=S, sample_seed=S + 5,
                                  classify=False, **_point_kw(c))
        _check_model(ctx, got, E, vox, S, S + 5)
    ctx.close()


@pytest.mark.parametrize("name", sorted(DEPTH))
def test_depth_cases_equal_the_model_and_the_points_form(name):
    from agile_grasp_amd import binding

    images, masks, ws = DEPTH[name]
    one, two = (binding.Context(np.zeros((2, 3))) for _ in range(2))
    pts = one.deproject(images)
    cams = D.image_index(images)
    packed = M.packed_masks(images, masks)
    E = M.eligible_model(pts, cams, packed, ws)
    vox = D.voxel_model(pts, cams, ws)
    S = 40
    got = one.localize_depth_masked(images, masks, ws, n_samples=S, sample_seed=3, classify=False)
    _check_model(one, got, E, vox, S, 3)
    want = two.localize_masked(pts, images[0]["data"].size, ws, packed, n_samples=S, sample_seed=3, classify=False, dense=True)
    assert two.sample_mask_count() == len(E)
    _same(got, want, name)
    one.close()
    two.close()


@pytest.mark.parametrize("mode", ["classified", "boundaries"])
def test_chain_equality(svm_model, main, mode):
    """The masked chain, depth and points form, against agh_localize with the list the masked call reports, on a second context.
    The rectangle was chosen with the CPU oracle (oracle_py.find_hands and classify on the voxel model, S = 300, seed 7): the
    explicit list alone yields 340 hypotheses and 206 kept hands, and with the workspace cut through the object 441 hypotheses,
    292 kept hands, 14 hypotheses within 2 cm of a face."""
    one, two, ref = _contexts(main["origins"], svm_model, n=3)
    ws = main["ws"] if mode == "classified" else main["ws_cut"]
    kw = dict(KW, filters_boundaries=mode == "boundaries")
    got = one.localize_depth_masked(main["images"], main["masks"], ws, n_samples=300, sample_seed=7, **kw)
    E = M.eligible_model(main["pts"], main["cams"], main["packed"], ws)
    _check_model(one, got, E, D.voxel_model(main["pts"], main["cams"], ws), 300, 7)
    want = ref.localize(np.array(main["pts"]), main["size_left"], ws, dense=True, samples=got["samples"], **kw)
    print(mode, "hypotheses", want["n_hypotheses"], "hands", len(want["hands"]), "handles", len(want["handles"]))
    assert want["n_hypotheses"] >= 20 and len(want["hands"]) >= 1
    _same(got, want, mode + " depth")
    pts_got = two.localize_masked(np.array(main["pts"]), main["size_left"], ws, main["packed"], dense=True, n_samples=300,
                                  sample_seed=7, **kw)
    _same(pts_got, want, mode + " points")
    if mode == "boundaries":
        plain = one.localize_depth_masked(main["images"], main["masks"], ws, n_samples=300, sample_seed=7, **KW)
        assert plain["n_hypotheses"] == got["n_hypotheses"] and len(plain["hands"]) >= len(got["hands"])


def test_skip_slots_in_the_chain(svm_model, main):
    """fewer eligible voxels than samples: the reference takes the list with its INT32_MIN slots"""
    one, ref = _contexts(main["origins"], svm_model)
    m0 = np.zeros(main["images"][0]["data"].shape, np.uint8)
    m0[130:144, 170:184] = 1  # (135 eligible voxels on an object: the CPU oracle finds 653 hypotheses there)
    packed = M.packed_masks(main["images"], [m0, None])
    E = M.eligible_model(main["pts"], main["cams"], packed, main["ws"])
    S = len(E) + 37
    got = one.localize_depth_masked(main["images"], [m0, None], main["ws"], n_samples=S, sample_seed=2, **KW)
    assert 20 < len(E) and (got["samples"][len(E):] == SKIP).all() and np.array_equal(got["samples"][:len(E)], E)
    want = ref.localize(np.array(main["pts"]), main["size_left"], main["ws"], dense=True, samples=got["samples"], **KW)
    assert want["n_hypotheses"] >= 1
    _same(got, want, "skip slots")


def test_an_all_ones_mask_equals_the_drawn_list(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    pts = np.array(main["pts"])
    kw = dict(KW, n_samples=300, sample_seed=9, dense=True)
    want = ref.localize(pts, main["size_left"], main["ws"], **kw)
    got = one.localize_masked(pts, main["size_left"], main["ws"], np.ones(len(pts), np.uint8), **kw)
    assert one.sample_mask_count() == want["n_voxels"] and want["n_hypotheses"] >= 20
    _same(got, want, "all ones")
    ones = [np.ones(im["data"].shape, np.uint8) for im in main["images"]]
    _same(one.localize_depth_masked(main["images"], ones, main["ws"], n_samples=300, sample_seed=9, **KW), want, "all ones, depth")


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_device_points_and_mask_at_any_byte_offset(svm_model, main, offset):
    import torch

    one, ref = _contexts(main["origins"], svm_model)
    for name, c in (("values", POINTS["values"]), ("tiny", POINTS["tiny"]), ("word_edge", POINTS["word_edge"])):
        assert len(c["points"]) % 4 != 0
        E, vox = _point_model(c)
        t = torch.from_numpy(np.concatenate([np.full(offset, 9, np.uint8), c["mask"], np.full(5, 9, np.uint8)])).cuda()
        view = t[offset:offset + len(c["mask"])]
        assert view.data_ptr() == t.data_ptr() + offset
        got = one.localize_masked(torch.from_numpy(c["points"]).cuda(), c["size_left"], c["workspace"], view, n_samples=20,
                                  sample_seed=4, classify=False, **_point_kw(c))
        _check_model(one, got, E, vox, 20, 4)
    pts = np.array(main["pts"])
    kw = dict(KW, n_samples=200, sample_seed=5, dense=True)
    want = ref.localize_masked(pts, main["size_left"], main["ws"], main["packed"], **kw)
    t = torch.from_numpy(np.concatenate([np.full(offset, 9, np.uint8), main["packed"]])).cuda()
    got = one.localize_masked(torch.from_numpy(pts).cuda(), main["size_left"], main["ws"], t[offset:], **kw)
    assert one.sample_mask_count() == ref.sample_mask_count() and want["n_hypotheses"] >= 20
    _same(got, want, "device points")


@pytest.mark.parametrize("name", ["main_random_padded", "u16_odd_stride_first_null", "total_1025_random_padded"])
def test_device_depth_masks_with_padded_rows(name):
    import torch

    from agile_grasp_amd import binding

    images, masks, ws = DEPTH[name]
    one, ref = (binding.Context(np.zeros((2, 3))) for _ in range(2))
    want = ref.localize_depth_masked(images, masks, ws, n_samples=60, sample_seed=8, classify=False)
    dev_images, dev_masks, keep = [], [], []
    for im, m in zip(images, masks):
        d = im["data"]
        full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
        full[:, :d.shape[1]] = d
        t = torch.from_numpy(full.view(np.int16) if d.dtype == np.uint16 else full).cuda()
        dev_images.append(dict(im, data=t[:, :d.shape[1]]))
        keep.append(t)
        if m is None:
            dev_masks.append(None)
            continue
        wide = np.full((m.shape[0], m.shape[1] + 3), 9, np.uint8)
        wide[:, :m.shape[1]] = m
        flat = torch.from_numpy(np.concatenate([np.full(1, 9, np.uint8), wide.reshape(-1)])).cuda()  # rows padded, base odd
        dev_masks.append(flat[1:].view(wide.shape)[:, :m.shape[1]])
        keep.append(flat)
    got = one.localize_depth_masked(dev_images, dev_masks, ws, n_samples=60, sample_seed=8, classify=False)
    assert one.sample_mask_count() == ref.sample_mask_count() > 0
    _same(got, want, name)
    one.close()
    ref.close()


def test_begin_and_end_equal_the_blocking_calls(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=250, sample_seed=6)
    want = ref.localize_depth_masked(main["images"], main["masks"], main["ws"], **kw)
    assert want["n_hypotheses"] >= 20
    assert one.localize_depth_masked(main["images"], main["masks"], main["ws"], phase="begin", **kw) is None
    _same(one.localize_end(), want, "depth begin + end")
    assert one.sample_mask_count() == ref.sample_mask_count()
    pts = np.array(main["pts"])
    assert one.localize_masked(pts, main["size_left"], main["ws"], main["packed"], dense=True, phase="begin", **kw) is None
    _same(one.localize_end(), want, "points begin + end")
    # a masked begin of host data never adopts a staged set: it drops it, and the next unmasked begin uploads its own
    staged = one.localize_stage(pts)
    one.localize_masked(staged, main["size_left"], main["ws"], main["packed"], dense=True, phase="begin", **kw)
    _same(one.localize_end(), want, "staged set dropped")
    one.localize_depth_stage(main["images"])
    one.localize_depth_masked(main["images"], main["masks"], main["ws"], phase="begin", **kw)
    _same(one.localize_end(), want, "staged depth set dropped")
    plain = ref.localize_depth(main["images"], main["ws"], **kw)
    one.localize_depth_begin(main["images"], main["ws"], **kw)
    _same(one.localize_end(), plain, "unmasked after the dropped sets")


def test_the_outgrown_bitmap_repeat_inside_a_masked_call(svm_model, main):
    """A small-extent capture sizes the context's bitmaps; the wide one's lattice outgrows them and the chain is run once more
    inside the call, with the mask the first pass copied.  Host and device forms."""
    import torch

    one, dev, ref = _contexts(main["origins"], svm_model, n=3)
    images, masks, ws = main["images"], main["masks"], main["ws"]
    kw = dict(KW, n_samples=300, sample_seed=6)
    mid = 0.5 * (ws[0::2] + ws[1::2])
    half = 0.08 * (ws[1::2] - ws[0::2])
    small = np.stack([mid - half, mid + half], axis=1).reshape(6)
    ones = [np.ones(im["data"].shape, np.uint8) for im in images]
    first = one.localize_depth_masked(images, ones, small, **kw)
    assert first["n_voxels"] > 100 and one.sample_mask_count() == first["n_voxels"]
    builds = one.grid_stats()["builds"]
    got = one.localize_depth_masked(images, masks, ws, **kw)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the chain twice: the lattice outgrew the kept bitmap)
    E = M.eligible_model(main["pts"], main["cams"], main["packed"], ws)
    _check_model(one, got, E, D.voxel_model(main["pts"], main["cams"], ws), 300, 6)
    pts = np.array(main["pts"])
    want = ref.localize(pts, main["size_left"], ws, dense=True, samples=got["samples"], **KW)
    assert want["n_hypotheses"] >= 20
    _same(got, want, "repeat, host")
    d_pts, d_ones, d_mask = torch.from_numpy(pts).cuda(), torch.ones(len(pts), dtype=torch.uint8).cuda(), torch.from_numpy(main["packed"]).cuda()
    dev.localize_masked(d_pts, main["size_left"], small, d_ones, dense=True, **kw)
    builds = dev.grid_stats()["builds"]
    got = dev.localize_masked(d_pts, main["size_left"], ws, d_mask, dense=True, **kw)
    assert dev.grid_stats()["builds"] - builds == 2 and dev.sample_mask_count() == len(E)
    _same(got, want, "repeat, device")


def test_no_sticky_state(svm_model, main):
    from agile_grasp_amd import binding

    one, fresh = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=200, sample_seed=5)
    one.localize_depth_masked(main["images"], main["masks"], main["ws"], **kw)
    assert one.sample_mask_count() > 0
    pts = np.array(main["pts"])
    want = fresh.localize(pts, main["size_left"], main["ws"], dense=True, **kw)
    _same(one.localize(pts, main["size_left"], main["ws"], dense=True, **kw), want, "unmasked after masked")
    for ctx in (one, fresh):
        with pytest.raises(binding.AghError) as e:
            ctx.sample_mask_count()
        assert e.value.code == binding.AGH_ERR_STATE
    _same(one.localize_depth(main["images"], main["ws"], **kw), want, "unmasked depth after masked")
    # ... and after a batch chain the count is gone too
    one.localize_masked(pts, main["size_left"], main["ws"], main["packed"], dense=True, **kw)
    assert one.sample_mask_count() > 0
    one.localize_batch([pts], [main["size_left"]], [main["ws"]], n_samples=50, dense=True, **KW)
    with pytest.raises(binding.AghError) as e:
        one.sample_mask_count()
    assert e.value.code == binding.AGH_ERR_STATE


def test_refusals(svm_model, main):
    from agile_grasp_amd import binding

    one, ref = _contexts(main["origins"], svm_model)
    images, masks, ws = main["images"], main["masks"], main["ws"]
    pts = np.array(main["pts"])
    kw = dict(KW, n_samples=200, sample_seed=8)
    want = ref.localize_depth_masked(images, masks, ws, **kw)
    M0 = ref.sample_mask_count()
    assert one.localize_depth_masked(images, masks, ws, **kw)["n_hypotheses"] == want["n_hypotheses"]
    bad, state = binding.AGH_ERR_INVALID_ARGUMENT, binding.AGH_ERR_STATE
    short = np.ones(images[0]["data"].shape, np.uint8)
    short_recs = [short, None]
    some = np.arange(10, dtype=np.int32)

    def short_stride(phase="both"):
        """a row stride below the width, through the raw record"""
        recs, keep, _ = binding.depth_image_records(images)
        mrecs, mkeep = binding.sample_mask_records(short_recs, False)
        mrecs[0].row_stride_bytes = images[0]["data"].shape[1] - 1
        lp, _, S, hcap = one._localize_params(0, ws, None, 200, 8, True, 2, 0.005, 0.003, False, False)
        if phase == "begin":
            return one._check(one.lib.agh_localize_depth_masked_begin(one._h, recs, mrecs, C.c_int32(2), C.byref(lp)))
        return one._localize_blocking(one.lib.agh_localize_depth_masked, (recs, mrecs, C.c_int32(2)), lp, S, hcap)

    calls = {
        "mask with sample_idx, points": (bad, lambda: one.localize_masked(pts, main["size_left"], ws, main["packed"], dense=True, samples=some, **KW)),
        "mask with sample_idx, depth": (bad, lambda: one.localize_depth_masked(images, masks, ws, samples=some, **KW)),
        "mask with sample_idx, begin": (bad, lambda: one.localize_masked(pts, main["size_left"], ws, main["packed"], dense=True, samples=some, phase="begin", **KW)),
        "NULL mask": (bad, lambda: one.localize_masked(pts, main["size_left"], ws, None, dense=True, **kw)),
        "NULL mask, begin": (bad, lambda: one.localize_masked(pts, main["size_left"], ws, None, dense=True, phase="begin", **kw)),
        "NULL masks": (bad, lambda: one.localize_depth_masked(images, None, ws, **kw)),
        "all-NULL masks": (bad, lambda: one.localize_depth_masked(images, [None, None], ws, **kw)),
        "all-NULL masks, begin": (bad, lambda: one.localize_depth_masked(images, [None, None], ws, phase="begin", **kw)),
        "short row stride": (bad, short_stride),
        "short row stride, begin": (bad, lambda: short_stride("begin")),
        "a twin's validation": (bad, lambda: one.localize_depth_masked(images, masks, ws, n_samples=-1, **KW)),
    }
    for what, (code, call) in calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == code, (what, str(e.value))
        # nothing queued, nothing bound or changed: no chain to end, the last count stands, the context still works
        with pytest.raises(binding.AghError) as e:
            one.localize_end()
        assert e.value.code == state, what
        assert one.sample_mask_count() == M0, what
    _same(one.localize_depth_masked(images, masks, ws, **kw), want, "after the refusals")
    plain = binding.Context(main["origins"])
    with pytest.raises(binding.AghError) as e:
        plain.localize_depth_masked(images, masks, ws, **kw)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    # mid-chain: every masked call and the count are refused, the chain in flight is untouched
    masked_calls = {
        "agh_localize_masked": lambda: one.localize_masked(pts, main["size_left"], ws, main["packed"], dense=True, **kw),
        "agh_localize_masked_begin": lambda: one.localize_masked(pts, main["size_left"], ws, main["packed"], dense=True, phase="begin", **kw),
        "agh_localize_depth_masked": lambda: one.localize_depth_masked(images, masks, ws, **kw),
        "agh_localize_depth_masked_begin": lambda: one.localize_depth_masked(images, masks, ws, phase="begin", **kw),
        "agh_get_sample_mask_count": one.sample_mask_count,
    }
    one.localize_depth_masked(images, masks, ws, phase="begin", **kw)
    keep, keep_s = one._loc_keep, one._loc_S
    for name, call in masked_calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == state and name + ": " in str(e.value), (name, str(e.value))
        one._loc_keep, one._loc_S = keep, keep_s
    _same(one.localize_end(), want, "after the mid-chain refusals")
    assert one.sample_mask_count() == M0
    # mid-batch likewise
    batch_want = ref.localize_batch([pts], [main["size_left"]], [ws], n_samples=100, dense=True, **KW)
    one.localize_batch_begin([pts], [main["size_left"]], [ws], n_samples=100, dense=True, **KW)
    for name, call in masked_calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == state and name + ": " in str(e.value), (name, str(e.value))
    _same(one.localize_batch_end()[0], batch_want[0], "after the mid-batch refusals")
    _same(one.localize_depth_masked(images, masks, ws, **kw), want, "at the end")
