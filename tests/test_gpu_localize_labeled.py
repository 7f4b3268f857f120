"""agh_localize_labeled* and agh_localize_depth_labeled* (include/agh.h): one capture, one sample list per object of a label
image.  The sample lists, the counts of eligible voxels and the voxelised cloud are held against the numpy model of
tests/label_cases.py; every object's span of every output against agh_localize_masked with the mask labels == j + 1 on a second
context -- exact equality throughout."""
import ctypes as C

import numpy as np
import pytest

from tests import depth_captures as D
from tests import label_cases as L
from tests import mask_cases as M
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
SKIP = -(1 << 31)
POINTS = L.point_cases()


def _kw(c):
    return dict(dense=c["dense"], cell_size=c["cell"])


def _model(c):
    cams = L.cams_of(c)
    keep = cams >= 0
    return L.eligible_lists(c, cams), D.voxel_model(c["points"][keep, :3], cams[keep], c["workspace"], c["cell"])


def _check_model(ctx, got, E, vox, S, seed):
    from agile_grasp_amd.binding import labeled_samples

    want = labeled_samples(E, S, seed)
    print("M", [len(e) for e in E], "S", S, "voxels", len(vox[0]), "hypotheses", [g["n_hypotheses"] for g in got])
    assert len(got) == len(E)
    assert np.array_equal(np.concatenate([g["samples"] for g in got]) if S else np.zeros(0, np.int32), want)
    assert np.array_equal(ctx.label_counts(), [len(e) for e in E])
    assert all(g["n_voxels"] == len(vox[0]) for g in got)
    gx, gc = ctx.cloud()
    assert np.array_equal(gx, vox[0]) and np.array_equal(gc, vox[1])


def _labeled(ctx, c, labels=None, **kw):
    return ctx.localize_labeled(c["points"], c["size_left"], c["workspace"], c["labels"] if labels is None else labels,
                                c["n_objects"], classify=False, **_kw(c), **kw)


@pytest.fixture(scope="module")
def main():
    """the main depth case with image 0 tiled 3 x 4 into objects 0 .. 11 and image 1's labels NULL; the model's points (read-only)"""
    images, ws, origins = D.main_case()
    pts = D.deproject_ref(images)
    pts.setflags(write=False)
    labels = [L.tiled_labels(images[0]["data"].shape), None]
    packed = M.packed_masks(images, labels)
    # a face of the workspace through a tile, hypotheses within 2 cm of it: the +x face through the last tile, whose column is the
    # one the cut shortens (x grows with the image column), so that the other columns keep their objects whole
    tile = pts[(packed == 12) & np.isfinite(pts).all(1)]
    ws_cut = ws.copy()
    ws_cut[1] = np.median(tile[:, 0]) + 0.01
    return dict(images=images, ws=ws, ws_cut=ws_cut, origins=origins, pts=pts, size_left=images[0]["data"].size, labels=labels,
                packed=packed, cams=D.image_index(images), K=12)


@pytest.mark.parametrize("name", sorted(POINTS))
def test_points_cases_equal_the_model(name):
    from agile_grasp_amd import binding

    c = POINTS[name]
    E, vox = _model(c)
    ctx = binding.Context(np.zeros((2, 3)))
    S = 200 if name == "dense_block" else min(max(len(e) for e in E) + 2, 24)
    got = _labeled(ctx, c, n_samples=S, sample_seed=11)
    _check_model(ctx, got, E, vox, S, 11)
    for j, e in enumerate(E):
        if len(e) == 0:
            assert (got[j]["samples"] == SKIP).all() and got[j]["n_hypotheses"] == 0 and len(got[j]["hands"]) == 0
            assert len(got[j]["handles"]) == 0
    # the label stage runs for n_samples = 0 too
    got = _labeled(ctx, c, n_samples=0)
    _check_model(ctx, got, E, vox, 0, 1)
    ctx.close()


def test_samples_around_the_counts():
    from agile_grasp_amd import binding

    c = POINTS["stride32"]
    E, vox = _model(c)
    ctx = binding.Context(np.zeros((2, 3)))
    sizes = set()
    for m in (len(e) for e in E):
        assert m > 5
        sizes |= {m - 1, m, m + 1, 2 * m + 3}
    for S in sorted(sizes):
        _check_model(ctx, _labeled(ctx, c, n_samples=S, sample_seed=S + 5), E, vox, S, S + 5)
    ctx.close()


def _masked_twins(ref, main, ws, form, kw):
    out, counts = [], []
    for j in range(main["K"]):
        mask = (main["packed"] == j + 1).astype(np.uint8)
        if form == "depth":
            n0 = main["size_left"]
            masks = [mask[:n0].reshape(main["images"][0]["data"].shape), None]
            out.append(ref.localize_depth_masked(main["images"], masks, ws, **kw) if masks[0].any() else None)
        else:
            out.append(ref.localize_masked(np.array(main["pts"]), main["size_left"], ws, mask, dense=True, **kw))
        counts.append(ref.sample_mask_count() if out[-1] is not None else 0)
    return out, counts


def _same_objects(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        if w is not None:
            _same(g, w, (what, j))


@pytest.mark.parametrize("mode", ["classified", "boundaries"])
def test_chain_equality(svm_model, main, mode):
    """Image 0 of the main case tiled 3 x 4 into objects 0 .. 11, image 1's labels NULL, S = 100, seed 7, the classifier on,
    min_inliers = 2.  With the CPU oracle (oracle_py.find_hands on the voxel model) this yields 826 hypotheses, between 41 and
    117 per object except object 8, which has M = 0.  Every object's span against agh_localize_masked of its mask on a second
    context, depth and points form; then with filters_boundaries on a workspace cut through a tile."""
    one, two, ref = _contexts(main["origins"], svm_model, n=3)
    ws = main["ws"] if mode == "classified" else main["ws_cut"]
    kw = dict(KW, n_samples=100, sample_seed=7, filters_boundaries=mode == "boundaries")
    got = one.localize_depth_labeled(main["images"], main["labels"], ws, main["K"], **kw)
    E = [M.eligible_model(main["pts"], main["cams"], main["packed"] == j + 1, ws) for j in range(main["K"])]
    _check_model(one, got, E, D.voxel_model(main["pts"], main["cams"], ws), 100, 7)
    print(mode, "hypotheses", [g["n_hypotheses"] for g in got], "hands", [len(g["hands"]) for g in got], "handles",
          [len(g["handles"]) for g in got])
    assert sum(g["n_hypotheses"] >= 20 for g in got) >= 10 and sum(len(g["handles"]) >= 1 for g in got) >= 2
    want, counts = _masked_twins(ref, main, ws, "points", kw)
    assert counts == [len(e) for e in E]
    _same_objects(got, want, mode + " depth")
    _same_objects(two.localize_labeled(np.array(main["pts"]), main["size_left"], ws, main["packed"], main["K"], dense=True, **kw),
                  want, mode + " points")
    if mode == "classified":
        assert len(E[8]) == 0 and got[8]["n_hypotheses"] == 0
        _same_objects(got, _masked_twins(ref, main, ws, "depth", kw)[0], "depth twins")
    else:
        plain = one.localize_depth_labeled(main["images"], main["labels"], ws, main["K"], **dict(kw, filters_boundaries=False))
        assert [p["n_hypotheses"] for p in plain] == [g["n_hypotheses"] for g in got]
        assert sum(len(p["hands"]) for p in plain) >= sum(len(g["hands"]) for g in got)


def test_one_object_equals_the_masked_call(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=200, sample_seed=5)
    m0 = np.zeros(main["images"][0]["data"].shape, np.uint8)
    m0[80:160, 120:200] = 1
    want = ref.localize_depth_masked(main["images"], [m0, None], main["ws"], **kw)
    got = one.localize_depth_labeled(main["images"], [m0, None], main["ws"], 1, **kw)
    assert len(got) == 1 and want["n_hypotheses"] >= 20 and list(one.label_counts()) == [ref.sample_mask_count()]
    _same(got[0], want, "one object")


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_device_points_and_labels_at_any_byte_offset(svm_model, main, offset):
    import torch

    one, ref = _contexts(main["origins"], svm_model)
    for name in ("values", "k1", "word_edge", "row_65"):
        c = POINTS[name]
        E, vox = _model(c)
        t = torch.from_numpy(np.concatenate([np.full(offset, 1, np.uint8), c["labels"], np.full(5, 1, np.uint8)])).cuda()
        view = t[offset:offset + len(c["labels"])]
        assert view.data_ptr() == t.data_ptr() + offset
        got = one.localize_labeled(torch.from_numpy(c["points"]).cuda(), c["size_left"], c["workspace"], view, c["n_objects"],
                                   n_samples=20, sample_seed=4, classify=False, **_kw(c))
        _check_model(one, got, E, vox, 20, 4)
    pts = np.array(main["pts"])
    kw = dict(KW, n_samples=60, sample_seed=5, dense=True)
    want = ref.localize_labeled(pts, main["size_left"], main["ws"], main["packed"], main["K"], **kw)
    t = torch.from_numpy(np.concatenate([np.full(offset, 1, np.uint8), main["packed"]])).cuda()
    got = one.localize_labeled(torch.from_numpy(pts).cuda(), main["size_left"], main["ws"], t[offset:], main["K"], **kw)
    assert np.array_equal(one.label_counts(), ref.label_counts()) and sum(w["n_hypotheses"] for w in want) >= 100
    _same_objects(got, want, "device points")


def test_device_depth_labels_with_padded_rows_and_an_odd_base(svm_model, main):
    import torch

    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=60, sample_seed=8)
    images, labels = main["images"], main["labels"]
    want = ref.localize_depth_labeled(images, labels, main["ws"], main["K"], **kw)
    dev_images, dev_labels, keep = [], [], []
    for im, m in zip(images, labels):
        d = im["data"]
        full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
        full[:, :d.shape[1]] = d
        t = torch.from_numpy(full.view(np.int16) if d.dtype == np.uint16 else full).cuda()
        dev_images.append(dict(im, data=t[:, :d.shape[1]]))
        keep.append(t)
        if m is None:
            dev_labels.append(None)
            continue
        wide = np.full((m.shape[0], m.shape[1] + 3), 1, np.uint8)
        wide[:, :m.shape[1]] = m
        flat = torch.from_numpy(np.concatenate([np.full(1, 1, np.uint8), wide.reshape(-1)])).cuda()  # rows padded, base odd
        dev_labels.append(flat[1:].view(wide.shape)[:, :m.shape[1]])
        keep.append(flat)
    got = one.localize_depth_labeled(dev_images, dev_labels, main["ws"], main["K"], **kw)
    assert np.array_equal(one.label_counts(), ref.label_counts()) and ref.label_counts().sum() > 0
    _same_objects(got, want, "device depth")
    # host labels in padded rows
    host = [np.ascontiguousarray(np.pad(labels[0], ((0, 0), (0, 5)), constant_values=1))[:, :labels[0].shape[1]], None]
    _same_objects(one.localize_depth_labeled(images, host, main["ws"], main["K"], **kw), want, "host padded")


def test_the_outgrown_bitmap_repeat_inside_a_labelled_call(svm_model, main):
    """A small-extent capture sizes the context's bitmaps; the wide one's lattice outgrows them and the chain is run once more
    inside the call, with the labels where the first pass left them.  Host and device forms."""
    import torch

    one, dev, ref = _contexts(main["origins"], svm_model, n=3)
    images, labels, ws, K = main["images"], main["labels"], main["ws"], main["K"]
    kw = dict(KW, n_samples=60, sample_seed=6)
    mid = 0.5 * (ws[0::2] + ws[1::2])
    half = 0.08 * (ws[1::2] - ws[0::2])
    small = np.stack([mid - half, mid + half], axis=1).reshape(6)
    pts = np.array(main["pts"])
    want = ref.localize_labeled(pts, main["size_left"], ws, main["packed"], K, dense=True, **kw)
    first = one.localize_depth_labeled(images, labels, small, K, **kw)
    assert first[0]["n_voxels"] > 100
    builds = one.grid_stats()["builds"]
    got = one.localize_depth_labeled(images, labels, ws, K, **kw)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the chain twice: the lattice outgrew the kept bitmap)
    E = [M.eligible_model(main["pts"], main["cams"], main["packed"] == j + 1, ws) for j in range(K)]
    _check_model(one, got, E, D.voxel_model(main["pts"], main["cams"], ws), 60, 6)
    assert sum(w["n_hypotheses"] for w in want) >= 100
    _same_objects(got, want, "repeat, host")
    d_pts, d_lab = torch.from_numpy(pts).cuda(), torch.from_numpy(main["packed"]).cuda()
    dev.localize_labeled(d_pts, main["size_left"], small, d_lab, K, dense=True, **kw)
    builds = dev.grid_stats()["builds"]
    got = dev.localize_labeled(d_pts, main["size_left"], ws, d_lab, K, dense=True, **kw)
    assert dev.grid_stats()["builds"] - builds == 2 and np.array_equal(dev.label_counts(), [len(e) for e in E])
    _same_objects(got, want, "repeat, device")


def test_no_sticky_state(svm_model, main):
    from agile_grasp_amd import binding

    one, fresh = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=100, sample_seed=5)
    pts = np.array(main["pts"])
    m0 = (main["packed"] == 6).astype(np.uint8)

    def labelled():
        one.localize_depth_labeled(main["images"], main["labels"], main["ws"], main["K"], **kw)
        assert one.label_counts().sum() > 0
        with pytest.raises(binding.AghError) as e:
            one.sample_mask_count()
        assert e.value.code == binding.AGH_ERR_STATE

    def no_counts(ctx):
        with pytest.raises(binding.AghError) as e:
            ctx.label_counts()
        assert e.value.code == binding.AGH_ERR_STATE

    no_counts(fresh)
    labelled()
    _same(one.localize(pts, main["size_left"], main["ws"], dense=True, **kw),
          fresh.localize(pts, main["size_left"], main["ws"], dense=True, **kw), "unmasked after labelled")
    no_counts(one)
    labelled()
    _same(one.localize_masked(pts, main["size_left"], main["ws"], m0, dense=True, **kw),
          fresh.localize_masked(pts, main["size_left"], main["ws"], m0, dense=True, **kw), "masked after labelled")
    assert one.sample_mask_count() == fresh.sample_mask_count() > 0
    no_counts(one)
    labelled()
    got = one.localize_batch([pts, pts[:50000]], [main["size_left"], 50000], [main["ws"]] * 2, n_samples=50, dense=True, **KW)
    want = fresh.localize_batch([pts, pts[:50000]], [main["size_left"], 50000], [main["ws"]] * 2, n_samples=50, dense=True, **KW)
    for k in range(2):
        _same(got[k], want[k], ("batch after labelled", k))
    no_counts(one)
    labelled()
    with pytest.raises(binding.AghError) as e:
        one.label_counts(cap_objects=main["K"] - 1)
    assert e.value.code == binding.AGH_ERR_CAPACITY
    assert len(one.label_counts(cap_objects=main["K"])) == main["K"]


def test_refusals(svm_model, main):
    from agile_grasp_amd import binding

    one, ref = _contexts(main["origins"], svm_model)
    images, labels, ws, K = main["images"], main["labels"], main["ws"], main["K"]
    pts = np.array(main["pts"])
    kw = dict(KW, n_samples=60, sample_seed=8)
    want = ref.localize_depth_labeled(images, labels, ws, K, **kw)
    M0 = ref.label_counts()
    got = one.localize_depth_labeled(images, labels, ws, K, **kw)
    assert [g["n_hypotheses"] for g in got] == [w["n_hypotheses"] for w in want]
    bad, state, cap = binding.AGH_ERR_INVALID_ARGUMENT, binding.AGH_ERR_STATE, binding.AGH_ERR_CAPACITY
    some = np.arange(10, dtype=np.int32)
    points = lambda **k: one.localize_labeled(pts, main["size_left"], ws, k.pop("labels", main["packed"]), k.pop("K", K),
                                              dense=True, **dict(kw, **k))
    depth = lambda **k: one.localize_depth_labeled(images, k.pop("labels", labels), ws, k.pop("K", K), **dict(kw, **k))

    def short_stride():
        """a row stride below the width, through the raw record"""
        recs, keep, _ = binding.depth_image_records(images)
        lrecs, lkeep = binding.label_image_records(labels, False)
        lrecs[0].row_stride_bytes = images[0]["data"].shape[1] - 1
        lp, _, S, _ = one._localize_params(0, ws, None, 60, 8, True, 2, 0.005, 0.003, False, False)
        return one._localize_labeled(one.lib.agh_localize_depth_labeled, (recs, lrecs, C.c_int32(2)), K, lp, S, None)

    calls = {
        "no objects": (bad, lambda: points(K=0)),
        "negative objects": (bad, lambda: depth(K=-1)),
        "65 objects": (bad, lambda: points(K=65)),
        "65 objects, depth": (bad, lambda: depth(K=65)),
        "n_objects x S above 2^24": (bad, lambda: points(K=64, n_samples=(1 << 18) + 1, caps=(1, 1, 1))),
        "labels with sample_idx, points": (bad, lambda: points(samples=some)),
        "labels with sample_idx, depth": (bad, lambda: depth(samples=some)),
        "NULL labels": (bad, lambda: points(labels=None)),
        "NULL label images": (bad, lambda: depth(labels=None)),
        "all-NULL label images": (bad, lambda: depth(labels=[None, None])),
        "short row stride": (bad, short_stride),
        "a twin's validation": (bad, lambda: depth(n_samples=-1)),
    }
    for what, (code, call) in calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == code, (what, str(e.value))
        # nothing queued, nothing bound or changed: no chain to end, the last counts stand, the context still works
        with pytest.raises(binding.AghError) as e:
            one.localize_end()
        assert e.value.code == state, what
        assert np.array_equal(one.label_counts(), M0), what
    _same_objects(depth(), want, "after the refusals")
    plain = binding.Context(main["origins"])
    with pytest.raises(binding.AghError) as e:
        plain.localize_depth_labeled(images, labels, ws, K, **kw)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    # buffers that are too small: every results[j] filled, and the repeat sized from them succeeds
    with pytest.raises(binding.AghError) as e:
        depth(caps=(1, 1, 1))
    assert e.value.code == cap and "agh_localize_labeled" in str(e.value)
    counts = one.last_batch_counts
    assert [r["n_hypotheses"] for r in counts] == [w["n_hypotheses"] for w in want]
    assert [r["n_hands"] for r in counts] == [len(w["hands"]) for w in want]
    assert [r["first_sample"] for r in counts] == [60 * j for j in range(K)]
    sized = (sum(r["n_handles"] for r in counts), sum(r["n_inlier_idx"] for r in counts), sum(r["n_hands"] for r in counts))
    _same_objects(depth(caps=sized), want, "sized from the counts")
    # mid-chain: every labelled call and the counts are refused, the chain in flight is untouched
    labelled_calls = {
        "agh_localize_labeled": points,
        "agh_localize_depth_labeled": depth,
        "agh_get_label_counts": one.label_counts,
    }
    m0 = (main["packed"] == 6).astype(np.uint8)
    mkw = dict(KW, n_samples=100, sample_seed=8)
    chain_want = ref.localize_masked(pts, main["size_left"], ws, m0, dense=True, **mkw)
    one.localize_masked(pts, main["size_left"], ws, m0, dense=True, phase="begin", **mkw)
    for name, call in labelled_calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == state and name + ": " in str(e.value), (name, str(e.value))
    _same(one.localize_end(), chain_want, "after the mid-chain refusals")
    # mid-batch likewise
    batch_want = ref.localize_batch([pts], [main["size_left"]], [ws], n_samples=100, dense=True, **KW)
    one.localize_batch_begin([pts], [main["size_left"]], [ws], n_samples=100, dense=True, **KW)
    for name, call in labelled_calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == state and name + ": " in str(e.value), (name, str(e.value))
    _same(one.localize_batch_end()[0], batch_want[0], "after the mid-batch refusals")
    _same_objects(depth(), want, "at the end")
