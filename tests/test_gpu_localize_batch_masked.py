"""agh_localize_batch_masked* and agh_localize_depth_batch_masked* (include/agh.h): the batch chains with every capture's samples
drawn under its own mask.  Sample lists, the counts of eligible voxels and the voxelised batch are held against the numpy model
of tests/mask_cases.py on the batches of tests/mask_batch_cases.py; every chain result against agh_localize_masked /
agh_localize_depth_masked per capture and against agh_localize_batch with the reported lists, on other contexts -- exact equality
throughout."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import depth_captures as D
from tests import mask_batch_cases as MB
from tests import mask_cases as M
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
SKIP = -(1 << 31)
POINT_BATCHES = MB.point_batches()


@functools.lru_cache(maxsize=None)
def _point_models(name):
    return [MB.point_model(c) for _, c in POINT_BATCHES[name]]


def _point_args(batch):
    cases = [c for _, c in batch]
    return dict(captures=[c["points"] for c in cases], sizes_left=[c["size_left"] for c in cases],
                workspaces=[c["workspace"] for c in cases], masks=[c["mask"] for c in cases]), dict(
                    dense=[c["dense"] for c in cases], cell_size=cases[0]["cell"])


def _check_model(ctx, got, models, S, seeds, what):
    """got: the batch's list of dicts; models: (E_k, voxel model of capture k) per capture"""
    from agile_grasp_amd.binding import masked_samples

    counts = ctx.batch_mask_counts()
    print(what, "M", [len(E) for E, _ in models], "S", S, "voxels", [len(v[0]) for _, v in models], "hypotheses",
          [g["n_hypotheses"] for g in got])
    assert counts.tolist() == [len(E) for E, _ in models], what
    for k, (E, vox) in enumerate(models):
        assert np.array_equal(got[k]["samples"], masked_samples(E, S[k], seeds[k])), (what, k)
        assert got[k]["n_voxels"] == len(vox[0]), (what, k)
        if len(E) == 0:
            assert got[k]["n_hypotheses"] == 0 and len(got[k]["hands"]) == 0 and len(got[k]["handles"]) == 0, (what, k)
    gx, gc = ctx.cloud()
    assert np.array_equal(gx, np.concatenate([v[0] for _, v in models])), what
    assert np.array_equal(gc, np.concatenate([v[1] for _, v in models])), what


def _run_point_batch(ctx, name, what):
    batch = POINT_BATCHES[name]
    models = _point_models(name)
    args, kw = _point_args(batch)
    S = [MB.n_samples(n, len(E)) for (n, _), (E, _) in zip(batch, models)]
    seeds = [MB.seed(k) for k in range(len(batch))]
    got = ctx.localize_batch_masked(**args, n_samples=S, sample_seeds=seeds, classify=False, **kw)
    _check_model(ctx, got, models, S, seeds, what)
    # the mask stage runs for n_samples = 0 too
    got = ctx.localize_batch_masked(**args, n_samples=0, classify=False, **kw)
    assert ctx.batch_mask_counts().tolist() == [len(E) for E, _ in models], what
    assert [g["n_voxels"] for g in got] == [len(v[0]) for _, v in models] and all(len(g["samples"]) == 0 for g in got), what


@pytest.mark.parametrize("name", sorted(POINT_BATCHES) + sorted(MB.SEQUENCES))
def test_point_batches_equal_the_model(name):
    """Each batch on a fresh context (the lattice-size synchronisation) and again on the same one (the kept slots); a sequence:
    its batches one after the other on one context."""
    from agile_grasp_amd import binding

    ctx = binding.Context(np.zeros((2, 3)))
    for batch in MB.SEQUENCES.get(name, (name, name)):
        _run_point_batch(ctx, batch, f"{name}: {batch}")
    ctx.close()


@pytest.mark.parametrize("name", ["edge", "main"])
def test_depth_batches_equal_the_model(name):
    from agile_grasp_amd import binding

    b = MB.depth_batches()[name]
    caps, masks, wss = b["captures"], b["masks"], b["workspaces"]
    ctx = binding.Context(np.zeros((2, 3)))
    pts = ctx.deproject_batch(caps)
    off = MB.raw_offsets(MB.depth_counts(b))
    models = [MB.depth_model(caps[k], masks[k], wss[k], pts[off[k]:off[k + 1]])[:2] for k in range(len(caps))]
    S = [MB.n_samples("", len(E)) for E, _ in models]
    seeds = [MB.seed(k) for k in range(len(caps))]
    for turn in ("fresh", "kept slots"):
        got = ctx.localize_depth_batch_masked(caps, masks, wss, n_samples=S, sample_seeds=seeds, classify=False)
        _check_model(ctx, got, models, S, seeds, f"{name}, {turn}")
    got = ctx.localize_depth_batch_masked(caps, masks, wss, n_samples=0, classify=False)
    assert ctx.batch_mask_counts().tolist() == [len(E) for E, _ in models] and all(len(g["samples"]) == 0 for g in got)
    ctx.close()


@pytest.fixture(scope="module")
def main():
    """the main batch with its rectangle masks, the captures' model points and packed masks (read-only), and a workspace with a
    face through capture 0's masked object"""
    b = MB.depth_batches()["main"]
    caps, masks, ws = b["captures"], b["masks"], b["workspaces"][0]
    pts = [D.deproject_ref(c) for c in caps]
    for p in pts:
        p.setflags(write=False)
    packed = [M.packed_masks(c, m) for c, m in zip(caps, masks)]
    obj = pts[0][(packed[0] != 0) & np.isfinite(pts[0]).all(1)]
    ws_cut = ws.copy()
    ws_cut[1] = np.median(obj[:, 0]) + 0.01
    return dict(caps=caps, masks=masks, ws=ws, ws_cut=ws_cut, origins=b["origins"], pts=pts, packed=packed,
                sizes=[c[0]["data"].size for c in caps], n=len(caps))


def _floors(want, what):
    print(what, "hypotheses", [w["n_hypotheses"] for w in want], "hands", [len(w["hands"]) for w in want], "handles",
          [len(w["handles"]) for w in want])
    assert all(w["n_hypotheses"] >= 20 and len(w["hands"]) >= 1 for w in want), what


@pytest.mark.parametrize("mode", ["classified", "boundaries"])
def test_chain_equality(svm_model, main, mode):
    """The masked batch, depth and points form, per capture against the masked call and against agh_localize_batch with the
    reported lists.  S = 300, seed 7 + k.  Capture 0 is tests/test_gpu_localize_masked.py's own case (340 hypotheses, 206 kept
    hands with the classifier; 441 and 292 with the workspace cut).  The other captures' counts, from the CPU oracle
    (oracle_py.find_hands and classify on the voxel models, with the lists the numpy model draws), classified mode:
    capture 1: 316 hypotheses, 183 kept hands (M = 5682); 2: 306, 168 (5635); 3: 281, 143 (5645); 4 (image 0 only): 349, 166
    (5685); 5 (capture 2 in float32 metres): 306, 160 (5635).  The floors below ask every capture's reference for work."""
    n = main["n"]
    one, two, ref, flat = _contexts(main["origins"], svm_model, n=4)
    ws = main["ws"] if mode == "classified" else main["ws_cut"]
    kw = dict(KW, filters_boundaries=mode == "boundaries")
    seeds = [7 + k for k in range(n)]
    got = one.localize_depth_batch_masked(main["caps"], main["masks"], ws, n_samples=300, sample_seeds=seeds, **kw)
    counts = one.batch_mask_counts()
    pts = [np.array(p) for p in main["pts"]]
    got_p = two.localize_batch_masked(pts, main["sizes"], ws, main["packed"], n_samples=300, sample_seeds=seeds, dense=True, **kw)
    assert np.array_equal(two.batch_mask_counts(), counts)
    singles = []
    for k in range(n):
        want = ref.localize_depth_masked(main["caps"][k], main["masks"][k], ws, n_samples=300, sample_seed=seeds[k], **kw)
        assert ref.sample_mask_count() == counts[k] > 300  # (M_k >= S: every stratum holds a voxel)
        singles.append(want)
        _same(got[k], want, f"{mode}: depth batch against the depth masked call, capture {k}")
        want_p = ref.localize_masked(pts[k], main["sizes"][k], ws, main["packed"][k], n_samples=300, sample_seed=seeds[k], dense=True, **kw)
        _same(got_p[k], want_p, f"{mode}: points batch against the masked call, capture {k}")
    _floors(singles, mode)
    listed = flat.localize_batch(pts, main["sizes"], ws, samples=[g["samples"] for g in got], dense=True, **kw)
    for k in range(n):
        _same(got[k], listed[k], f"{mode}: depth batch against the batch with explicit lists, capture {k}")
        _same(got_p[k], listed[k], f"{mode}: points batch against the batch with explicit lists, capture {k}")


def test_identity_masks_equal_the_drawn_batch(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    n = main["n"]
    pts = [np.array(p) for p in main["pts"]]
    seeds = [21 + k for k in range(n)]
    kw = dict(KW, n_samples=200, sample_seeds=seeds)
    want = ref.localize_batch(pts, main["sizes"], main["ws"], dense=True, **kw)
    _floors(want, "all ones")
    got = one.localize_batch_masked(pts, main["sizes"], main["ws"], [np.ones(len(p), np.uint8) for p in pts], dense=True, **kw)
    assert one.batch_mask_counts().tolist() == [w["n_voxels"] for w in want]
    ones = [[np.ones(im["data"].shape, np.uint8) for im in c] for c in main["caps"]]
    got_d = one.localize_depth_batch_masked(main["caps"], ones, main["ws"], **kw)
    for k in range(n):
        _same(got[k], want[k], f"all ones, points, capture {k}")
        _same(got_d[k], want[k], f"all ones, depth, capture {k}")


def _device_slice(a, offset):
    """`a` (uint8, any shape) in device memory, `offset` bytes into its allocation, rows 3 bytes longer than they are wide"""
    import torch

    a2 = a.reshape(1, -1) if a.ndim == 1 else a
    wide = np.full((a2.shape[0], a2.shape[1] + (3 if a.ndim == 2 else 0)), 9, np.uint8)
    wide[:, :a2.shape[1]] = a2
    flat = torch.from_numpy(np.concatenate([np.full(offset, 9, np.uint8), wide.reshape(-1), np.full(5, 9, np.uint8)])).cuda()
    view = flat[offset:offset + wide.size].view(wide.shape)[:, :a2.shape[1]]
    assert view.data_ptr() == flat.data_ptr() + offset
    return (view[0] if a.ndim == 1 else view), flat


def test_device_forms_with_masks_at_byte_offsets(svm_model, main):
    """captures and masks as torch tensors on the GPU, every mask a slice that starts 1, 2 or 3 bytes into its allocation"""
    import torch

    from agile_grasp_amd import binding

    for name in ("cm", "mm_rotated"):
        batch = POINT_BATCHES[name]
        host, dev = (binding.Context(np.zeros((2, 3))) for _ in range(2))
        args, kw = _point_args(batch)
        models = _point_models(name)
        S = [MB.n_samples(n, len(E)) for (n, _), (E, _) in zip(batch, models)]
        seeds = [MB.seed(k) for k in range(len(batch))]
        want = host.localize_batch_masked(**args, n_samples=S, sample_seeds=seeds, classify=False, **kw)
        keep = [_device_slice(m, 1 + k % 3) for k, m in enumerate(args["masks"])]
        d_args = dict(args, captures=[torch.from_numpy(p).cuda() for p in args["captures"]], masks=[v for v, _ in keep])
        got = dev.localize_batch_masked(**d_args, n_samples=S, sample_seeds=seeds, classify=False, **kw)
        _check_model(dev, got, models, S, seeds, f"device points, {name}")
        for k in range(len(batch)):
            _same(got[k], want[k], f"device points, {name}, capture {k}")
        host.close()
        dev.close()
    n = main["n"]
    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=250, sample_seeds=[31 + k for k in range(n)])
    want = ref.localize_depth_batch_masked(main["caps"], main["masks"], main["ws"], **kw)
    _floors(want, "device depth")
    d_caps, d_masks, keep = [], [], []
    for k, (images, masks) in enumerate(zip(main["caps"], main["masks"])):
        d_images = []
        for im in images:
            d = im["data"]
            full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
            full[:, :d.shape[1]] = d
            t = torch.from_numpy(full.view(np.int16) if d.dtype == np.uint16 else full).cuda()
            d_images.append(dict(im, data=t[:, :d.shape[1]]))
        d_caps.append(d_images)
        views = [None if m is None else _device_slice(np.asarray(m), 1 + k % 3) for m in masks]
        keep.append(views)
        d_masks.append([None if v is None else v[0] for v in views])
    got = one.localize_depth_batch_masked(d_caps, d_masks, main["ws"], **kw)
    assert np.array_equal(one.batch_mask_counts(), ref.batch_mask_counts())
    pts = [torch.from_numpy(np.array(p)).cuda() for p in main["pts"]]
    packed = [_device_slice(m, 1 + k % 3) for k, m in enumerate(main["packed"])]
    got_p = one.localize_batch_masked(pts, main["sizes"], main["ws"], [v for v, _ in packed], dense=True, **kw)
    assert np.array_equal(one.batch_mask_counts(), ref.batch_mask_counts())
    for k in range(n):
        _same(got[k], want[k], f"device depth, capture {k}")
        _same(got_p[k], want[k], f"device points of the depth captures, capture {k}")


def test_begin_and_end(svm_model, main):
    from agile_grasp_amd import binding

    n = main["n"]
    one, ref, fresh = _contexts(main["origins"], svm_model, n=3)
    kw = dict(KW, n_samples=250, sample_seeds=[41 + k for k in range(n)])
    pts = [np.array(p) for p in main["pts"]]
    want = ref.localize_depth_batch_masked(main["caps"], main["masks"], main["ws"], **kw)
    counts = ref.batch_mask_counts()
    _floors(want, "begin + end")
    one.localize_depth_batch_masked_begin(main["caps"], main["masks"], main["ws"], **kw)
    pending = one._batch_pending
    # a second begin in flight, of either form, and the getter: AGH_ERR_STATE, the chain untouched
    refused = {
        "agh_localize_depth_batch_masked_begin": lambda: one.localize_depth_batch_masked_begin(main["caps"], main["masks"], main["ws"], **kw),
        "agh_localize_batch_masked_begin": lambda: one.localize_batch_masked_begin(pts, main["sizes"], main["ws"], main["packed"], dense=True, **kw),
        "agh_localize_depth_batch_masked": lambda: one.localize_depth_batch_masked(main["caps"], main["masks"], main["ws"], **kw),
        "agh_localize_batch_masked": lambda: one.localize_batch_masked(pts, main["sizes"], main["ws"], main["packed"], dense=True, **kw),
        "agh_get_batch_mask_counts": one.batch_mask_counts,
    }
    for name, call in refused.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE and name + ": " in str(e.value), (name, str(e.value))
        one._batch_pending = pending
    got = one.localize_batch_end()
    for k in range(n):
        _same(got[k], want[k], f"depth begin + end, capture {k}")
    assert np.array_equal(one.batch_mask_counts(), counts)
    one.localize_batch_masked_begin(pts, main["sizes"], main["ws"], main["packed"], dense=True, **kw)
    got = one.localize_batch_end()
    for k in range(n):
        _same(got[k], want[k], f"points begin + end, capture {k}")
    # a pending staged set is dropped by a masked host begin; the results do not change
    staged = one.localize_batch_stage(pts)
    one.localize_batch_masked_begin(staged, main["sizes"], main["ws"], main["packed"], dense=True, **kw)
    got = one.localize_batch_end()
    for k in range(n):
        _same(got[k], want[k], f"staged set dropped, capture {k}")
    assert np.array_equal(one.batch_mask_counts(), counts)
    # an unmasked batch afterwards: what a fresh context returns, and the counts are gone
    plain_kw = dict(KW, n_samples=120, sample_seeds=[51 + k for k in range(n)], dense=True)
    plain = fresh.localize_batch(pts, main["sizes"], main["ws"], **plain_kw)
    got = one.localize_batch(pts, main["sizes"], main["ws"], **plain_kw)
    for k in range(n):
        _same(got[k], plain[k], f"unmasked after masked, capture {k}")
    for ctx in (one, fresh):
        with pytest.raises(binding.AghError) as e:
            ctx.batch_mask_counts()
        assert e.value.code == binding.AGH_ERR_STATE
    # ... and after a masked batch the single chains' getters have nothing
    one.localize_batch_masked(pts, main["sizes"], main["ws"], main["packed"], dense=True, **kw)
    for getter in (one.sample_mask_count, one.label_counts):
        with pytest.raises(binding.AghError) as e:
            getter()
        assert e.value.code == binding.AGH_ERR_STATE
    # ... and a single masked chain takes the batch's counts away
    one.localize_depth_masked(main["caps"][0], main["masks"][0], main["ws"], n_samples=50, **KW)
    with pytest.raises(binding.AghError) as e:
        one.batch_mask_counts()
    assert e.value.code == binding.AGH_ERR_STATE


def test_the_outgrown_slot_repeat_inside_a_masked_batch(svm_model, main):
    """A small-extent batch sizes the context's bitmap slots; the wide one's lattices outgrow them and the batch is run once more
    inside the call, with the masks where the first pass left them.  Host depth form and device points form."""
    import torch

    one, dev, ref = _contexts(main["origins"], svm_model, n=3)
    caps, masks, ws = main["caps"][:3], main["masks"][:3], main["ws"]
    kw = dict(KW, n_samples=200, sample_seeds=[6, 7, 8])
    mid = 0.5 * (ws[0::2] + ws[1::2])
    half = 0.08 * (ws[1::2] - ws[0::2])
    small = np.stack([mid - half, mid + half], axis=1).reshape(6)
    ones = [[np.ones(im["data"].shape, np.uint8) for im in c] for c in caps]
    first = one.localize_depth_batch_masked(caps, ones, small, **kw)
    assert all(f["n_voxels"] > 100 for f in first) and one.batch_mask_counts().tolist() == [f["n_voxels"] for f in first]
    builds = one.grid_stats()["builds"]
    got = one.localize_depth_batch_masked(caps, masks, ws, **kw)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the batch twice: the lattices outgrew the kept slots)
    want = ref.localize_depth_batch_masked(caps, masks, ws, **kw)
    _floors(want, "outgrown")
    assert np.array_equal(one.batch_mask_counts(), ref.batch_mask_counts())
    for k in range(3):
        _same(got[k], want[k], f"repeat, host depth, capture {k}")
    d_pts = [torch.from_numpy(np.array(p)).cuda() for p in main["pts"][:3]]
    d_ones = [torch.ones(len(p), dtype=torch.uint8).cuda() for p in d_pts]
    d_masks = [torch.from_numpy(m).cuda() for m in main["packed"][:3]]
    dev.localize_batch_masked(d_pts, main["sizes"][:3], small, d_ones, dense=True, **kw)
    builds = dev.grid_stats()["builds"]
    got = dev.localize_batch_masked(d_pts, main["sizes"][:3], ws, d_masks, dense=True, **kw)
    assert dev.grid_stats()["builds"] - builds == 2 and np.array_equal(dev.batch_mask_counts(), ref.batch_mask_counts())
    for k in range(3):
        _same(got[k], want[k], f"repeat, device points, capture {k}")


def test_errors_leave_the_context_usable(svm_model, main):
    from agile_grasp_amd import binding

    n = main["n"]
    one, ref = _contexts(main["origins"], svm_model)
    caps, masks, ws = main["caps"], main["masks"], main["ws"]
    pts = [np.array(p) for p in main["pts"]]
    kw = dict(KW, n_samples=200, sample_seeds=[61 + k for k in range(n)])
    want = ref.localize_depth_batch_masked(caps, masks, ws, **kw)
    counts = ref.batch_mask_counts()
    got = one.localize_depth_batch_masked(caps, masks, ws, **kw)
    bad, state, capacity = binding.AGH_ERR_INVALID_ARGUMENT, binding.AGH_ERR_STATE, binding.AGH_ERR_CAPACITY
    some = np.arange(10, dtype=np.int32)

    def short_stride(begin=False):
        """capture 2's image 0 mask with a row stride below the width, through the raw records"""
        a = one._depth_batch_masked_args(caps, masks, ws, dict(kw))
        a["mrecs"][4].row_stride_bytes = caps[2][0]["data"].shape[1] - 1
        if begin:
            return one._check(one.lib.agh_localize_depth_batch_masked_begin(one._h, a["recs"], a["mrecs"], a["n_images"], a["lps"],
                                                                            C.c_int32(a["Ck"])))
        return one._batch_collect(a, None, lambda *o: one.lib.agh_localize_depth_batch_masked(
            one._h, a["recs"], a["mrecs"], a["n_images"], a["lps"], C.c_int32(a["Ck"]), *o))

    def with_one(seq, k, v):
        out = list(seq)
        out[k] = v
        return out

    lists = [None] * n
    lists[3] = some
    calls = {
        "a NULL mask of one capture": ("capture 2", lambda: one.localize_batch_masked(pts, main["sizes"], ws, with_one(main["packed"], 2, None), dense=True, **kw)),
        "a NULL mask, begin": ("capture 2", lambda: one.localize_batch_masked_begin(pts, main["sizes"], ws, with_one(main["packed"], 2, None), dense=True, **kw)),
        "NULL masks, points": ("masks is NULL", lambda: one.localize_batch_masked(pts, main["sizes"], ws, None, dense=True, **kw)),
        "NULL masks, depth": ("masks is NULL", lambda: one.localize_depth_batch_masked(caps, None, ws, **kw)),
        "all-NULL records of one capture": ("capture 1", lambda: one.localize_depth_batch_masked(caps, with_one(masks, 1, [None, None]), ws, **kw)),
        "all-NULL records, begin": ("capture 1", lambda: one.localize_depth_batch_masked_begin(caps, with_one(masks, 1, [None, None]), ws, **kw)),
        "a stride below the width": ("capture 2, image 0", short_stride),
        "a stride below the width, begin": ("capture 2, image 0", lambda: short_stride(True)),
        "sample_idx with a mask, depth": ("capture 3", lambda: one.localize_depth_batch_masked(caps, masks, ws, samples=lists, n_samples=200, **KW)),
        "sample_idx with a mask, points": ("capture 3", lambda: one.localize_batch_masked(pts, main["sizes"], ws, main["packed"], samples=lists, n_samples=200, dense=True, **KW)),
        "a twin's validation": ("capture 0", lambda: one.localize_depth_batch_masked(caps, masks, ws, n_samples=-1, **KW)),
    }
    epoch = one.epoch()
    for what, (text, call) in calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == bad and text in str(e.value), (what, str(e.value))
        one._batch_pending = None
        # nothing launched, nothing queued: the epoch stands, there is no chain to end, the last counts stand
        assert one.epoch() == epoch, what
        with pytest.raises(binding.AghError) as e:
            one.localize_batch_end()
        assert e.value.code == state, what
        assert np.array_equal(one.batch_mask_counts(), counts), what
    # cap_captures too small
    with pytest.raises(binding.AghError) as e:
        one.batch_mask_counts(cap_captures=n - 1)
    assert e.value.code == capacity
    # output buffers too small: AGH_ERR_CAPACITY with every results[k] filled, then the call again with the sizes reported
    with pytest.raises(binding.AghError) as e:
        one.localize_depth_batch_masked(caps, masks, ws, caps=(1, 1, 1), **kw)
    assert e.value.code == capacity
    reported = one.last_batch_counts
    assert [r["n_hypotheses"] for r in reported] == [w["n_hypotheses"] for w in want]
    assert [r["n_hands"] for r in reported] == [len(w["hands"]) for w in want]
    assert [r["n_handles"] for r in reported] == [len(w["handles"]) for w in want]
    assert np.array_equal(one.batch_mask_counts(), counts)
    sizes = tuple(sum(r[f] for r in reported) for f in ("n_handles", "n_inlier_idx", "n_hands"))
    again = one.localize_depth_batch_masked(caps, masks, ws, caps=sizes, **kw)
    plain = binding.Context(main["origins"])
    with pytest.raises(binding.AghError) as e:
        plain.localize_depth_batch_masked(caps, masks, ws, **kw)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    final = one.localize_batch_masked(pts, main["sizes"], ws, main["packed"], dense=True, **kw)
    for k in range(n):
        _same(got[k], want[k], f"before the errors, capture {k}")
        _same(again[k], want[k], f"with the sizes reported, capture {k}")
        _same(final[k], want[k], f"after the errors, capture {k}")
