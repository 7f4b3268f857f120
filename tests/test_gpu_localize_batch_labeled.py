"""agh_localize_batch_labeled* and agh_localize_depth_batch_labeled* (include/agh.h): the batch chains with one sample list per
object of every capture's label image.  Sample lists, the counts of eligible voxels and the voxelised batch are held against the
numpy model of tests/label_cases.py on the batches of tests/label_batch_cases.py; every chain result against
agh_localize_labeled / agh_localize_depth_labeled per capture, agh_localize_masked per object and agh_localize_batch_masked, on
other contexts -- exact equality throughout."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import depth_captures as D
from tests import label_batch_cases as LB
from tests import label_cases as L
from tests import mask_batch_cases as MB
from tests import mask_cases as M
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
SKIP = -(1 << 31)
POINT_BATCHES = LB.point_batches()
TILES = ((3, 4), (2, 2), (1, 1), (2, 3), (1, 2), (1, 3))  # rows x columns of image 0's tiling, capture after capture
N_OBJECTS = [r * c for r, c in TILES]  # 12, 4, 1, 6, 2, 3: 28 lists


@functools.lru_cache(maxsize=None)
def _point_models(name):
    return [LB.point_model(c) for _, c in POINT_BATCHES[name]]


def _point_args(batch):
    cases = [c for _, c in batch]
    return dict(captures=[c["points"] for c in cases], sizes_left=[c["size_left"] for c in cases],
                workspaces=[c["workspace"] for c in cases], labels=[c["labels"] for c in cases],
                n_objects=[c["n_objects"] for c in cases]), dict(dense=[c["dense"] for c in cases], cell_size=cases[0]["cell"])


def _check_model(ctx, got, models, S, seeds, what):
    """got: per capture a list of dicts per object; models: ([E_{k,0} ..], voxel model of capture k) per capture"""
    from agile_grasp_amd.binding import batch_labeled_samples

    ms = [len(e) for E, _ in models for e in E]
    print(what, "M", ms, "S", S, "voxels", [len(v[0]) for _, v in models], "hypotheses", [g["n_hypotheses"] for objs in got for g in objs])
    assert ctx.batch_label_counts().tolist() == ms, what
    assert [len(objs) for objs in got] == [len(E) for E, _ in models], what
    drawn = [g["samples"] for objs in got for g in objs]
    assert np.array_equal(np.concatenate(drawn), batch_labeled_samples([E for E, _ in models], S, seeds)), what
    for k, (E, vox) in enumerate(models):
        for j, e in enumerate(E):
            g = got[k][j]
            assert g["n_voxels"] == len(vox[0]) and len(g["samples"]) == S[k], (what, k, j)
            if len(e) == 0:
                assert (g["samples"] == SKIP).all() and g["n_hypotheses"] == 0 and len(g["hands"]) == 0 and len(g["handles"]) == 0, (what, k, j)
    gx, gc = ctx.cloud()
    assert np.array_equal(gx, np.concatenate([v[0] for _, v in models])), what
    assert np.array_equal(gc, np.concatenate([v[1] for _, v in models])), what


def _run_point_batch(ctx, name, what):
    batch = POINT_BATCHES[name]
    models = _point_models(name)
    args, kw = _point_args(batch)
    S = [LB.n_samples(n, [len(e) for e in E]) for (n, _), (E, _) in zip(batch, models)]
    seeds = [LB.seed(k) for k in range(len(batch))]
    got = ctx.localize_batch_labeled(**args, n_samples=S, sample_seeds=seeds, classify=False, **kw)
    _check_model(ctx, got, models, S, seeds, what)
    # the label stage runs for n_samples = 0 too
    got = ctx.localize_batch_labeled(**args, n_samples=0, classify=False, **kw)
    _check_model(ctx, got, models, [0] * len(batch), seeds, what + ", S = 0")


@pytest.mark.parametrize("name", sorted(POINT_BATCHES) + sorted(LB.SEQUENCES))
def test_point_batches_equal_the_model(name):
    """Each batch on a fresh context (the lattice-size synchronisation) and again on the same one (the kept slots); a sequence:
    its batches one after the other on one context."""
    from agile_grasp_amd import binding

    ctx = binding.Context(np.zeros((2, 3)))
    for batch in LB.SEQUENCES.get(name, (name, name)):
        _run_point_batch(ctx, batch, f"{name}: {batch}")
    ctx.close()


def test_samples_around_the_counts():
    """S_k one below the shortest list of capture k, equal to its longest, one above it, and beyond twice it"""
    from agile_grasp_amd import binding

    batch = POINT_BATCHES["mm"]
    models = _point_models("mm")
    args, kw = _point_args(batch)
    ctx = binding.Context(np.zeros((2, 3)))
    lens = [[len(e) for e in E] for E, _ in models]
    assert all(min(m) > 5 for m in lens)
    for turn, S in enumerate(([min(m) - 1 for m in lens], [max(m) for m in lens], [max(m) + 1 for m in lens],
                              [2 * max(m) + 3 for m in lens], [min(lens[0]) - 1, 2 * max(lens[1]) + 3])):
        seeds = [S[0] + 5, turn + 1]
        got = ctx.localize_batch_labeled(**args, n_samples=S, sample_seeds=seeds, classify=False, **kw)
        _check_model(ctx, got, models, S, seeds, f"S = {S}")
    ctx.close()


@pytest.fixture(scope="module")
def main():
    """the main depth batch (6 captures) with image 0 tiled differently per capture (12, 4, 1, 6, 2 and 3 objects) and image 1's
    labels NULL; the captures' model points and packed labels (read-only); a workspace with a face through capture 0's last tile"""
    caps, ws, origins = MB.DB.main_batch()
    pts = [D.deproject_ref(c) for c in caps]
    for p in pts:
        p.setflags(write=False)
    labels = [[L.tiled_labels(c[0]["data"].shape, r, q), None][:len(c)] for c, (r, q) in zip(caps, TILES)]
    packed = [M.packed_masks(c, m) for c, m in zip(caps, labels)]
    tile = pts[0][(packed[0] == 12) & np.isfinite(pts[0]).all(1)]
    ws_cut = ws.copy()
    ws_cut[1] = np.median(tile[:, 0]) + 0.01
    return dict(caps=caps, labels=labels, ws=ws, ws_cut=ws_cut, origins=origins, pts=pts, packed=packed,
                sizes=[c[0]["data"].size for c in caps], n=len(caps), K=list(N_OBJECTS))


def _floors(want, what):
    """want: per capture the labelled reference's list of dicts"""
    print(what, "hypotheses", [[w["n_hypotheses"] for w in objs] for objs in want], "hands", [[len(w["hands"]) for w in objs] for objs in want],
          "handles", [[len(w["handles"]) for w in objs] for objs in want])
    assert all(max(w["n_hypotheses"] for w in objs) >= 20 for objs in want), what
    assert sum(len(w["handles"]) for objs in want for w in objs) >= 2, what


def _same_objects(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (what, "object", j))


def _labeled_references(ref, main, ws, kw, seeds, form="depth"):
    out, counts = [], []
    for k in range(main["n"]):
        if form == "depth":
            out.append(ref.localize_depth_labeled(main["caps"][k], main["labels"][k], ws, main["K"][k], sample_seed=seeds[k], **kw))
        else:
            out.append(ref.localize_labeled(np.array(main["pts"][k]), main["sizes"][k], ws, main["packed"][k], main["K"][k], dense=True,
                                            sample_seed=seeds[k], **kw))
        counts += ref.label_counts().tolist()
    return out, counts


@pytest.mark.parametrize("mode", ["classified", "boundaries"])
def test_chain_equality(svm_model, main, mode):
    """The labelled batch, depth and points form, per capture against the labelled call on that capture alone, and for captures
    1 and 3 per object against agh_localize_masked with the mask labels == j + 1.  Image 0 of the six captures of the main depth
    batch is tiled 3 x 4, 2 x 2, 1 x 1, 2 x 3, 1 x 2 and 1 x 3 (28 lists), image 1's labels are NULL; S = 100 per object, seed
    7 + k, the classifier on, min_inliers = 2; "boundaries": filters_boundaries with the +x face of the workspace through capture
    0's last tile.  Hypotheses per list with the CPU oracle (oracle_py.find_hands on the voxel models, with the lists the numpy
    model draws; "classified" workspace), and the eligible voxels M:
      capture 0 (tests/test_gpu_localize_labeled.py's own case): 69 47 49 104 77 41 94 50 0 117 99 79 (object 8: M = 0; the others
                 M = 700 .. 5669)
      capture 1: 44 45 97 95 (M = 3960 .. 11166);  capture 2: 58 (M = 30663);  capture 3: 48 33 65 83 121 38 (M = 1203 .. 8040);
      capture 4 (image 0 only): 91 80 (M = 15050, 15572);  capture 5 (capture 2 in float32 metres): 49 82 45 (M = 8178 .. 13539)
    The labelled references report the same counts, and 41 handles in all.  The floors below are conditions on the references
    alone: every capture's has an object with 20 hypotheses or more, and the references hold two handles or more in all."""
    n = main["n"]
    one, two, ref = _contexts(main["origins"], svm_model, n=3)
    ws = main["ws"] if mode == "classified" else main["ws_cut"]
    kw = dict(KW, n_samples=100, filters_boundaries=mode == "boundaries")
    seeds = [7 + k for k in range(n)]
    got = one.localize_depth_batch_labeled(main["caps"], main["labels"], ws, main["K"], sample_seeds=seeds, **kw)
    counts = one.batch_label_counts().tolist()
    pts = [np.array(p) for p in main["pts"]]
    got_p = two.localize_batch_labeled(pts, main["sizes"], ws, main["packed"], main["K"], sample_seeds=seeds, dense=True, **kw)
    assert two.batch_label_counts().tolist() == counts and len(counts) == sum(main["K"]) == 28
    want, want_counts = _labeled_references(ref, main, ws, kw, seeds, "depth")
    _floors(want, mode)
    assert counts == want_counts
    want_p, _ = _labeled_references(ref, main, ws, kw, seeds, "points")
    for k in range(n):
        _same_objects(got[k], want[k], f"{mode}: depth batch against the depth labelled call, capture {k}")
        _same_objects(got_p[k], want_p[k], f"{mode}: points batch against the labelled call, capture {k}")
    first = LB.first_lists([(None, dict(n_objects=K)) for K in main["K"]])
    for k in (1, 3):
        for j in range(main["K"][k]):
            mask = (main["packed"][k] == j + 1).astype(np.uint8)
            twin = ref.localize_masked(pts[k], main["sizes"][k], ws, mask, n_samples=100, sample_seed=seeds[k], dense=True,
                                       **dict(KW, filters_boundaries=mode == "boundaries"))
            assert ref.sample_mask_count() == counts[first[k] + j]
            _same(got[k][j], twin, f"{mode}: against the masked call, capture {k}, object {j}")


def test_one_object_batches_equal_the_masked_batch(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    n = main["n"]
    masks = [[MB.depth_batches()["main"]["masks"][k][0], None][:len(c)] for k, c in enumerate(main["caps"])]
    kw = dict(KW, n_samples=200, sample_seeds=[5 + k for k in range(n)])
    want = ref.localize_depth_batch_masked(main["caps"], masks, main["ws"], **kw)
    got = one.localize_depth_batch_labeled(main["caps"], masks, main["ws"], [1] * n, **kw)
    assert all(w["n_hypotheses"] >= 20 for w in want)
    assert one.batch_label_counts().tolist() == ref.batch_mask_counts().tolist()
    for k in range(n):
        assert len(got[k]) == 1
        _same(got[k][0], want[k], f"one object per capture, capture {k}")


def test_a_batch_of_one_capture_equals_the_labelled_call(svm_model, main):
    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=100)
    for k in (0, 4):
        want = ref.localize_depth_labeled(main["caps"][k], main["labels"][k], main["ws"], main["K"][k], sample_seed=3, **kw)
        got = one.localize_depth_batch_labeled([main["caps"][k]], [main["labels"][k]], main["ws"], [main["K"][k]], sample_seeds=[3], **kw)
        assert len(got) == 1 and max(w["n_hypotheses"] for w in want) >= 20
        assert one.batch_label_counts().tolist() == ref.label_counts().tolist()
        _same_objects(got[0], want, f"a batch of capture {k} alone")


def _device_labels(a, offset):
    """`a` ((N,) uint8) in device memory, `offset` bytes into its allocation, other labels on either side"""
    import torch

    t = torch.from_numpy(np.concatenate([np.full(offset, 1, np.uint8), a, np.full(5, 1, np.uint8)])).cuda()
    view = t[offset:offset + len(a)]
    assert view.data_ptr() == t.data_ptr() + offset
    return view


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_device_points_and_labels_at_byte_offsets(svm_model, main, offset):
    import torch

    from agile_grasp_amd import binding

    for name in ("cm_small", "mm_reversed"):
        batch = POINT_BATCHES[name]
        dev = binding.Context(np.zeros((2, 3)))
        args, kw = _point_args(batch)
        models = _point_models(name)
        S = [LB.n_samples(n, [len(e) for e in E]) for (n, _), (E, _) in zip(batch, models)]
        seeds = [LB.seed(k) for k in range(len(batch))]
        d_args = dict(args, captures=[torch.from_numpy(p).cuda() for p in args["captures"]],
                      labels=[_device_labels(m, (offset + k) % 4 if offset else 0) for k, m in enumerate(args["labels"])])
        got = dev.localize_batch_labeled(**d_args, n_samples=S, sample_seeds=seeds, classify=False, **kw)
        _check_model(dev, got, models, S, seeds, f"device points, {name}, offset {offset}")
        dev.close()
    n = main["n"]
    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=60, sample_seeds=[31 + k for k in range(n)], dense=True)
    pts = [np.array(p) for p in main["pts"]]
    want = ref.localize_batch_labeled(pts, main["sizes"], main["ws"], main["packed"], main["K"], **kw)
    assert sum(w["n_hypotheses"] for objs in want for w in objs) >= 100
    got = one.localize_batch_labeled([torch.from_numpy(p).cuda() for p in pts], main["sizes"], main["ws"],
                                     [_device_labels(m, offset) for m in main["packed"]], main["K"], **kw)
    assert one.batch_label_counts().tolist() == ref.batch_label_counts().tolist()
    for k in range(n):
        _same_objects(got[k], want[k], f"device points of the depth captures, offset {offset}, capture {k}")


def test_device_depth_labels_with_padded_rows_and_an_odd_base(svm_model, main):
    import torch

    n = main["n"]
    one, ref = _contexts(main["origins"], svm_model)
    kw = dict(KW, n_samples=60, sample_seeds=[41 + k for k in range(n)])
    want = ref.localize_depth_batch_labeled(main["caps"], main["labels"], main["ws"], main["K"], **kw)
    assert sum(w["n_hypotheses"] for objs in want for w in objs) >= 100
    d_caps, d_labels, keep = [], [], []
    for k, (images, labels) in enumerate(zip(main["caps"], main["labels"])):
        d_images, d_lab = [], []
        for im, m in zip(images, labels):
            d = im["data"]
            full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
            full[:, :d.shape[1]] = d
            t = torch.from_numpy(full.view(np.int16) if d.dtype == np.uint16 else full).cuda()
            d_images.append(dict(im, data=t[:, :d.shape[1]]))
            if m is None:
                d_lab.append(None)
                continue
            base = 1 + 2 * (k % 2)  # an odd base: 1 or 3 bytes into the allocation; rows 3 bytes longer than they are wide
            wide = np.full((m.shape[0], m.shape[1] + 3), 9, np.uint8)
            wide[:, :m.shape[1]] = m
            flat = torch.from_numpy(np.concatenate([np.full(base, 9, np.uint8), wide.reshape(-1)])).cuda()
            view = flat[base:].view(wide.shape)[:, :m.shape[1]]
            assert view.data_ptr() % 2 == 1 and view.stride(0) == m.shape[1] + 3
            keep.append(flat)
            d_lab.append(view)
        d_caps.append(d_images)
        d_labels.append(d_lab)
    got = one.localize_depth_batch_labeled(d_caps, d_labels, main["ws"], main["K"], **kw)
    assert one.batch_label_counts().tolist() == ref.batch_label_counts().tolist()
    for k in range(n):
        _same_objects(got[k], want[k], f"device depth, capture {k}")


def test_begin_and_end(svm_model, main):
    from agile_grasp_amd import binding

    n = main["n"]
    one, ref, fresh = _contexts(main["origins"], svm_model, n=3)
    kw = dict(KW, n_samples=80, sample_seeds=[51 + k for k in range(n)])
    pts = [np.array(p) for p in main["pts"]]
    caps, labels, ws, K = main["caps"], main["labels"], main["ws"], main["K"]
    want = ref.localize_depth_batch_labeled(caps, labels, ws, K, **kw)
    counts = ref.batch_label_counts().tolist()
    _floors(want, "begin + end")
    one.localize_depth_batch_labeled_begin(caps, labels, ws, K, **kw)
    pending = one._batch_pending
    # a second begin in flight, of either form, the blocking calls and the getter: AGH_ERR_STATE, the chain untouched
    refused = {
        "agh_localize_depth_batch_labeled_begin": lambda: one.localize_depth_batch_labeled_begin(caps, labels, ws, K, **kw),
        "agh_localize_batch_labeled_begin": lambda: one.localize_batch_labeled_begin(pts, main["sizes"], ws, main["packed"], K, dense=True, **kw),
        "agh_localize_depth_batch_labeled": lambda: one.localize_depth_batch_labeled(caps, labels, ws, K, **kw),
        "agh_localize_batch_labeled": lambda: one.localize_batch_labeled(pts, main["sizes"], ws, main["packed"], K, dense=True, **kw),
        "agh_get_batch_label_counts": one.batch_label_counts,
    }
    for name, call in refused.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE and name + ": " in str(e.value), (name, str(e.value))
        one._batch_pending = pending
    got = one.localize_batch_end()
    for k in range(n):
        _same_objects(got[k], want[k], f"depth begin + end, capture {k}")
    assert one.batch_label_counts().tolist() == counts
    one.localize_batch_labeled_begin(pts, main["sizes"], ws, main["packed"], K, dense=True, **kw)
    got = one.localize_batch_end()
    for k in range(n):
        _same_objects(got[k], want[k], f"points begin + end, capture {k}")
    # a pending staged set is dropped by a labelled host begin; the results do not change
    staged = one.localize_batch_stage(pts)
    one.localize_batch_labeled_begin(staged, main["sizes"], ws, main["packed"], K, dense=True, **kw)
    got = one.localize_batch_end()
    for k in range(n):
        _same_objects(got[k], want[k], f"staged set dropped, capture {k}")
    assert one.batch_label_counts().tolist() == counts
    # the counts getters: after a labelled batch the other three have nothing ...
    for getter in (one.sample_mask_count, one.label_counts, one.batch_mask_counts):
        with pytest.raises(binding.AghError) as e:
            getter()
        assert e.value.code == binding.AGH_ERR_STATE
    with pytest.raises(binding.AghError) as e:
        one.batch_label_counts(cap_lists=len(counts) - 1)
    assert e.value.code == binding.AGH_ERR_CAPACITY
    # ... and after any other chain this one has nothing: a fresh context, an unmasked batch (which equals a fresh context's), a
    # masked batch, a labelled single chain, a masked single chain
    with pytest.raises(binding.AghError) as e:
        fresh.batch_label_counts()
    assert e.value.code == binding.AGH_ERR_STATE
    plain_kw = dict(KW, n_samples=120, sample_seeds=[61 + k for k in range(n)], dense=True)
    plain = fresh.localize_batch(pts, main["sizes"], ws, **plain_kw)
    got = one.localize_batch(pts, main["sizes"], ws, **plain_kw)
    for k in range(n):
        _same(got[k], plain[k], f"unlabelled after labelled, capture {k}")
    others = {
        "unmasked batch": lambda: None,
        "masked batch": lambda: one.localize_batch_masked(pts[:2], main["sizes"][:2], ws, [(p != 0).astype(np.uint8) for p in main["packed"][:2]],
                                                         n_samples=20, dense=True, **KW),
        "labelled single": lambda: one.localize_depth_labeled(caps[0], labels[0], ws, K[0], n_samples=20, **KW),
        "masked single": lambda: one.localize_depth_masked(caps[0], [(labels[0][0] == 1).astype(np.uint8), None], ws, n_samples=20, **KW),
    }
    for what, call in others.items():
        call()
        with pytest.raises(binding.AghError) as e:
            one.batch_label_counts()
        assert e.value.code == binding.AGH_ERR_STATE, what
        one.localize_depth_batch_labeled(caps[:2], labels[:2], ws, K[:2], n_samples=10, **KW)
        assert one.batch_label_counts().tolist() == counts[:K[0] + K[1]], what


def test_the_outgrown_slot_repeat_inside_a_labelled_batch(svm_model, main):
    """A small-extent batch sizes the context's bitmap slots; the wide one's lattices outgrow them and the batch is run once more
    inside the call, with the labels where the first pass left them.  Host depth form and device points form."""
    import torch

    one, dev, ref = _contexts(main["origins"], svm_model, n=3)
    caps, labels, ws, K = main["caps"][:3], main["labels"][:3], main["ws"], main["K"][:3]
    kw = dict(KW, n_samples=80, sample_seeds=[6, 7, 8])
    mid = 0.5 * (ws[0::2] + ws[1::2])
    half = 0.08 * (ws[1::2] - ws[0::2])
    small = np.stack([mid - half, mid + half], axis=1).reshape(6)
    first = one.localize_depth_batch_labeled(caps, labels, small, K, **kw)
    assert all(objs[0]["n_voxels"] > 100 for objs in first)
    builds = one.grid_stats()["builds"]
    got = one.localize_depth_batch_labeled(caps, labels, ws, K, **kw)
    assert one.grid_stats()["builds"] - builds == 2  # (the call ran the batch twice: the lattices outgrew the kept slots)
    want = ref.localize_depth_batch_labeled(caps, labels, ws, K, **kw)
    _floors(want, "outgrown")
    assert one.batch_label_counts().tolist() == ref.batch_label_counts().tolist()
    for k in range(3):
        _same_objects(got[k], want[k], f"repeat, host depth, capture {k}")
    d_pts = [torch.from_numpy(np.array(p)).cuda() for p in main["pts"][:3]]
    d_labels = [torch.from_numpy(m).cuda() for m in main["packed"][:3]]
    dev.localize_batch_labeled(d_pts, main["sizes"][:3], small, d_labels, K, dense=True, **kw)
    builds = dev.grid_stats()["builds"]
    got = dev.localize_batch_labeled(d_pts, main["sizes"][:3], ws, d_labels, K, dense=True, **kw)
    assert dev.grid_stats()["builds"] - builds == 2 and dev.batch_label_counts().tolist() == ref.batch_label_counts().tolist()
    for k in range(3):
        _same_objects(got[k], want[k], f"repeat, device points, capture {k}")


def test_errors_leave_the_context_usable(svm_model, main):
    from agile_grasp_amd import binding

    n = main["n"]
    one, ref = _contexts(main["origins"], svm_model)
    caps, labels, ws, K = main["caps"], main["labels"], main["ws"], main["K"]
    pts = [np.array(p) for p in main["pts"]]
    kw = dict(KW, n_samples=60, sample_seeds=[71 + k for k in range(n)])
    want = ref.localize_depth_batch_labeled(caps, labels, ws, K, **kw)
    counts = ref.batch_label_counts().tolist()
    got = one.localize_depth_batch_labeled(caps, labels, ws, K, **kw)
    bad, state, capacity = binding.AGH_ERR_INVALID_ARGUMENT, binding.AGH_ERR_STATE, binding.AGH_ERR_CAPACITY
    some = np.arange(10, dtype=np.int32)

    def short_stride(begin=False):
        """capture 2's image 0 label image with a row stride below the width, through the raw records"""
        a = one._depth_batch_labeled_args(caps, labels, ws, K, dict(kw))
        a["mrecs"][4].row_stride_bytes = caps[2][0]["data"].shape[1] - 1
        if begin:
            return one._check(one.lib.agh_localize_depth_batch_labeled_begin(one._h, a["recs"], a["mrecs"], a["n_images"], a["n_obj"],
                                                                             a["lps"], C.c_int32(a["n_captures"])))
        return one._batch_labeled_collect(a, None, lambda *o: one.lib.agh_localize_depth_batch_labeled(
            one._h, a["recs"], a["mrecs"], a["n_images"], a["n_obj"], a["lps"], C.c_int32(a["n_captures"]), *o))

    def with_one(seq, k, v):
        out = list(seq)
        out[k] = v
        return out

    lists = [None] * n
    lists[3] = some
    points = lambda **over: one.localize_batch_labeled(pts, main["sizes"], ws, **{**dict(labels=main["packed"], n_objects=K, dense=True, **kw), **over})
    depth = lambda **over: one.localize_depth_batch_labeled(caps, **{**dict(labels=labels, workspaces=ws, n_objects=K, **kw), **over})
    calls = {
        "65 lists": ("capture 5", lambda: depth(n_objects=[12, 12, 12, 12, 12, 5])),
        "65 lists, begin": ("capture 5", lambda: one.localize_depth_batch_labeled_begin(caps, labels, ws, [12, 12, 12, 12, 12, 5], **kw)),
        "n_objects = 0": ("capture 2", lambda: depth(n_objects=with_one(K, 2, 0))),
        "n_objects = 65": ("capture 4", lambda: points(n_objects=with_one(K, 4, 65))),
        "NULL n_objects": ("n_objects is NULL", lambda: points(n_objects=None)),
        "a NULL label array of one capture": ("capture 2", lambda: points(labels=with_one(main["packed"], 2, None))),
        "a NULL label array, begin": ("capture 2", lambda: one.localize_batch_labeled_begin(pts, main["sizes"], ws, with_one(main["packed"], 2, None), K, dense=True, **kw)),
        "NULL labels, points": ("labels is NULL", lambda: points(labels=None)),
        "NULL labels, depth": ("labels is NULL", lambda: depth(labels=None)),
        "all-NULL records of one capture": ("capture 1", lambda: depth(labels=with_one(labels, 1, [None, None]))),
        "all-NULL records, begin": ("capture 1", lambda: one.localize_depth_batch_labeled_begin(caps, with_one(labels, 1, [None, None]), ws, K, **kw)),
        "a stride below the width": ("capture 2, image 0", short_stride),
        "a stride below the width, begin": ("capture 2, image 0", lambda: short_stride(True)),
        "sample_idx with labels, depth": ("capture 3", lambda: one.localize_depth_batch_labeled(caps, labels, ws, K, samples=lists, n_samples=60, **KW)),
        "sample_idx with labels, points": ("capture 3", lambda: one.localize_batch_labeled(pts, main["sizes"], ws, main["packed"], K, samples=lists, n_samples=60, dense=True, **KW)),
        "more than 2^24 samples": ("capture 2", lambda: depth(n_samples=1 << 20)),  # (12 + 4) x 2^20 = 2^24 is allowed
        "a twin's validation": ("capture 0", lambda: depth(n_samples=-1)),
    }
    epoch = one.epoch()

    def nothing_happened(what):
        one._batch_pending = None
        # nothing launched, nothing queued: the epoch stands, there is no chain to end, the last counts stand
        assert one.epoch() == epoch, what
        with pytest.raises(binding.AghError) as e:
            one.localize_batch_end()
        assert e.value.code == state, what
        assert one.batch_label_counts().tolist() == counts, what

    for what, (text, call) in calls.items():
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == bad and text in str(e.value), (what, str(e.value))
        nothing_happened(what)
    # a camera-origin table with a row per LIST: origins are per capture
    one.set_cloud_cam_origins(np.stack([main["origins"]] * sum(K)))
    with pytest.raises(binding.AghError) as e:
        depth()
    assert e.value.code == bad
    nothing_happened("a camera-origin table with L rows")
    one.set_cloud_cam_origins(np.stack([main["origins"]] * n))
    tabled = depth()
    one.set_cloud_cam_origins(None)
    # output buffers too small: AGH_ERR_CAPACITY with every results[l] filled, then the call again with the sizes reported
    with pytest.raises(binding.AghError) as e:
        depth(caps=(1, 1, 1))
    assert e.value.code == capacity
    reported = one.last_batch_counts
    flat = [w for objs in want for w in objs]
    assert len(reported) == len(flat) == sum(K)
    assert [r["n_hypotheses"] for r in reported] == [w["n_hypotheses"] for w in flat]
    assert [r["n_hands"] for r in reported] == [len(w["hands"]) for w in flat]
    assert [r["n_handles"] for r in reported] == [len(w["handles"]) for w in flat]
    assert [r["first_sample"] for r in reported] == [60 * l for l in range(len(flat))]
    assert one.batch_label_counts().tolist() == counts
    sizes = tuple(sum(r[f] for r in reported) for f in ("n_handles", "n_inlier_idx", "n_hands"))
    assert sizes[2] >= 1
    again = depth(caps=sizes)
    plain = binding.Context(main["origins"])
    with pytest.raises(binding.AghError) as e:
        plain.localize_depth_batch_labeled(caps, labels, ws, K, **kw)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    final = points()
    for k in range(n):
        _same_objects(got[k], want[k], f"before the errors, capture {k}")
        _same_objects(tabled[k], want[k], f"with the context's origins in a table of n_captures rows, capture {k}")
        _same_objects(again[k], want[k], f"with the sizes reported, capture {k}")
        _same_objects(final[k], want[k], f"after the errors, capture {k}")
