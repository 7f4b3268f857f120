"""agh_set_depth_filter (include/agh.h): flying pixels, speckles and out-of-range readings rejected inside the deprojection.
k_deproject_filtered and k_deproject_filtered_batch are held bit for bit -- values, NaN pattern and the four counts per view --
against the float32 numpy model of tests/depth_filter_cases.py; every depth chain with the filter set is held, by exact equality,
against its points form on the model's points (stride 12, size_left = W0 x H0, dense = 1) on a second context that has no filter."""
import ctypes as C

import numpy as np
import pytest

from tests import cluster_cases as CC
from tests import depth_captures as D
from tests import depth_filter_cases as FC
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same
from tests.test_gpu_localize_clustered import _depth_scene
from tests.test_gpu_localize_depth import _bits

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
CASES = FC.cases()
LOOSE = FC.params(max_jump_abs=0.04, min_support=3)  # for the 64 x 48 table scene, whose pixels lie 1.3 cm apart


def _equal_points(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, int(diff.sum()))


@pytest.fixture(scope="module")
def inj():
    """the injected main case, the model's points with and without the filter, and the voxel models (read-only)"""
    images, masks, ws, origins, fp = FC.injected_main()
    pts, counts = FC.filter_points(images, fp)
    plain = D.deproject_ref(images)
    for a in (pts, plain):
        a.setflags(write=False)
    cams = D.image_index(images)
    return dict(images=images, masks=masks, ws=ws, origins=origins, fp=fp, pts=pts, counts=counts, plain=plain, cams=cams,
                size_left=images[0]["data"].size, vox=D.voxel_model(pts, cams, ws), vox_plain=D.voxel_model(plain, cams, ws))


@pytest.mark.parametrize("name", sorted(CASES))
def test_filtered_deprojection_equals_the_model(name):
    from agile_grasp_amd import binding

    case = CASES[name]
    ctx = binding.Context(np.zeros((2, 3)))
    ctx.set_depth_filter(**case["fp"])
    held = ctx.depth_filter()
    assert {k: getattr(held, k) for k in case["fp"]} == case["fp"]
    want, counts = FC.filter_points(case["images"], case["fp"])
    got = ctx.deproject(case["images"])
    got_counts = ctx.depth_filter_counts()
    print(name, "points", len(want), "counts", counts.tolist(), "got", got_counts.tolist())
    _equal_points(got, want, name)
    assert np.array_equal(got_counts, counts)
    ctx.close()


def test_batch_deprojection_equals_the_model_capture_by_capture():
    from agile_grasp_amd import binding

    caps, fp = FC.batch_captures()
    assert sorted({len(c) for c in caps}) == [1, 2]
    ctx, single = binding.Context(np.zeros((2, 3))), binding.Context(np.zeros((2, 3)))
    for c in (ctx, single):
        c.set_depth_filter(**fp)
    got = ctx.deproject_batch(caps)
    counts = ctx.depth_filter_counts()
    models = [FC.filter_points(images, fp) for images in caps]
    _equal_points(got, np.concatenate([m[0] for m in models]), "batch")
    assert np.array_equal(counts, np.concatenate([m[1] for m in models]))  # launch order: capture k's views behind capture k - 1's
    first = 0
    for k, images in enumerate(caps):
        one = single.deproject(images)
        _equal_points(got[first:first + len(one)], one, ("capture", k))
        assert np.array_equal(single.depth_filter_counts(), models[k][1]), k
        first += len(one)
    small = (binding.AghDepthFilterCounts * 2)()
    assert ctx.lib.agh_get_depth_filter_counts(ctx._h, small, C.c_int32(2)) == binding.AGH_ERR_CAPACITY
    # the same batch without the filter, on the same context: the plain kernel, and no counts
    ctx.clear_depth_filter()
    _equal_points(ctx.deproject_batch(caps), np.concatenate([D.deproject_ref(images) for images in caps]), "unfiltered batch")
    assert ctx.depth_filter_counts().shape == (0, 4)
    ctx.close()
    single.close()


@pytest.mark.parametrize("form", ["host", "device", "staged"])
def test_depth_chain_equals_the_points_chain_on_the_models_points(svm_model, inj, form):
    import torch

    one, ref = _contexts(inj["origins"], svm_model)
    kw = dict(KW, n_samples=200, sample_seed=9)
    want = ref.localize(np.array(inj["pts"]), inj["size_left"], inj["ws"], dense=True, **kw)
    print(form, "voxels", want["n_voxels"], "hypotheses", want["n_hypotheses"], "hands", len(want["hands"]))
    assert want["n_hypotheses"] >= 20 and want["n_voxels"] == len(inj["vox"][0])
    one.set_depth_filter(**inj["fp"])
    if form == "host":
        got = one.localize_depth(inj["images"], inj["ws"], **kw)
    elif form == "device":
        dev = []
        for im in inj["images"]:  # rows padded, read in place with their strides
            d = im["data"]
            full = np.zeros((d.shape[0], d.strides[0] // d.itemsize), d.dtype)
            full[:, :d.shape[1]] = d
            t = torch.from_numpy(full.view(np.int16)).cuda()
            dev.append(dict(im, data=t[:, :d.shape[1]], keep=t))
        got = one.localize_depth(dev, inj["ws"], **kw)
    else:
        # staged while NO filter is set: the stage is a pure copy, and the filter set when the adopting begin deprojects counts
        one.clear_depth_filter()
        one.localize_depth_begin(inj["images"][:1], inj["ws"], **kw)
        one.localize_depth_stage(inj["images"])
        one.localize_end()
        assert one.depth_filter_counts().shape == (0, 4)
        one.set_depth_filter(**inj["fp"])
        saved = [np.array(im["data"]) for im in inj["images"]]
        one.localize_depth_begin(inj["images"], inj["ws"], **kw)  # adopted: same pixel arrays
        got = one.localize_end()
        assert all(np.array_equal(s, im["data"]) for s, im in zip(saved, inj["images"]))
    _same(got, want, form)
    assert np.array_equal(one.depth_filter_counts(), inj["counts"])
    gx, gc = one.cloud()
    assert np.array_equal(gx, inj["vox"][0]) and np.array_equal(gc, inj["vox"][1])
    one.close()
    ref.close()


def test_masked_and_labelled_depth_forms_equal_their_points_forms(svm_model, inj):
    one, ref = _contexts(inj["origins"], svm_model)
    one.set_depth_filter(**inj["fp"])
    kw = dict(KW, n_samples=200, sample_seed=5)
    shape0 = inj["images"][0]["data"].shape
    n1 = inj["images"][1]["data"].size
    m0 = np.zeros(shape0, np.uint8)
    m0[80:160, 120:200] = 1
    packed = np.concatenate([m0.reshape(-1), np.zeros(n1, np.uint8)])
    want = ref.localize_masked(np.array(inj["pts"]), inj["size_left"], inj["ws"], packed, dense=True, **kw)
    got = one.localize_depth_masked(inj["images"], [m0, None], inj["ws"], **kw)
    assert want["n_hypotheses"] >= 20 and one.sample_mask_count() == ref.sample_mask_count()
    _same(got, want, "masked")
    lab0 = np.zeros(shape0, np.uint8)
    lab0[:120, :160], lab0[:120, 160:], lab0[120:, :160], lab0[120:, 160:] = 1, 2, 3, 4
    packed = np.concatenate([lab0.reshape(-1), np.zeros(n1, np.uint8)])
    want = ref.localize_labeled(np.array(inj["pts"]), inj["size_left"], inj["ws"], packed, 4, dense=True, **kw)
    got = one.localize_depth_labeled(inj["images"], [lab0, None], inj["ws"], 4, **kw)
    assert sum(w["n_hypotheses"] for w in want) >= 20 and np.array_equal(one.label_counts(), ref.label_counts())
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("labelled", j))
    assert np.array_equal(one.depth_filter_counts(), inj["counts"])
    one.close()
    ref.close()


def test_clustered_and_fitted_depth_forms_equal_their_points_forms(svm_model):
    from agile_grasp_amd import binding

    xyz, size_left, ws, origins, cp = CC.table_scene()
    images, dcp = _depth_scene(dict(xyz=xyz, size_left=size_left, cp=cp))
    pts, counts = FC.filter_points(images, LOOSE)
    print("table scene: counts", counts.tolist())
    assert (counts[:, 2] > 0).all() and (counts[:, 3] > 10 * counts[:, 2]).all()  # the filter bites, and leaves a scene
    one, ref = _contexts(origins, svm_model)
    one.set_depth_filter(**LOOSE)
    kw = dict(KW, n_samples=20, sample_seed=3)
    want = ref.localize_clustered(pts, images[0]["data"].size, ws, binding.cluster_params(**dcp), dense=True, **kw)
    got = one.localize_depth_clustered(images, ws, binding.cluster_params(**dcp), **kw)
    assert ref.cluster_info()["n_objects"] >= 1 and np.array_equal(one.cluster_labels(), ref.cluster_labels())
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("clustered", j))
    assert np.array_equal(one.depth_filter_counts(), counts)
    fp = dict(distance_threshold=0.006, seed=5, n_candidates=64)
    want = ref.localize_clustered_fit(pts, images[0]["data"].size, ws, binding.plane_fit_params(**fp), binding.cluster_params(**dcp),
                                      dense=True, **kw)
    got = one.localize_depth_clustered_fit(images, ws, binding.plane_fit_params(**fp), binding.cluster_params(**dcp), **kw)
    assert ref.plane_fit()["found"] and np.array_equal(one.plane_fit()["plane"], ref.plane_fit()["plane"])
    assert np.array_equal(one.cluster_labels(), ref.cluster_labels())
    for j, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("fitted", j))
    one.close()
    ref.close()


def test_depth_batch_forms_equal_their_points_forms(svm_model, inj):
    one, ref = _contexts(inj["origins"], svm_model)
    one.set_depth_filter(**inj["fp"])
    caps = [inj["images"], inj["images"][:1]]
    n0 = inj["size_left"]
    pts = [np.array(inj["pts"]), np.array(inj["pts"][:n0])]
    ws = [inj["ws"], inj["ws"]]
    kw = dict(KW, n_samples=[200, 150], sample_seeds=[3, 4])
    want = ref.localize_batch(pts, [n0, n0], ws, dense=True, **kw)
    got = one.localize_depth_batch(caps, ws, **kw)
    assert all(w["n_hypotheses"] >= 20 for w in want)
    for k in range(2):
        _same(got[k], want[k], ("batch", k))
    assert np.array_equal(one.depth_filter_counts(), np.concatenate([inj["counts"], inj["counts"][:1]]))
    lab0 = np.zeros(inj["images"][0]["data"].shape, np.uint8)
    lab0[:, :160], lab0[:, 160:] = 1, 2
    n1 = inj["images"][1]["data"].size
    packed = [np.concatenate([lab0.reshape(-1), np.zeros(n1, np.uint8)]), lab0.reshape(-1)]
    kw = dict(KW, n_samples=[100, 100], sample_seeds=[5, 6])
    want = ref.localize_batch_labeled(pts, [n0, n0], ws, packed, [2, 2], dense=True, **kw)
    got = one.localize_depth_batch_labeled(caps, [[lab0, None], [lab0]], ws, [2, 2], **kw)
    assert sum(w["n_hypotheses"] for objs in want for w in objs) >= 20
    for k in range(2):
        for j in range(2):
            _same(got[k][j], want[k][j], ("labelled batch", k, j))
    one.close()
    ref.close()


def test_the_setting_is_sticky_and_clears_to_the_unfiltered_call(svm_model, inj):
    one, never = _contexts(inj["origins"], svm_model)
    kw = dict(KW, n_samples=200, sample_seed=2)
    assert one.depth_filter() is None and one.depth_filter_counts().shape == (0, 4)
    one.set_depth_filter(**inj["fp"])
    a = one.localize_depth(inj["images"], inj["ws"], **kw)
    _equal_points(one.deproject(inj["images"]), inj["pts"], "between the chains")  # it survives clouds and chains
    b = one.localize_depth(inj["images"], inj["ws"], **kw)
    _same(a, b, "twice")
    assert np.array_equal(one.depth_filter_counts(), inj["counts"])
    one.clear_depth_filter()
    assert one.depth_filter() is None
    plain = one.localize_depth(inj["images"], inj["ws"], **kw)
    assert one.depth_filter_counts().shape == (0, 4)  # the last deprojection ran unfiltered
    _same(plain, never.localize_depth(inj["images"], inj["ws"], **kw), "cleared")
    _equal_points(one.deproject(inj["images"]), never.deproject(inj["images"]), "cleared")
    _equal_points(one.deproject(inj["images"]), inj["plain"], "cleared, against the model")
    one.close()
    never.close()


def test_the_setter_is_refused_mid_chain_and_leaves_the_chain_alone(svm_model, inj):
    from agile_grasp_amd import binding

    one, ref = _contexts(inj["origins"], svm_model)
    kw = dict(KW, n_samples=200, sample_seed=4)
    one.set_depth_filter(**inj["fp"])
    ref.set_depth_filter(**inj["fp"])
    want = ref.localize_depth(inj["images"], inj["ws"], **kw)
    one.localize_depth_begin(inj["images"], inj["ws"], **kw)
    for call in (lambda: one.set_depth_filter(radius=2), one.clear_depth_filter, one.depth_filter_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    assert one.depth_filter().radius == 1  # (the getter is host-side and stays allowed)
    _same(one.localize_end(), want, "single chain")
    caps, ws = [inj["images"], inj["images"][:1]], [inj["ws"], inj["ws"]]
    bkw = dict(KW, n_samples=[200, 100], sample_seeds=[1, 2])
    bwant = ref.localize_depth_batch(caps, ws, **bkw)
    one.localize_depth_batch_begin(caps, ws, **bkw)
    for call in (lambda: one.set_depth_filter(min_support=1), one.clear_depth_filter, one.depth_filter_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    got = one.localize_batch_end()
    for k in range(2):
        _same(got[k], bwant[k], ("batch chain", k))
    assert np.array_equal(one.depth_filter_counts(), ref.depth_filter_counts())
    one.set_depth_filter(radius=2)  # ... and after the end the setter works again
    assert one.depth_filter().radius == 2
    one.close()
    ref.close()


def test_every_refusal_names_its_field_and_keeps_the_old_filter():
    from agile_grasp_amd import binding

    case = CASES["f32_65x17_r2_s3"]
    ctx = binding.Context(np.zeros((2, 3)))
    ctx.set_depth_filter(**case["fp"])
    want, counts = FC.filter_points(case["images"], case["fp"])
    nan, inf = float("nan"), float("inf")
    bad = (("radius", (0, 3, -1)), ("min_support", (0, 25, -2)), ("max_jump_abs", (-0.001, nan, inf)),
           ("max_jump_rel", (-1.0, nan, inf)), ("z_min", (-0.1, nan, inf)), ("z_max", (case["fp"]["z_min"], 0.0, nan, -inf)))
    for field, values in bad:
        for v in values:
            with pytest.raises(binding.AghError) as e:
                ctx.set_depth_filter(**dict(case["fp"], **{field: v}))
            assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "agh_set_depth_filter: " + field in str(e.value), (field, v)
    with pytest.raises(binding.AghError) as e:  # (2 r + 1)^2 - 1 follows the radius
        ctx.set_depth_filter(radius=1, min_support=9)
    assert "min_support" in str(e.value)
    held = ctx.depth_filter()
    assert {k: getattr(held, k) for k in case["fp"]} == case["fp"]
    _equal_points(ctx.deproject(case["images"]), want, "after the refusals")
    assert np.array_equal(ctx.depth_filter_counts(), counts)
    ctx.close()


def test_the_filter_changes_the_voxel_count_of_the_injected_case(svm_model, inj):
    (one,) = _contexts(inj["origins"], svm_model, n=1)
    kw = dict(KW, n_samples=200, sample_seed=7)
    plain = one.localize_depth(inj["images"], inj["ws"], **kw)
    one.set_depth_filter(**inj["fp"])
    filtered = one.localize_depth(inj["images"], inj["ws"], **kw)
    print("voxels: unfiltered", plain["n_voxels"], "filtered", filtered["n_voxels"], "hypotheses", plain["n_hypotheses"],
          filtered["n_hypotheses"])
    assert plain["n_voxels"] == len(inj["vox_plain"][0]) and filtered["n_voxels"] == len(inj["vox"][0])
    assert plain["n_voxels"] != filtered["n_voxels"]
    one.close()
