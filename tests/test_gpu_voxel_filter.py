"""agh_set_voxel_filter (include/agh.h): voxels without enough occupied neighbours pruned inside the voxeliser.  k_vox_prune is
held, by exact equality, against the numpy model of tests/voxel_filter_cases.py: the filtered cloud is the UNFILTERED cloud with the
model's rows removed, the six counts are the model's; every chain with the filter set is held against the stage-wise calls on the
filtered preprocessing, or against the plain chain on the model's sample lists."""
import ctypes as C

import numpy as np
import pytest

from tests import cluster_cases as CC
from tests import depth_captures as D
from tests import mask_cases as M
from tests import voxel_filter_cases as VF
from tests.test_gpu_boundary_chain import _assert_same, _contexts, _stagewise
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
CASES = VF.cases()
SKIP = -(1 << 31)


def _ctx():
    from agile_grasp_amd import binding

    return binding.Context(np.zeros((2, 3)))


def _preprocess(ctx, c):
    nv = ctx.preprocess(c["points"], c["size_left"], c["workspace"], c["cell"], dense=c["dense"])
    xyz, cam = ctx.cloud() if nv else (np.zeros((0, 3), np.float32), np.zeros(0, np.int32))
    assert len(xyz) == nv
    return xyz, cam


def _fp(c):
    return dict(radius=c["radius"], min_neighbors=c["min_neighbors"])


def _is_filtered(ctx, c, plain, m, what):
    xyz, cam = _preprocess(ctx, c)
    counts = ctx.voxel_filter_counts()
    print(what, "voxels", len(plain[0]), "->", len(xyz), "counts", counts.tolist(), "model", m["counts"].tolist())
    assert np.array_equal(xyz, plain[0][m["keep"]]) and np.array_equal(cam, plain[1][m["keep"]]), what
    assert counts.shape == (1, 6) and np.array_equal(counts[0], m["counts"]), what


@pytest.fixture(scope="module")
def speckle():
    c = VF.speckle_capture()
    cams = VF.case_cams(c)
    m = VF.case_model(c)
    vox = VF.filtered_cloud(c["points"], cams, c["workspace"], c["cell"], m["keep"])
    return dict(c, cams=cams, model=m, vox=vox, fp=_fp(c))


@pytest.mark.parametrize("name", sorted(CASES))
def test_filtered_preprocessing_is_the_unfiltered_cloud_without_the_models_rows(name):
    c = CASES[name]
    m = VF.case_model(c)
    ctx, never = _ctx(), _ctx()
    plain = _preprocess(never, c)
    want = VF.unfiltered_cloud(c["points"], VF.case_cams(c), c["workspace"], c["cell"])
    assert np.array_equal(plain[0], want[0]) and np.array_equal(plain[1], want[1])
    assert never.voxel_filter_counts().shape == (0, 6)
    ctx.set_voxel_filter(**_fp(c))
    _is_filtered(ctx, c, plain, m, name + ", the context's first cloud")
    _is_filtered(ctx, c, plain, m, name + ", the kept bitmaps")  # (the speculative pass, on the two bitmaps swapped)
    ctx.clear_voxel_filter()
    again = _preprocess(ctx, c)
    assert np.array_equal(again[0], plain[0]) and np.array_equal(again[1], plain[1])
    assert ctx.voxel_filter_counts().shape == (0, 6)
    ctx.close()
    never.close()


def test_the_lattice_outgrown_repeat_runs_the_filter_again():
    small, big = CASES["last_word"], CASES["cam1_seams"]
    ctx, never = _ctx(), _ctx()
    ctx.set_voxel_filter(radius=2, min_neighbors=2)
    for c in (small, big, small, CASES["ball_r3"]):
        c = dict(c, radius=2, min_neighbors=2)
        _is_filtered(ctx, c, _preprocess(never, c), VF.case_model(c), "outgrown")
    # ... and inside agh_localize, whose repeat is the whole call
    c = dict(big, radius=2, min_neighbors=2)
    m = VF.case_model(c)
    one = _ctx()
    one.set_voxel_filter(radius=2, min_neighbors=2)
    kw = dict(classify=False, cell_size=c["cell"], dense=True, n_samples=8, sample_seed=3)
    one.localize(small["points"], small["size_left"], small["workspace"], **kw)
    got = one.localize(c["points"], c["size_left"], c["workspace"], **kw)
    assert got["n_voxels"] == m["keep"].sum() and np.array_equal(one.voxel_filter_counts()[0], m["counts"])
    plain = _preprocess(never, c)
    gx, gc = one.cloud()
    assert np.array_equal(gx, plain[0][m["keep"]]) and np.array_equal(gc, plain[1][m["keep"]])
    for x in (ctx, never, one):
        x.close()


def _all_outside(c):
    """the case's points, every one outside the workspace"""
    return dict(c, workspace=np.array([5.0, 6.0, 5.0, 6.0, 5.0, 6.0]))


def test_a_wholly_pruned_capture_behaves_as_one_outside_the_workspace():
    c = CASES["one_voxel"]
    ctx, never = _ctx(), _ctx()
    ctx.set_voxel_filter(**_fp(c))
    kw = dict(classify=False, cell_size=c["cell"], dense=True, n_samples=4, sample_seed=1)
    from agile_grasp_amd.binding import AghError

    def outcome(call):
        try:
            return ("returned", call())
        except AghError as e:
            return ("refused", e.code)

    mine = outcome(lambda: ctx.preprocess(c["points"], c["size_left"], c["workspace"], c["cell"], dense=True))
    theirs = outcome(lambda: never.preprocess(c["points"], c["size_left"], _all_outside(c)["workspace"], c["cell"], dense=True))
    print("agh_preprocess with no voxel left:", mine, theirs)
    assert mine == theirs
    got = ctx.localize(c["points"], c["size_left"], c["workspace"], **kw)
    want = never.localize(c["points"], c["size_left"], _all_outside(c)["workspace"], **kw)
    _same(got, want, "all pruned")
    assert got["n_voxels"] == 0 and len(got["hands"]) == 0 and (got["samples"] == SKIP).all()
    assert ctx.voxel_filter_counts().tolist() == [[1, 0, 1, 0, 0, 0]]
    ctx.close()
    never.close()


def test_batch_of_an_empty_a_wholly_pruned_and_an_ordinary_capture():
    """three lattices in one agh_localize_batch; capture k equals the single filtered call on capture k alone"""
    fp = dict(radius=2, min_neighbors=2)
    empty = dict(CASES["one_voxel"], points=np.zeros((0, 3), np.float32), size_left=0)
    caps = [empty, CASES["one_voxel"], CASES["cam1_seams"], CASES["dense_block"]]
    ctx, single, never = _ctx(), _ctx(), _ctx()
    ctx.set_voxel_filter(**fp)
    single.set_voxel_filter(**fp)
    kw = dict(classify=False, cell_size=VF.CELL, dense=True)
    for rnd in range(2):  # (the second round on the kept slots, swapped)
        got = ctx.localize_batch([c["points"] for c in caps], [c["size_left"] for c in caps], [c["workspace"] for c in caps],
                                 n_samples=[4, 4, 16, 16], sample_seeds=[1, 2, 3, 4], **kw)
        counts = ctx.voxel_filter_counts()
        assert counts.shape == (4, 6)
        gx, gc = ctx.cloud()
        first = 0
        for k, c in enumerate(caps):
            m = VF.case_model(dict(c, **fp))
            want = single.localize(c["points"], c["size_left"], c["workspace"], n_samples=[4, 4, 16, 16][k], sample_seed=k + 1, **kw)
            _same(got[k], want, ("capture", k, rnd))
            assert np.array_equal(counts[k], m["counts"]), (k, rnd)
            assert np.array_equal(single.voxel_filter_counts()[0], m["counts"])
            nv = int(m["keep"].sum())
            assert got[k]["n_voxels"] == nv
            if nv:
                plain = _preprocess(never, c)
                assert np.array_equal(gx[first:first + nv], plain[0][m["keep"]]) and np.array_equal(gc[first:first + nv], plain[1][m["keep"]])
            first += nv
        assert first == len(gx)
    from agile_grasp_amd import binding

    recs = (binding.AghVoxelFilterCounts * 3)()
    assert ctx.lib.agh_get_voxel_filter_counts(ctx._h, recs, C.c_int32(3)) == binding.AGH_ERR_CAPACITY
    # the other captures are untouched by a neighbour: the ordinary ones alone give the same rows
    alone = ctx.localize_batch([caps[2]["points"]], [caps[2]["size_left"]], [caps[2]["workspace"]], n_samples=[16], sample_seeds=[3], **kw)
    _same(alone[0], got[2], "alone")
    for x in (ctx, single, never):
        x.close()


def test_localize_equals_the_stage_wise_calls_on_the_filtered_preprocessing(svm_model, speckle):
    c = speckle
    one, chain = _contexts(c["origins"], svm_model)
    one.set_voxel_filter(**c["fp"])
    chain.set_voxel_filter(**c["fp"])
    got = one.localize(c["points"], c["size_left"], c["workspace"], n_samples=400, sample_seed=3, filters_boundaries=True, **KW)
    gx, gc = one.cloud()
    assert np.array_equal(gx, c["vox"][0]) and np.array_equal(gc, c["vox"][1])
    assert np.array_equal(one.voxel_filter_counts()[0], c["model"]["counts"])
    h, hd, idx, bite = _stagewise(chain, c["points"], c["size_left"], c["workspace"], got["samples"], True)
    print("voxels", got["n_voxels"], "counts", c["model"]["counts"].tolist(), bite)
    assert got["n_voxels"] == len(c["vox"][0]) and got["n_hypotheses"] == bite["n_hyp"] >= 20
    from agile_grasp_amd.binding import draw_samples

    assert np.array_equal(got["samples"], draw_samples(len(c["vox"][0]), 400, 3))  # the strata are the survivors'
    _assert_same(got, h, hd, idx)
    one.close()
    chain.close()


def test_masked_and_labelled_chains_count_surviving_voxels_only(svm_model, speckle):
    """the mask covers the injected points (whose voxels go) and half the scene; the labels give every injected point the OTHER
    half's object: a pruned voxel's point must mark nothing -- with the prune kernel alone it would mark the next surviving voxel"""
    from agile_grasp_amd.binding import labeled_samples, masked_samples

    c = speckle
    one, ref = _contexts(c["origins"], svm_model)
    one.set_voxel_filter(**c["fp"])
    ref.set_voxel_filter(**c["fp"])
    pts, keep = c["points"], c["model"]["keep"]
    with np.errstate(invalid="ignore"):
        low = pts[:, 1] < 0.0
    mask = (low | c["injected"]).astype(np.uint8)
    E = VF.filtered_eligible(pts, c["cams"], mask, c["workspace"], c["cell"], keep)
    E_unfiltered = M.eligible_model(pts, c["cams"], mask, c["workspace"], c["cell"])
    assert len(E) < len(E_unfiltered) - 100  # the mask covers pruned voxels
    kw = dict(KW, n_samples=200, sample_seed=5)
    got = one.localize_masked(pts, c["size_left"], c["workspace"], mask, **kw)
    print("eligible", len(E), "unfiltered", len(E_unfiltered), "hypotheses", got["n_hypotheses"])
    assert one.sample_mask_count() == len(E)
    assert np.array_equal(got["samples"], masked_samples(E, 200, 5))
    _same(got, ref.localize(pts, c["size_left"], c["workspace"], samples=got["samples"], **KW), "masked")
    assert got["n_hypotheses"] >= 10
    labels = np.where(low, 1, 2).astype(np.uint8)
    labels[c["injected"]] = 3 - labels[c["injected"]]
    lists = [VF.filtered_eligible(pts, c["cams"], labels == j + 1, c["workspace"], c["cell"], keep) for j in range(2)]
    gotl = one.localize_labeled(pts, c["size_left"], c["workspace"], labels, 2, **kw)
    print("lists", [len(e) for e in lists], "counts", one.label_counts().tolist())
    assert np.array_equal(one.label_counts(), [len(e) for e in lists])
    assert np.array_equal(np.concatenate([g["samples"] for g in gotl]), labeled_samples(lists, 200, 5))
    for j in range(2):
        _same(gotl[j], ref.localize(pts, c["size_left"], c["workspace"], samples=gotl[j]["samples"], **KW), ("labelled", j))
    # the batch form, two captures: the speckle capture and a lattice case with labels on its pruned voxels
    lat = CASES["seams"]
    lm = VF.case_model(dict(lat, **c["fp"]))
    lat_cams = VF.case_cams(lat)
    lat_labels = (1 + np.arange(len(lat["points"])) % 2).astype(np.uint8)
    lat_lists = [VF.filtered_eligible(lat["points"], lat_cams, lat_labels == j + 1, lat["workspace"], lat["cell"], lm["keep"])
                 for j in range(2)]
    for cell, cap, lab, want_lists in ((c["cell"], c, labels, lists), (lat["cell"], lat, lat_labels, lat_lists)):
        gb = one.localize_batch_labeled([cap["points"], cap["points"]], [cap["size_left"]] * 2, [cap["workspace"]] * 2, [lab, lab],
                                        [2, 2], n_samples=[50, 60], sample_seeds=[5, 6], dense=cap["dense"], cell_size=cell,
                                        classify=False)
        counts = one.batch_label_counts()
        print("batch lists", counts.tolist())
        assert np.array_equal(np.asarray(counts).reshape(-1), [len(e) for e in want_lists] * 2)
        for k, (S, seed) in enumerate(((50, 5), (60, 6))):
            assert np.array_equal(np.concatenate([g["samples"] for g in gb[k]]), labeled_samples(want_lists, S, seed)), k
    one.close()
    ref.close()


def test_clustered_chain_clusters_the_survivors(svm_model):
    xyz, size_left, ws, origins, cp = CC.table_scene()
    pts, size_left, injected = VF.inject(xyz, size_left, ws, 200, 7)
    fp = dict(radius=2, min_neighbors=4)
    cams = M.camera_ids(pts, size_left, True)
    m = VF.filter_model(pts, cams, ws, 0.003, **fp)
    vox = VF.filtered_cloud(pts, cams, ws, 0.003, m["keep"])
    print("table scene: counts", m["counts"].tolist())
    assert m["counts"][2:4].sum() >= 150
    (one,) = _contexts(origins, svm_model, n=1)
    one.set_voxel_filter(**fp)
    from tests.test_gpu_localize_clustered import _check_model, _cp

    got = one.localize_clustered(pts, size_left, ws, _cp(cp), n_samples=20, sample_seed=3, dense=True, **KW)
    mod = _check_model(one, got, cp, 20, 3, vox)
    assert mod["n_objects"] == 3
    assert np.array_equal(one.voxel_filter_counts()[0], m["counts"])
    one.close()


def test_depth_chain_with_both_filters_equals_the_points_chain_on_the_depth_models_points(svm_model):
    from tests import depth_filter_cases as FC

    images, _masks, ws, origins, dfp = FC.injected_main()
    pts, _counts = FC.filter_points(images, dfp)
    one, ref = _contexts(origins, svm_model)
    fp = dict(radius=2, min_neighbors=4)
    for x in (one, ref):
        x.set_voxel_filter(**fp)
    one.set_depth_filter(**dfp)
    kw = dict(KW, n_samples=200, sample_seed=9)
    size_left = images[0]["data"].size
    want = ref.localize(pts, size_left, ws, dense=True, **kw)
    got = one.localize_depth(images, ws, **kw)
    m = VF.filter_model(pts, D.image_index(images), ws, 0.003, **fp)
    print("voxels", got["n_voxels"], "counts", m["counts"].tolist(), "hypotheses", got["n_hypotheses"])
    _same(got, want, "depth")
    assert np.array_equal(one.voxel_filter_counts()[0], m["counts"]) and m["counts"][2:4].sum() > 0
    assert got["n_voxels"] == m["counts"][4:].sum() and len(one.depth_filter_counts()) == len(images)
    one.close()
    ref.close()


def test_a_begin_stage_end_round_and_the_mid_chain_refusals(svm_model, speckle):
    from agile_grasp_amd import binding

    c = speckle
    one, ref = _contexts(c["origins"], svm_model)
    for x in (one, ref):
        x.set_voxel_filter(**c["fp"])
    kw = dict(KW, n_samples=150, sample_seed=4)
    pts = np.array(c["points"])
    want = ref.localize(pts, c["size_left"], c["workspace"], **kw)
    one.localize_begin(pts, c["size_left"], c["workspace"], **kw)
    one.localize_stage(pts)
    for call in (lambda: one.set_voxel_filter(radius=3), one.clear_voxel_filter, one.voxel_filter_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    assert one.voxel_filter().radius == c["fp"]["radius"]  # (the getter is host-side and stays allowed)
    _same(one.localize_end(), want, "first")
    one.localize_begin(pts, c["size_left"], c["workspace"], **kw)  # adopts the staged capture
    _same(one.localize_end(), want, "staged")
    assert np.array_equal(one.voxel_filter_counts()[0], c["model"]["counts"])
    # a batch stream
    caps, sl, ws = [pts, pts[:len(pts) // 2]], [c["size_left"], c["size_left"]], [c["workspace"]] * 2
    bkw = dict(KW, n_samples=[100, 80], sample_seeds=[1, 2])
    bwant = ref.localize_batch(caps, sl, ws, **bkw)
    one.localize_batch_begin(caps, sl, ws, **bkw)
    one.localize_batch_stage(caps)
    for call in (lambda: one.set_voxel_filter(min_neighbors=1), one.clear_voxel_filter, one.voxel_filter_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    got = one.localize_batch_end()
    one.localize_batch_begin(caps, sl, ws, **bkw)
    again = one.localize_batch_end()
    for k in range(2):
        _same(got[k], bwant[k], ("batch chain", k))
        _same(again[k], bwant[k], ("staged batch", k))
    assert np.array_equal(one.voxel_filter_counts(), ref.voxel_filter_counts()) and one.voxel_filter_counts().shape == (2, 6)
    one.set_voxel_filter(radius=3)  # ... and after the end the setter works again
    assert one.voxel_filter().radius == 3
    one.close()
    ref.close()


def test_a_context_whose_filter_was_never_set_is_unchanged(svm_model, speckle):
    """the chain of tests/test_gpu_boundary_chain.py on the speckle capture: the one call against the stage-wise calls, and the
    voxels the unfiltered model's"""
    c = speckle
    one, chain = _contexts(c["origins"], svm_model)
    got = one.localize(c["points"], c["size_left"], c["workspace"], n_samples=300, sample_seed=3, filters_boundaries=True, **KW)
    h, hd, idx, bite = _stagewise(chain, c["points"], c["size_left"], c["workspace"], got["samples"], True)
    _assert_same(got, h, hd, idx)
    want = VF.unfiltered_cloud(c["points"], c["cams"], c["workspace"], c["cell"])
    gx, gc = one.cloud()
    assert np.array_equal(gx, want[0]) and np.array_equal(gc, want[1]) and got["n_voxels"] == len(want[0])
    assert one.voxel_filter() is None and one.voxel_filter_counts().shape == (0, 6)
    one.close()
    chain.close()
