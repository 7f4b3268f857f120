"""agh_set_voxel_filter (include/agh.h) in the masked, labelled and clustered batch chains: k_mask_mark_batch and
k_label_mark_batch against each capture's own pruned bitmap slot, the cluster and plane-fit stages on a pruned batch, the life
cycle of the batch's second set of bitmap slots, the batch streams and the depth batch forms.  The batches and their models are
tests/voxel_filter_batch_cases.py's -- the existing numpy models composed -- and tests/test_voxel_filter_batch_cases.py proves
that a kernel which read another capture's slot, or let a pruned voxel's point mark, would give other lists on them.  Exact
equality throughout: integers, and floats bit for bit through _same."""
import functools

import numpy as np
import pytest

from tests import depth_captures as D
from tests import mask_cases as M
from tests import plane_fit_batch_cases as PB
from tests import plane_fit_cases as PF
from tests import voxel_filter_batch_cases as VB
from tests import voxel_filter_cases as VF
from tests.test_gpu_boundary_chain import _contexts
from tests.test_gpu_localize_batch import _same
from tests.test_gpu_localize_batch_clustered import _check_models as _check_given_plane
from tests.test_gpu_localize_batch_clustered import _same_batch
from tests.test_gpu_localize_batch_clustered_fit import _call_cases as _call_fitted
from tests.test_gpu_localize_batch_clustered_fit import _check_models as _check_fitted
from tests.test_gpu_localize_batch_clustered_fit import _cps, _fps, _same_candidates, _same_fit

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)
LKW = dict(classify=False, cell_size=VF.CELL, dense=True)  # the lattice batches: tiny, the classifier off
SKIP = -(1 << 31)
# the batches every test iterates over whole, forwards (False) and reversed (True)
LATTICE = {rev: VB.lattice_batch(rev) for rev in (False, True)}
BRIDGED = {rev: VB.bridged_batch(rev) for rev in (False, True)}
NO_VOXEL = ("empty", "one_voxel")  # no point, and wholly pruned


def _ctx(fp=None, origins=None):
    from agile_grasp_amd import binding

    ctx = binding.Context(np.zeros((2, 3)) if origins is None else origins)
    if fp is not None:
        ctx.set_voxel_filter(**fp)
    return ctx


def _close(*ctxs):
    for c in ctxs:
        c.close()


def _same_capture(got, want, what):
    """one capture of a batch: a dict of the masked form, a list of dicts per object of the labelled one"""
    if isinstance(got, list):
        _same_batch([got], [want], what)
    else:
        _same(got, want, what)


def _masked_plan(batch, filtered=True):
    """(models, S, seeds) of a lattice batch in the masked form"""
    models = [VB.masked_model(c, filtered=filtered) for _, c in batch]
    return models, [VB.masked_samples_of(n, len(E)) for (n, _), (E, _) in zip(batch, models)], [VB.seed(k) for k in range(len(batch))]


def _labeled_plan(batch, filtered=True):
    models = [VB.labeled_model(c, filtered=filtered) for _, c in batch]
    S = [VB.labeled_samples_of(n, [len(e) for e in E]) for (n, _), (E, _) in zip(batch, models)]
    return models, S, [VB.seed(k) for k in range(len(batch))]


def _masked_call(ctx, batch, S, seeds, f=None):
    f = ctx.localize_batch_masked if f is None else f
    return f(**VB.args(batch), masks=[c["mask"] for _, c in batch], n_samples=S, sample_seeds=seeds, **LKW)


def _labeled_call(ctx, batch, S, seeds, f=None):
    f = ctx.localize_batch_labeled if f is None else f
    return f(**VB.args(batch), labels=[c["labels"] for _, c in batch], n_objects=[c["n_objects"] for _, c in batch], n_samples=S,
             sample_seeds=seeds, **LKW)


def _check_filter_counts(ctx, batch, filtered, what):
    counts = ctx.voxel_filter_counts()
    if not filtered:
        assert counts.shape == (0, 6), what
        return
    assert counts.shape == (len(batch), 6), what
    for k, (name, c) in enumerate(batch):
        assert np.array_equal(counts[k], c["model"]["counts"]), (what, k, name, counts[k].tolist(), c["model"]["counts"].tolist())


def _check_cloud(ctx, batch, clouds, what):
    """the bound cloud slice by slice: capture k's rows are its model's"""
    gx, gc = ctx.cloud() if sum(len(v[0]) for v in clouds) else (np.zeros((0, 3), np.float32), np.zeros(0, np.int32))
    first = 0
    for k, ((name, _c), (xyz, cams)) in enumerate(zip(batch, clouds)):
        assert np.array_equal(gx[first:first + len(xyz)], xyz) and np.array_equal(gc[first:first + len(xyz)], cams), (what, k, name)
        first += len(xyz)
    assert first == len(gx), what


def _check_masked(ctx, batch, got, plan, what, filtered=True):
    from agile_grasp_amd.binding import masked_samples

    models, S, seeds = plan
    counts = ctx.batch_mask_counts().tolist()
    print(what, "M", counts, "model", [len(E) for E, _ in models], "S", S, "voxels", [g["n_voxels"] for g in got])
    assert len(got) == len(batch) == len(counts), what
    wrong = [(k, name, counts[k], len(E)) for k, ((name, _c), (E, _v)) in enumerate(zip(batch, models)) if counts[k] != len(E)]
    assert not wrong, (what, "M_k differs from the model's in (capture, name, got, model)", wrong)
    for k, ((name, _c), (E, vox)) in enumerate(zip(batch, models)):
        tag = (what, "capture", k, name)
        assert got[k]["n_voxels"] == len(vox[0]), tag
        assert np.array_equal(got[k]["samples"], masked_samples(E, S[k], seeds[k])), tag
        if len(E) == 0:
            assert (got[k]["samples"] == SKIP).all() and len(got[k]["samples"]) == S[k], tag
            assert got[k]["n_hypotheses"] == 0 and len(got[k]["hands"]) == 0 and len(got[k]["handles"]) == 0, tag
    _check_filter_counts(ctx, batch, filtered, what)
    _check_cloud(ctx, batch, [v for _, v in models], what)


def _check_labeled(ctx, batch, got, plan, what, filtered=True):
    from agile_grasp_amd.binding import labeled_samples

    models, S, seeds = plan
    counts = ctx.batch_label_counts().tolist()
    print(what, "M", counts, "model", [len(e) for E, _ in models for e in E], "S", S)
    assert len(got) == len(batch) and len(counts) == sum(len(E) for E, _ in models), what
    first = np.concatenate([[0], np.cumsum([len(E) for E, _ in models])])
    wrong = [(k, name, counts[first[k]:first[k + 1]], [len(e) for e in E]) for k, ((name, _c), (E, _v)) in enumerate(zip(batch, models))
             if counts[first[k]:first[k + 1]] != [len(e) for e in E]]
    assert not wrong, (what, "the M_kj differ from the model's in (capture, name, got, model)", wrong)
    for k, ((name, _c), (E, vox)) in enumerate(zip(batch, models)):
        tag = (what, "capture", k, name)
        assert len(got[k]) == len(E) and all(g["n_voxels"] == len(vox[0]) for g in got[k]), tag
        assert np.array_equal(np.concatenate([g["samples"] for g in got[k]]), labeled_samples(E, S[k], seeds[k])), tag
        for e, g in zip(E, got[k]):
            if len(e) == 0:
                assert (g["samples"] == SKIP).all() and len(g["samples"]) == S[k] and g["n_hypotheses"] == 0 and len(g["hands"]) == 0, tag
    _check_filter_counts(ctx, batch, filtered, what)
    _check_cloud(ctx, batch, [v for _, v in models], what)


# ---- a. and b.: the masked and the labelled batch against the model ----

def test_masked_batch_equals_the_model_forwards_and_reversed():
    """Eight lattice captures at radius 2, min_neighbors 2, each tested against ITS slot of the pruned bitmap: an empty and a
    wholly pruned capture between ordinary ones, camera-1 lattices, 39 179 voxels beside 3.  The masks cover every point of a
    pruned voxel: none of them may mark."""
    ctx = _ctx(VB.LATTICE_FILTER)
    for rev in (False, True):
        batch = LATTICE[rev]
        plan = _masked_plan(batch)
        none = [0] * len(batch)  # (the mask stage runs for n_samples = 0 too: every capture's count, before anything is drawn)
        _check_masked(ctx, batch, _masked_call(ctx, batch, none, plan[2]), (plan[0], none, plan[2]), "S = 0")
        got = _masked_call(ctx, batch, plan[1], plan[2])
        _check_masked(ctx, batch, got, plan, "reversed" if rev else "forwards")
        for k, (name, _c) in enumerate(batch):
            if name in NO_VOXEL:
                assert ctx.batch_mask_counts()[k] == 0 and got[k]["n_voxels"] == 0 and len(got[k]["samples"]) > 0, name
                assert (got[k]["samples"] == SKIP).all() and got[k]["n_hypotheses"] == 0, name
    ctx.close()


def test_labelled_batch_equals_the_model_forwards_and_reversed():
    """The same captures with two objects each; the points of pruned voxels carry the object their next surviving row lacks."""
    ctx = _ctx(VB.LATTICE_FILTER)
    for rev in (False, True):
        batch = LATTICE[rev]
        plan = _labeled_plan(batch)
        none = [0] * len(batch)
        _check_labeled(ctx, batch, _labeled_call(ctx, batch, none, plan[2]), (plan[0], none, plan[2]), "S = 0")
        got = _labeled_call(ctx, batch, plan[1], plan[2])
        _check_labeled(ctx, batch, got, plan, "reversed" if rev else "forwards")
        for k, (name, _c) in enumerate(batch):
            if name in NO_VOXEL:
                assert all(g["n_voxels"] == 0 and len(g["samples"]) > 0 and (g["samples"] == SKIP).all() and g["n_hypotheses"] == 0
                           for g in got[k]), name
    ctx.close()


# ---- c. the clustered and the fitted batch against the model ----

def _bridged_counts(ctx, batch, what):
    counts = ctx.voxel_filter_counts()
    assert counts.shape == (len(batch), 6), what
    for k, (name, c) in enumerate(batch):
        assert np.array_equal(counts[k], VB.bridged_filter_model(c)["counts"]), (what, k, name, counts[k].tolist())


def _bridged_objects(info, batch, n_objects, sizes, what):
    """the bridged captures of the last clustered batch report `n_objects` objects of `sizes` voxels"""
    first = np.concatenate([[0], np.cumsum([c["cp"]["max_objects"] for _, c in batch])])
    seen = 0
    for k, (name, _c) in enumerate(batch):
        if name.startswith("bridged"):
            assert info["n_objects"][k] == n_objects and list(info["n_voxels"][first[k]:first[k] + len(sizes)]) == sizes, (what, k, name)
            seen += 1
    assert seen == 2, what


def _given_plane_call(ctx, batch, S, seeds):
    a = PB.args(batch)
    return ctx.localize_batch_clustered(a["captures"], a["sizes_left"], a["workspaces"], _cps(a["cp"]), n_samples=S, sample_seeds=seeds,
                                        classify=False, dense=a["dense"], cell_size=a["cell"])


def test_clustered_batch_clusters_each_captures_survivors():
    """Radius 1, min_neighbors 3 takes the bridge between the two blocks away: two objects of 27 and 16 voxels where the
    unfiltered capture has one of 49 -- in the batch forwards and reversed, and one of 49 again once the filter is cleared."""
    ctx = _ctx(VB.BRIDGED_FILTER, PF.ABOVE)
    S, seeds = [7, 5, 7, 6], [11, 12, 13, 14]
    for rev in (False, True):
        batch = BRIDGED[rev]
        models = VB.cluster_models(batch)
        got = _given_plane_call(ctx, batch, S, seeds)
        _check_given_plane(ctx, got, [c["cp"] for _, c in batch], S, seeds, models=[m["cluster"] for m in models],
                           clouds=[m["cloud"] for m in models])
        _bridged_objects(ctx.batch_cluster_info(), batch, 2, [27, 16], ("filtered", rev))
        _bridged_counts(ctx, batch, ("filtered", rev))
    ctx.clear_voxel_filter()
    batch = BRIDGED[True]
    models = VB.cluster_models(batch, fp=None)
    got = _given_plane_call(ctx, batch, S, seeds)
    _check_given_plane(ctx, got, [c["cp"] for _, c in batch], S, seeds, models=[m["cluster"] for m in models],
                       clouds=[m["cloud"] for m in models])
    _bridged_objects(ctx.batch_cluster_info(), batch, 1, [49], "cleared")
    assert ctx.voxel_filter_counts().shape == (0, 6)
    ctx.close()


def _fitted_samples(got, batch, models, what, S=7, seed=11):
    from agile_grasp_amd.binding import labeled_samples

    for k, ((name, _c), m) in enumerate(zip(batch, models)):
        assert m["fit"]["found"], (what, k, name)
        assert np.array_equal(np.concatenate([g["samples"] for g in got[k]]), labeled_samples(m["cluster"]["lists"], S, seed)), (what, k, name)


def test_fitted_batch_fits_and_clusters_each_captures_survivors():
    """The plane-fit stage draws its candidates among the survivors (140 inliers where the unfiltered floor has 144) and the
    clusters stand on the fitted plane; then the filter cleared on the same context; then the single fitted call, filtered."""
    ctx = _ctx(VB.BRIDGED_FILTER, PF.ABOVE)
    for rev in (False, True):
        batch = BRIDGED[rev]
        models = VB.cluster_models(batch, fitted=True)
        got = _call_fitted(ctx, batch)
        _check_fitted(ctx, batch, got, models, "reversed" if rev else "forwards")
        _fitted_samples(got, batch, models, rev)
        _bridged_objects(ctx.batch_cluster_info(), batch, 2, [27, 16], ("filtered", rev))
        _bridged_counts(ctx, batch, ("filtered", rev))
        assert [f["n_inliers"] for f, (n, _c) in zip(ctx.batch_plane_fit(), batch) if n.startswith("bridged")] == [140, 140]
    ctx.clear_voxel_filter()
    batch = BRIDGED[True]
    models = VB.cluster_models(batch, fp=None, fitted=True)
    got = _call_fitted(ctx, batch)
    _check_fitted(ctx, batch, got, models, "cleared")
    _fitted_samples(got, batch, models, "cleared")
    _bridged_objects(ctx.batch_cluster_info(), batch, 1, [49], "cleared")
    # agh_localize_clustered_fit on the bridged capture alone, filtered
    ctx.set_voxel_filter(**VB.BRIDGED_FILTER)
    (name, c), = BRIDGED[False][:1]
    (m,) = VB.cluster_models([(name, c)], fitted=True)
    got = ctx.localize_clustered_fit(c["points"], c["size_left"], c["workspace"], _fps([c["fp"]])[0], _cps([c["cp"]])[0], n_samples=7,
                                     sample_seed=11, classify=False, dense=c["dense"], cell_size=c["cell"])
    xyz, cams = ctx.cloud()
    assert np.array_equal(xyz, m["cloud"][0]) and np.array_equal(cams, m["cloud"][1])
    _same_fit(ctx.plane_fit(), m["fit"], "single")
    _same_candidates(ctx.plane_fit_candidates(), m["fit"], "single")
    info, cm = ctx.cluster_info(), m["cluster"]
    assert np.array_equal(ctx.cluster_labels(), cm["labels"])
    assert (info["n_foreground"], info["n_components"], info["n_objects"]) == (cm["n_foreground"], cm["n_components"], cm["n_objects"])
    assert np.array_equal(info["n_voxels"], cm["sizes"]) and np.array_equal(info["ids"], cm["ids"]) and list(cm["sizes"][:2]) == [27, 16]
    _fitted_samples([got], [(name, c)], [m], "single")
    assert np.array_equal(ctx.voxel_filter_counts()[0], VB.bridged_filter_model(c)["counts"])
    ctx.close()


# ---- d. a batch equals its single calls ----

def test_masked_and_labelled_batches_equal_their_single_calls():
    """Capture k of the filtered batch against the filtered single call on capture k alone, on a second context with the same
    filter; and a batch of one capture against the single call."""
    one, single = _ctx(VB.LATTICE_FILTER), _ctx(VB.LATTICE_FILTER)
    batch = LATTICE[False]
    _m, S, seeds = _masked_plan(batch)
    got = _masked_call(one, batch, S, seeds)
    counts = one.batch_mask_counts()
    singles = []
    for k, (name, c) in enumerate(batch):
        want = single.localize_masked(c["points"], c["size_left"], c["workspace"], c["mask"], n_samples=S[k], sample_seed=seeds[k], **LKW)
        assert single.sample_mask_count() == counts[k], (k, name)
        _same(got[k], want, ("masked", "capture", k, name))
        singles.append(want)
    for k in (1, 3, 7):
        alone = _masked_call(one, batch[k:k + 1], S[k:k + 1], seeds[k:k + 1])
        _same(alone[0], singles[k], ("masked", "a batch of one", k))
        assert one.batch_mask_counts().tolist() == [counts[k]] and one.voxel_filter_counts().shape == (1, 6)
    _m, S, seeds = _labeled_plan(batch)
    got = _labeled_call(one, batch, S, seeds)
    counts = one.batch_label_counts().reshape(len(batch), 2)
    singles = []
    for k, (name, c) in enumerate(batch):
        want = single.localize_labeled(c["points"], c["size_left"], c["workspace"], c["labels"], 2, n_samples=S[k], sample_seed=seeds[k], **LKW)
        assert np.array_equal(single.label_counts(), counts[k]), (k, name)
        _same_batch([got[k]], [want], ("labelled", "capture", k, name))
        singles.append(want)
    for k in (1, 3, 7):
        alone = _labeled_call(one, batch[k:k + 1], S[k:k + 1], seeds[k:k + 1])
        _same_batch(alone, [singles[k]], ("labelled", "a batch of one", k))
    _close(one, single)


def test_clustered_batches_equal_their_single_calls():
    one, single = _ctx(VB.BRIDGED_FILTER, PF.ABOVE), _ctx(VB.BRIDGED_FILTER, PF.ABOVE)
    batch = BRIDGED[False]
    S, seeds = [7, 5, 7, 6], [11, 12, 13, 14]
    got = _given_plane_call(one, batch, S, seeds)
    labels, info = one.batch_cluster_labels(), one.batch_cluster_info()
    off = np.concatenate([[0], np.cumsum([objs[0]["n_voxels"] for objs in got])])
    singles = []
    for k, (name, c) in enumerate(batch):
        want = single.localize_clustered(c["points"], c["size_left"], c["workspace"], _cps([c["cp"]])[0], n_samples=S[k],
                                         sample_seed=seeds[k], classify=False, dense=c["dense"], cell_size=c["cell"])
        _same_batch([got[k]], [want], ("clustered", "capture", k, name))
        assert np.array_equal(labels[off[k]:off[k + 1]], single.cluster_labels()), (k, name)
        assert info["n_objects"][k] == single.cluster_info()["n_objects"], (k, name)
        singles.append(want)
    alone = _given_plane_call(one, batch[:1], S[:1], seeds[:1])
    _same_batch(alone, singles[:1], "clustered, a batch of one")
    # ... and the fitted form
    got = _call_fitted(one, batch)
    fits = one.batch_plane_fit()
    for k, (name, c) in enumerate(batch):
        want = single.localize_clustered_fit(c["points"], c["size_left"], c["workspace"], _fps([c["fp"]])[0], _cps([c["cp"]])[0],
                                             n_samples=7, sample_seed=11, classify=False, dense=c["dense"], cell_size=c["cell"])
        _same_batch([got[k]], [want], ("fitted", "capture", k, name))
        _same_fit(fits[k], single.plane_fit(), ("fitted", k, name))
    _close(one, single)


# ---- e. the life cycle of the second slot set ----

def _cycle_batches():
    """The batches of the life-cycle sequence.  two: its largest lattice sizes the slots (24 576 words); grown: the capture of
    voxel_filter_batch_cases.outgrowing_case between two ordinary ones; ten: more captures than any batch before."""
    by_name = dict(LATTICE[False])
    two = [(n, by_name[n]) for n in ("cam1_block_neighbours", "seams")]
    grown = [("seams", by_name["seams"]), ("outgrowing", VB.outgrowing_case()), ("last_word", by_name["last_word"])]
    ten = LATTICE[False] + [(n, by_name[n]) for n in ("cam1_seams", "last_word")]
    return two, grown, ten


def _life_cycle(plan_of, call, check, start_filtered):
    """One context through the sequence, every step against the model and against a context that never had a filter
    (unfiltered steps) or always had it (filtered steps)."""
    two, grown, ten = _cycle_batches()
    one, never, always = _ctx(VB.LATTICE_FILTER if start_filtered else None), _ctx(), _ctx(VB.LATTICE_FILTER)

    def step(what, batch, filtered, repeat_builds=None):
        plan = plan_of(batch, filtered)
        builds = one.grid_stats()["builds"]
        got = call(one, batch, plan[1], plan[2])
        if repeat_builds is not None:  # (an outgrown slot: the call runs the batch twice)
            assert one.grid_stats()["builds"] - builds == repeat_builds, what
        check(one, batch, got, plan, what, filtered=filtered)
        want = call(always if filtered else never, batch, plan[1], plan[2])
        for k in range(len(batch)):
            _same_capture(got[k], want[k], (what, "capture", k, batch[k][0]))

    if not start_filtered:
        step("i. unfiltered, two captures", two, False)
        one.set_voxel_filter(**VB.LATTICE_FILTER)
    step("ii. the filter set on existing slots", two, True)
    step("iii. slots regrown by C after a swap", LATTICE[False], True)
    step("iv. the outgrown-slot repeat, filtered", grown, True, repeat_builds=2)
    one.clear_voxel_filter()
    step("v. cleared, more captures than before", ten, False)
    assert one.voxel_filter_counts().shape == (0, 6)
    one.set_voxel_filter(**VB.LATTICE_FILTER)
    step("vi. set again", ten, True)
    step("vi. set again, the second time", ten, True)
    _close(one, never, always)


def test_life_cycle_of_the_pruned_slots_masked():
    """i. an unfiltered batch makes the first slot set alone; ii. the filter set on a context whose slots exist; iii. eight
    captures: both sets regrown after a swap; iv. a lattice that outgrows the slots: the repeat inside the call, filtered;
    v. the filter cleared and more captures than ever: the first set grows while the second keeps its old size; vi. set again,
    twice."""
    _life_cycle(_masked_plan, _masked_call, _check_masked, start_filtered=False)


def test_life_cycle_of_the_pruned_slots_labelled():
    """Steps ii to vi in the labelled form, on a context whose first batch is filtered: the outgrown-slot repeat (iv) and the
    cleared, larger batch (v) through k_label_mark_batch's bitmap, rank table and block prefixes."""
    _life_cycle(_labeled_plan, _labeled_call, _check_labeled, start_filtered=True)


# ---- f. streams ----

def _refused_mid_chain(ctx):
    from agile_grasp_amd import binding

    for call in (lambda: ctx.set_voxel_filter(radius=3), ctx.clear_voxel_filter, ctx.voxel_filter_counts):
        with pytest.raises(binding.AghError) as e:
            call()
        assert e.value.code == binding.AGH_ERR_STATE
    assert ctx.voxel_filter().radius == VB.LATTICE_FILTER["radius"]


@pytest.mark.parametrize("form", ["masked", "labelled"])
def test_streams_filtered(form):
    """begin / stage / end of the masked and the labelled batch with the filter set: the first end, and the end of a begin that
    names the staged captures (a masked or labelled begin of host data never adopts a staged set -- it drops it and reads the
    caller's arrays), both equal the blocking call; mid-chain the filter's setter, clearer and counts are refused with
    AGH_ERR_STATE and the chain is unharmed."""
    one, ref = _ctx(VB.LATTICE_FILTER), _ctx(VB.LATTICE_FILTER)
    batch = LATTICE[False]
    plan_of, call, check, begin_of = {
        "masked": (_masked_plan, _masked_call, _check_masked, lambda c: c.localize_batch_masked_begin),
        "labelled": (_labeled_plan, _labeled_call, _check_labeled, lambda c: c.localize_batch_labeled_begin)}[form]
    plan = plan_of(batch)
    want = call(ref, batch, plan[1], plan[2])
    same = lambda got, what: [_same_capture(g, w, (form, what, k)) for k, (g, w) in enumerate(zip(got, want))]
    call(one, batch, plan[1], plan[2], f=begin_of(one))
    staged = one.localize_batch_stage([np.array(c["points"]) for _, c in batch])
    _refused_mid_chain(one)
    got = one.localize_batch_end()
    same(got, "the first end")
    check(one, batch, got, plan, form + ", the first end")
    named = [(n, dict(c, points=p)) for (n, c), p in zip(batch, staged)]
    call(one, named, plan[1], plan[2], f=begin_of(one))
    _refused_mid_chain(one)
    got = one.localize_batch_end()
    same(got, "the begin that names the staged captures")
    check(one, batch, got, plan, form + ", after the staged set")
    one.set_voxel_filter(radius=3)  # ... and after the end the setter works again
    assert one.voxel_filter().radius == 3
    _close(one, ref)


# ---- g. the depth batch forms ----

@functools.lru_cache(maxsize=None)
def _depth_inputs():
    from tests import depth_filter_cases as FC

    images, inj_masks, ws, origins, dfp = FC.injected_main()
    shape0, n1 = images[0]["data"].shape, images[1]["data"].size
    m0 = np.array(inj_masks[0], np.uint8)  # the injected pixels (which fly 15 cm in front of their surface), and a rectangle
    m0[80:160, 120:200] = 1
    lab0 = np.zeros(shape0, np.uint8)
    lab0[:, :160], lab0[:, 160:] = 1, 2
    lab0[inj_masks[0]] = 3 - lab0[inj_masks[0]]  # ... the injected pixels with the other half's object
    return dict(images=images, ws=ws, origins=origins, dfp=dfp, caps=[images, images[:1]], n0=images[0]["data"].size,
                masks=[[m0, None], [m0]], labels=[[lab0, None], [lab0]],
                packed_masks=[np.concatenate([m0.reshape(-1), np.zeros(n1, np.uint8)]), m0.reshape(-1).copy()],
                packed_labels=[np.concatenate([lab0.reshape(-1), np.zeros(n1, np.uint8)]), lab0.reshape(-1).copy()])


@pytest.mark.parametrize("depth_filter", [False, True], ids=["voxel_filter_alone", "with_the_depth_filter"])
def test_depth_batch_forms_equal_their_points_forms(svm_model, depth_filter):
    """agh_localize_depth_batch_masked, _labeled and _clustered on injected_main's two images and its first image alone, with the
    voxel filter, against the points forms on the deprojection model's points -- and with the depth filter beside it, on
    depth_filter_cases.filter_points' points."""
    from tests import depth_filter_cases as FC

    d = _depth_inputs()
    fp = dict(radius=2, min_neighbors=4)
    one, ref = _contexts(d["origins"], svm_model)
    for x in (one, ref):
        x.set_voxel_filter(**fp)
    if depth_filter:
        one.set_depth_filter(**d["dfp"])
        all_pts = FC.filter_points(d["images"], d["dfp"])[0]
    else:
        all_pts = D.deproject_ref(d["images"])
    n0, ws = d["n0"], [d["ws"], d["ws"]]
    pts = [np.array(all_pts), np.array(all_pts[:n0])]
    models = [VF.filter_model(p, D.image_index(images), d["ws"], M.CELL, **fp) for p, images in zip(pts, d["caps"])]
    print("counts", [m["counts"].tolist() for m in models])
    assert all(m["counts"][2:4].sum() > 0 and m["counts"][4:].sum() > 1000 for m in models)

    def counts_are_the_models(what):
        for x in (one, ref):
            got = x.voxel_filter_counts()
            assert got.shape == (2, 6) and all(np.array_equal(got[k], models[k]["counts"]) for k in range(2)), what

    kw = dict(KW, n_samples=[100, 80], sample_seeds=[3, 4])
    want = ref.localize_batch_masked(pts, [n0, n0], ws, d["packed_masks"], dense=True, **kw)
    got = one.localize_depth_batch_masked(d["caps"], d["masks"], ws, **kw)
    E = [VF.filtered_eligible(p, D.image_index(images), pm, d["ws"], M.CELL, m["keep"])
         for p, images, pm, m in zip(pts, d["caps"], d["packed_masks"], models)]
    assert one.batch_mask_counts().tolist() == ref.batch_mask_counts().tolist() == [len(e) for e in E]
    assert sum(w["n_hypotheses"] for w in want) > 0
    for k in range(2):
        _same(got[k], want[k], ("masked", k))
    counts_are_the_models("masked")
    kw = dict(KW, n_samples=[60, 50], sample_seeds=[5, 6])
    want = ref.localize_batch_labeled(pts, [n0, n0], ws, d["packed_labels"], [2, 2], dense=True, **kw)
    got = one.localize_depth_batch_labeled(d["caps"], d["labels"], ws, [2, 2], **kw)
    lists = [len(VF.filtered_eligible(p, D.image_index(images), pl == j + 1, d["ws"], M.CELL, m["keep"]))
             for p, images, pl, m in zip(pts, d["caps"], d["packed_labels"], models) for j in range(2)]
    assert one.batch_label_counts().tolist() == ref.batch_label_counts().tolist() == lists
    assert sum(w["n_hypotheses"] for objs in want for w in objs) > 0
    _same_batch(got, want, "labelled")
    counts_are_the_models("labelled")
    # foreground: everything more than 5 mm inside the workspace's upper z face
    cp = dict(plane=(0.0, 0.0, -1.0, float(d["ws"][5])), min_height=0.005, max_height=10.0, tolerance=0.007, min_voxels=50, max_objects=3)
    kw = dict(KW, n_samples=[40, 30], sample_seeds=[7, 8])
    want = ref.localize_batch_clustered(pts, [n0, n0], ws, _cps([cp, cp]), dense=True, **kw)
    got = one.localize_depth_batch_clustered(d["caps"], ws, _cps([cp, cp]), **kw)
    info = one.batch_cluster_info()
    print("objects", list(info["n_objects"]), "voxels", list(info["n_voxels"]))
    assert all(n >= 1 for n in info["n_objects"]) and np.array_equal(one.batch_cluster_labels(), ref.batch_cluster_labels())
    assert all(np.array_equal(info[f], ref.batch_cluster_info()[f]) for f in info)
    _same_batch(got, want, "clustered")
    counts_are_the_models("clustered")
    if depth_filter:
        assert len(one.depth_filter_counts()) == 3
    _close(one, ref)
