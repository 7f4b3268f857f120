"""The tail of the localize chains at its edges: kept-hand compaction across its scan blocks, the handle search under a device-side
count on both sides of every variant switch, the capacity errors, and the handles-only requeue after k_handle_batch declines --
alone and in a batch whose lists decline one by one.

The lists are tests/chain_tail_cases.py's (tests/test_chain_tail_cases.py proves on the CPU that each sits on its edge).  Every
result is held, field by field and exactly, against the four separate entry points on a second context, against the oracle's
handle search on the hands the chain returned, and (classify off) against the oracle's hands of the list.  The count of timed
handle searches of a profiling context (level 1: one event pair per queued search, so the counter is exact) shows where the search
was queued twice.

Not covered: more than 1024 handles out of a chain (k_handle_build's bounded grid taking a second stride).  Every voxel of this
cloud as a sample yields 345 handles at min_inliers = 1 with any length accepted, and no multiset of samples yields more than the
distinct hands do.
"""
import numpy as np
import pytest

from tests import chain_tail_cases as tc
from tests.test_preprocess import HANDLE_FIELDS, HYP_FIELDS, _four_calls

pytestmark = pytest.mark.gpu

ORACLE_HAND_FIELDS = ("sample", "orientation", "axis", "approach", "binormal", "bottom", "surface", "width")


@pytest.fixture(scope="module")
def table():
    return tc.build_table()


@pytest.fixture(scope="module")
def cases(table):
    return tc.single_cases(table)


def _ctx(t, svm_model, **kw):
    from agile_grasp_amd import binding

    c = binding.Context(t.rc.cam_origins, **kw)
    c.load_svm(*svm_model)
    return c


def _searches(ctx):
    return ctx.timing(counts=True)[1].get("handle_search", 0)


def _localize(ctx, t, lst, form="host", **kw):
    rc = t.rc
    kw = dict(dict(classify=False, min_inliers=2), **kw)
    samples = np.ascontiguousarray(t.s[lst])
    if form == "device":
        import torch

        return ctx.localize(torch.from_numpy(np.ascontiguousarray(rc.xyz)).cuda(), rc.size_left, rc.workspace, samples=samples, **kw)
    if form == "begin_end":
        ctx.localize_begin(np.ascontiguousarray(rc.xyz), rc.size_left, rc.workspace, samples=samples, **kw)
        return ctx.localize_end()
    return ctx.localize(rc.xyz, rc.size_left, rc.workspace, samples=samples, **kw)


def _against_oracle(got, t, lst, classify, min_inliers):
    from oracle import oracle_py as O

    if not classify:
        want = tc.hands_of(t, lst)
        assert len(got["hands"]) == len(want) == got["n_hypotheses"]
        for f in ORACLE_HAND_FIELDS:
            assert np.array_equal(got["hands"][f], want[f]), f
    hd, idx = O.find_handles(got["hands"], min_inliers, 0.005)
    assert len(got["handles"]) == len(hd) and np.array_equal(got["inlier_idx"], idx)
    for f in HANDLE_FIELDS:
        assert np.array_equal(got["handles"][f], hd[f]), f


def _check(got, t, lst, ref, classify=False, min_inliers=2):
    """got == the four-call chain of `ref` == the oracle; returns the four-call hands and handles."""
    h, hd, idx = _four_calls(ref, t.rc, np.ascontiguousarray(t.s[lst]), classify, min_inliers)
    assert got["n_voxels"] == t.n_voxels == ref.n and got["n_hypotheses"] == ref.last_n
    assert np.array_equal(got["samples"], t.s[lst])
    assert len(got["hands"]) == len(h)
    for f in HYP_FIELDS:
        assert np.array_equal(got["hands"][f], h[f]), f
    assert len(got["handles"]) == len(hd) and np.array_equal(got["inlier_idx"], idx)
    for f in HANDLE_FIELDS:
        assert np.array_equal(got["handles"][f], hd[f]), f
    _against_oracle(got, t, lst, classify, min_inliers)
    return h, hd


def test_kept_hand_counts_at_the_variant_and_block_edges(table, cases, svm_model):
    """K = 640 / 641 under d_H with both LDS variants queued, 80 samples (only the small one queued: no sample of the cloud has
    eight hypotheses, so the list is the exact fit of three hands each), 1023 / 1024 / 1025 hypotheses (compact_kept_records'
    first block edge) and 8192 (the last accepted size), one after the other on one context; then K = 641 with the raw capture on
    the device and through agh_localize_begin / _end."""
    t = table
    one, ref = _ctx(t, svm_model), _ctx(t, svm_model)
    n_handles = 0
    for name in ("K640", "K641", "S80", "N1023", "N1024", "N1025", "K8192", "K640"):
        c = cases[name]
        got = _localize(one, t, c["lst"])
        assert got["n_hypotheses"] == len(got["hands"]) == c["K"], name
        _, hd = _check(got, t, c["lst"], ref)
        print(name, "S", len(c["lst"]), "K", len(got["hands"]), "handles", len(hd))
        n_handles += len(hd)
    assert n_handles > 0
    for form in ("device", "begin_end"):
        got = _localize(one, t, cases["K641"]["lst"], form)
        assert len(got["hands"]) == 641
        _check(got, t, cases["K641"]["lst"], ref)


def test_compaction_carries_across_blocks_with_holes(table, svm_model):
    """classify on, more than 2048 hypotheses of which the classifier keeps some: the ordered compaction's carry crosses two
    block edges over lists with holes."""
    t = table
    lst = tc.classify_list(t)
    one, ref = _ctx(t, svm_model), _ctx(t, svm_model)
    got = _localize(one, t, lst, classify=True)
    print("hypotheses", got["n_hypotheses"], "kept", len(got["hands"]), "handles", len(got["handles"]))
    assert got["n_hypotheses"] > 2048 and 0 < len(got["hands"]) < got["n_hypotheses"]
    h, _ = _check(got, t, lst, ref, classify=True)
    kept_at = np.flatnonzero(ref.classify())
    assert kept_at.min() < 1024 and kept_at.max() >= 2048  # kept records in the first block and beyond the second edge


def test_capacity_errors_leave_the_context_working(table, cases, svm_model):
    """8193 kept hands and a seed with 2049 inliers: AGH_ERR_CAPACITY out of the chain, each naming its limit, and the next chain
    on the context is right."""
    from agile_grasp_amd import binding

    t = table
    one, ref = _ctx(t, svm_model), _ctx(t, svm_model)
    for name, text in (("K8193", "more than 8192 hands"), ("R2049", "more than 2048 inliers")):
        with pytest.raises(binding.AghError) as e:
            _localize(one, t, cases[name]["lst"])
        assert e.value.code == binding.AGH_ERR_CAPACITY and text in str(e.value), name
        got = _localize(one, t, cases["K640"]["lst"])
        assert len(got["hands"]) == 640
        _check(got, t, cases["K640"]["lst"], ref)


@pytest.mark.parametrize("variant", ["small", "general"])
def test_declined_search_is_requeued_alone(table, cases, svm_model, variant):
    """One sample 129 times: k_handle_batch declines on the device, the chain's one synchronisation sees it, the handle search
    alone is queued once more with k_handle_greedy behind it (the LDS variant for K <= 640) and the search's counts survive.  A
    profiling context counts the searches: one for a plain chain, two for the first declined one, one for the next (the
    sequential kernel is queued along), one for the 128-row chain after it -- which leaves the guess off again."""
    t = table
    declined = cases["R129small" if variant == "small" else "R129general"]["lst"]
    one, ref = _ctx(t, svm_model, profile=True), _ctx(t, svm_model)
    _check(_localize(one, t, cases["K640"]["lst"]), t, cases["K640"]["lst"], ref)  # (switches any capacity class on)
    _searches(one)
    for lst, want in ((cases["K640"]["lst"], 1), (declined, 2), (declined, 1), (cases["R128"]["lst"], 1), (declined, 2)):
        got = _localize(one, t, lst)
        n = _searches(one)
        print(variant, "K", len(got["hands"]), "timed handle searches", n)
        assert n == want
        _check(got, t, lst, ref)
    plain = _ctx(t, svm_model)
    for form in ("device", "begin_end", "host"):  # each the first declined chain after a chain that was not
        _check(_localize(plain, t, declined, form), t, declined, ref)
        _check(_localize(plain, t, cases["R128"]["lst"], form), t, cases["R128"]["lst"], ref)


def _batch(ctx, t, lists, form="call"):
    rc = t.rc
    caps = [np.ascontiguousarray(rc.xyz).copy() for _ in lists]
    kw = dict(samples=[np.ascontiguousarray(t.s[l]) for l in lists], classify=False, min_inliers=2)
    if form == "begin_end":
        ctx.localize_batch_begin(caps, [rc.size_left] * len(lists), [rc.workspace] * len(lists), **kw)
        return ctx.localize_batch_end()
    return ctx.localize_batch(caps, [rc.size_left] * len(lists), [rc.workspace] * len(lists), **kw)


def test_batch_with_one_declining_list(table, svm_model):
    """Three captures side by side, one of whose lists holds a row of 129: the batch-wide repeat queues k_handle_greedy for every
    list, and it must leave the two that did not decline alone.  The declining list in the middle and last, a batch of plain
    lists after it on the same context, and one mixed batch through agh_localize_batch_begin / _end; every capture against
    agh_localize on a second context and against the oracle."""
    t = table
    b = tc.batch_lists(t)
    one, ref = _ctx(t, svm_model, profile=True), _ctx(t, svm_model)
    single = {}

    def check(got, lists, Ks):
        assert len(got) == len(lists)
        for k, (g, lst, K) in enumerate(zip(got, lists, Ks)):
            key = lst.tobytes()
            if key not in single:
                single[key] = _localize(ref, t, lst)
            r = single[key]
            assert g["n_voxels"] == r["n_voxels"] == t.n_voxels and g["n_hypotheses"] == r["n_hypotheses"] == K, k
            assert np.array_equal(g["samples"], r["samples"]) and len(g["hands"]) == len(r["hands"]) == K, k
            for f in HYP_FIELDS:
                assert np.array_equal(g["hands"][f], r["hands"][f]), (k, f)
            assert len(g["handles"]) == len(r["handles"]) and np.array_equal(g["inlier_idx"], r["inlier_idx"]), k
            for f in HANDLE_FIELDS:
                assert np.array_equal(g["handles"][f], r["handles"][f]), (k, f)
            _against_oracle(g, t, lst, False, 2)
        assert sum(len(g["handles"]) for g in got) > 0

    check(_batch(one, t, b["plain"]), b["plain"], b["K"]["plain"])  # (switches any capacity class on)
    _searches(one)
    for kind, want in (("plain", 1), ("mixed", 2), ("last", 1), ("plain", 1), ("last", 2), ("mixed", 1)):
        got = _batch(one, t, b[kind])
        n = _searches(one)
        print(kind, "timed handle searches", n)
        assert n == want, kind
        check(got, b[kind], b["K"][kind])
    plain = _ctx(t, svm_model)
    for kind in ("mixed", "plain", "last"):
        check(_batch(plain, t, b[kind], "begin_end"), b[kind], b["K"][kind])
