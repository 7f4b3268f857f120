"""The kernels at their capacity-class and launch-size boundaries, against the oracle with exact equality.

Each case is built (tests/capacity_clouds.py, checked on the CPU by tests/test_capacity_clouds.py) to sit exactly on a
count where the code switches instantiation, tile, LDS class or launch, and each test also proves that it got there: from
the context's neighbour counts, the numpy crop count, S or the length of the list.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import capacity_clouds as cc
from tests.test_gpu_parity import FLOAT_FIELDS, INT_FIELDS, assert_frames_equal, assert_hyps_equal
from tests.test_handles import FIELDS as HANDLE_FIELDS

pytestmark = pytest.mark.gpu


def _ctx(**kw):
    from agile_grasp_amd import binding

    return binding.Context(cc.cams(), **kw)


def _oracle(geom=None, **kw):
    return cc._params(geom or {}, **kw)


# ---- Taubin capacity classes -----------------------------------------------------------------------------------
def test_taubin_classes_at_their_edges_det():
    """1 .. 6145 neighbours in one list: K1a's 256 / 1152 / 4096 hand-offs, the 4096 class's list walk, the 6144 class
    and the retries that switch the classes on; then the same call again with every class on."""
    from oracle import oracle_py as O

    xyz, cam, s = cc.ball_cloud(cc.TAUBIN_DET, 0.03, seed=1, filler=500)
    ref = O.find_hands(_oracle(), xyz, cam, s)
    ctx = _ctx()
    ctx.set_cloud(xyz, cam)
    for _ in range(2):
        hyps = ctx.find_hands(s)
        nt, nh = ctx.neighbor_counts()
        assert nt.tolist() == list(cc.TAUBIN_DET) and np.array_equal(nh, ref["nh"])
        assert_frames_equal(ctx.frames(), ref["frames"])
        assert len(hyps) > len(s) and (np.bincount(hyps["sample"], minlength=len(s)) > 0).all()
        assert_hyps_equal(hyps, ref["hyps"])


def test_rand50_draw_edges():
    """49 / 50 / 51 neighbours (draws only for n > 50) and 1152 / 1153 early in a list: a wrong draw offset shifts every
    later sample's normals."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    xyz, cam, s = cc.rand50_cloud()
    for seed in (1, 7):
        ref = O.find_hands(_oracle(normals_mode=O.NORMALS_RAND50, rand_seed=seed), xyz, cam, s)
        ctx = _ctx(normals_mode=binding.NORMALS_RAND50, rand_seed=seed)
        ctx.set_cloud(xyz, cam)
        hyps = ctx.find_hands(s)
        nt, _ = ctx.neighbor_counts()
        assert nt[:len(cc.RAND50_EDGE)].tolist() == list(cc.RAND50_EDGE)
        assert_frames_equal(ctx.frames(), ref["frames"])
        assert len(hyps) > len(s)
        assert_hyps_equal(hyps, ref["hyps"])


@pytest.mark.parametrize("total", cc.ALLPOINTS_SIZES)
def test_all_points_pass_at_class_and_chunk_edges(total):
    """calculates_antipodal: r = 0.01 balls of 128/129, 256/257, 1152/1153 points, and a cloud of kNormalsChunk points or
    one more (a last chunk of one point).  Every point's normal and the antipodal labels against the oracle."""
    from oracle import oracle_py as O

    xyz, cam, s = cc.ball_cloud(cc.ALLPOINTS, 0.01, seed=2, total=total)
    p = _oracle()
    fr = O.fit_frames(p, xyz, cam, np.arange(total, dtype=np.int32), 0.01)
    assert len(xyz) == total and fr["n_nb"][s].tolist() == list(cc.ALLPOINTS)
    ctx = _ctx()
    ctx.set_cloud(xyz, cam)
    hyps = ctx.find_hands(s, calculates_antipodal=True)
    ref = O.find_hands(p, xyz, cam, s, calculates_antipodal=True)
    assert_frames_equal(ctx.frames(), ref["frames"])
    assert len(hyps) > 0 and hyps["half_antipodal"].any()
    assert_hyps_equal(hyps, ref["hyps"])
    exp = np.where(fr["valid"][:, None] != 0, fr["normal"], 0.0)
    exp[s] = np.where(ref["frames"]["valid"][:, None] != 0, ref["frames"]["normal"], exp[s])  # (hand_search.cpp:102)
    got = ctx.normals()
    assert np.array_equal(got, exp)
    assert np.abs(got[-1]).sum() > 0  # the last chunk's point has its normal


# ---- the sweep's LDS tile ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(cc.TILES))
def test_sweep_tile_edges(kind):
    """Hand crops of T - 1, T, T + 1, 2T and 2T + 1 points for every tile size of k_hand_sweep: the reservation that does
    not fit closes the tile and the wave resumes from its cursor.  The crop's points sit in the hands' closing region, so
    a point lost or doubled at the hand-off changes n_in_box.  normals_probe3 and train_probe3 repeat the antipodal and the
    training tile with the general-probe geometry: <1, kLutProbe, kLutProbe> and <2, ..> with a hand that needs a third probe."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    xyz, cam, s, geom, fr0 = cc.tile_cloud(kind)
    T = cc.TILES[kind]
    k = len(cc.tile_targets(T))
    g = {**cc.HAND_DEFAULTS, **geom}
    p = _oracle(geom)
    train = kind in ("train", "train_probe3")
    anti = train or kind in ("normals", "normals_probe3")
    ctx = _ctx(**geom)
    if train:
        ctx.set_training_images(True)
    ctx.set_cloud(xyz, cam)
    hyps = ctx.find_hands(s, calculates_antipodal=anti)
    if train:
        ref = O.find_hands_training(p, xyz, cam, s)
        ref_fr = O.fit_frames(p, xyz, cam, s, g["nn_radius_taubin"])
    else:
        ref = O.find_hands(p, xyz, cam, s, calculates_antipodal=anti, want_images=True)
        ref_fr = ref["frames"]
    frames = ctx.frames()
    assert_frames_equal(frames, ref_fr)
    crop = [cc.crop_count(xyz, xyz[s[j]], frames["axis"][j], g["nn_radius_hands"], g["hand_height"]) for j in range(k)]
    assert crop == list(cc.tile_targets(T))
    if kind == "wg4":
        assert len(s) > 4096  # k_hand_sweep's four-per-CU form
    for j in range(k):
        assert (hyps["n_in_box"][hyps["sample"] == j] > 400).any(), j  # (more points than the sample's own patch holds)
    assert_hyps_equal(hyps, ref["hyps"])
    if train:
        packed = ctx.training_images()
        images = binding.unpack_images(packed.reshape(-1, 250)).reshape(-1, 3, 8000)
        assert np.array_equal(images, ref["images"])
        assert np.array_equal(ctx.hog_images(packed.reshape(-1, 250)), O.hog_many(ref["images"].reshape(-1, 8000)))
    else:
        assert np.array_equal(ctx.images(), ref["images"])


# ---- sample-count dispatch and the three compaction paths ---------------------------------------------------------
@pytest.fixture(scope="module")
def c2_lists():
    """65 537 distinct samples of C2 and the oracle's result for all of them (samples are independent, so every prefix's
    result is the prefix of this one)."""
    from agile_grasp_amd import synthetic
    from oracle import oracle_py as O

    sc = synthetic.config("C2")
    s = np.random.default_rng(11).permutation(sc.n)[:max(cc.SAMPLE_COUNTS)].astype(np.int32)
    ref = O.find_hands(O.default_params(sc.cam_origins, num_threads=min(os.cpu_count() or 1, 16)), sc.xyz, sc.cam, s)
    return sc, s, ref


def _prefix(ref, S):
    h = ref["hyps"]
    return h[h["sample"] < S], ref["frames"][:S]


def test_sample_counts_det(c2_lists):
    """S = 1 .. 65 537: k_taubin_eigen's eight lanes per sample up to 4096, the scheduling orders, the sweep's block order
    from S = 128, WG4 beyond 4096, and compaction fused (<= 4096), in two launches (<= 65 536) and in three beyond."""
    from agile_grasp_amd import binding

    sc, s, ref = c2_lists
    ctx = binding.Context(sc.cam_origins)
    ctx.set_cloud(sc.xyz, sc.cam)
    for S in cc.SAMPLE_COUNTS:
        hyps = ctx.find_hands(s[:S])
        rh, rf = _prefix(ref, S)
        assert ctx.last_samples == S and len(ctx.frames()) == S
        assert_frames_equal(ctx.frames(), rf)
        assert_hyps_equal(hyps, rh)
    assert (rh["sample"] >= 256 * 1024 // 8).any()  # (slots beyond k_compact_top's first 256-entry chunk hold hypotheses)


def test_sample_counts_rand50(c2_lists):
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    sc, s, _ = c2_lists
    sub = s[:4097]
    ref = O.find_hands(O.default_params(sc.cam_origins, normals_mode=O.NORMALS_RAND50, rand_seed=3,
                                        num_threads=min(os.cpu_count() or 1, 16)), sc.xyz, sc.cam, sub)
    ctx = binding.Context(sc.cam_origins, normals_mode=binding.NORMALS_RAND50, rand_seed=3)
    ctx.set_cloud(sc.xyz, sc.cam)
    for S in (4096, 4097):
        hyps = ctx.find_hands(sub[:S])
        rh, rf = _prefix(ref, S)
        assert_frames_equal(ctx.frames(), rf)
        assert_hyps_equal(hyps, rh)


# ---- output length ----------------------------------------------------------------------------------------------
def _find_cap(ctx, samples, cap, with_out=True):
    """agh_find_hands with an explicit cap: (rc, *n_out, the records written)."""
    from agile_grasp_amd import binding

    out = np.zeros(max(cap, 1), binding.HYP_DTYPE)
    n = C.c_int64(-1)
    rc = ctx.lib.agh_find_hands(ctx._h, samples.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(len(samples)), C.c_int(0),
                                out.ctypes.data_as(C.c_void_p) if with_out else None, C.c_int64(cap), C.byref(n))
    return rc, n.value, out


@pytest.mark.parametrize("S", [100, 5000, 65537])  # one S per compaction path
def test_output_capacity_host_and_device(c2_lists, S):
    """Host: cap = count is enough, cap = count - 1 and cap = 0 are AGH_ERR_CAPACITY with *n_out = count, and the context
    then answers in full.  Device: cap = count - 1 is reported by agh_synchronize, *d_n_out holds the count and d_out the
    first cap records (include/agh.h)."""
    import torch

    from agile_grasp_amd import binding

    sc, s, ref = c2_lists
    sub = np.ascontiguousarray(s[:S])
    rh, _ = _prefix(ref, S)
    count = len(rh)
    assert count > 1
    ctx = binding.Context(sc.cam_origins)
    ctx.set_cloud(sc.xyz, sc.cam)
    for cap, with_out in ((count - 1, True), (0, False), (0, True)):
        rc, n, _ = _find_cap(ctx, sub, cap, with_out)
        assert (rc, n) == (binding.AGH_ERR_CAPACITY, count), cap
    rc, n, out = _find_cap(ctx, sub, count)
    assert (rc, n) == (0, count)
    assert_hyps_equal(out[:n], rh)
    # the device entry point
    s_t = torch.from_numpy(sub).cuda()
    out_t = torch.zeros((count - 1) * 160, dtype=torch.uint8, device="cuda")
    n_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.find_hands_torch(s_t, out_t, n_t)
    with pytest.raises(binding.AghError) as e:
        ctx.synchronize()
    assert e.value.code == binding.AGH_ERR_CAPACITY
    assert int(n_t.item()) == count
    got = np.frombuffer(out_t.cpu().numpy().tobytes(), dtype=binding.HYP_DTYPE)
    for f in INT_FIELDS + FLOAT_FIELDS:
        assert np.array_equal(got[f], rh[f][:count - 1]), f
    assert_hyps_equal(ctx.find_hands(sub), rh)  # ... and the context still works


def test_pinned_mirror_edge(c2_lists):
    """Host lists of exactly 65 536 (kMirrorMaxRecords) and 65 537 hypotheses: the second finishes from the device copy.
    A shuffled multiset of C2 samples with six hypotheses each (duplicates are independent work items)."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    sc, s, ref = c2_lists
    y = np.bincount(ref["hyps"]["sample"], minlength=len(s))
    rng = np.random.default_rng(5)
    y6 = s[y == 6]
    assert len(y6) > 50
    body = list(rng.choice(y6, 65536 // 6)) + [s[np.flatnonzero(y == 65536 % 6)[0]]]
    one = s[np.flatnonzero(y == 1)[0]]
    ctx = binding.Context(sc.cam_origins)
    ctx.set_cloud(sc.xyz, sc.cam)
    for want, lst in zip(cc.MIRROR_COUNTS, (body, body + [one])):
        lst = np.array(lst, np.int32)[rng.permutation(len(lst))]
        r = O.find_hands(O.default_params(sc.cam_origins, num_threads=min(os.cpu_count() or 1, 16)), sc.xyz, sc.cam, lst)
        assert len(r["hyps"]) == want
        hyps = ctx.find_hands(lst)
        assert_hyps_equal(hyps, r["hyps"])


# ---- handle search ----------------------------------------------------------------------------------------------
def _handles_equal(ctx, hands, mi=3, ml=0.005):
    from oracle import oracle_py as O

    ghd, gidx = ctx.find_handles(hands, mi, ml)
    hd, idx = O.find_handles(hands, mi, ml)
    assert len(ghd) == len(hd) and np.array_equal(gidx, idx)
    for f in HANDLE_FIELDS:
        assert np.array_equal(ghd[f], hd[f]), f
    return hd


@pytest.mark.parametrize("H", cc.HANDLE_COUNTS)
def test_handle_search_hand_counts(H):
    """H = 640 / 641 (LDS and general variants), 1024 / 1025 (W > 16), 4096 / 4097 (the two-half walk, W > 64), 8192."""
    hands = cc.handle_hands(H, 0, seed=H)
    ctx = _ctx()
    for _ in range(2):
        hd = _handles_equal(ctx, hands)
        assert len(hd) > H // 40


def test_handle_search_inliers_of_one_seed():
    """64 / 65 inliers (k_handle_batch takes two members per lane beyond one wave's row) in both variants, 2048 inliers
    (kHandleListCap, far beyond kMaxRow: k_handle_greedy) and 2049: AGH_ERR_CAPACITY, after which the context still works."""
    from agile_grasp_amd import binding

    ctx = _ctx()
    for H, big in cc.HANDLE_SEEDS:
        hands = cc.handle_hands(H, big, seed=H + big)
        if big > 2048:
            with pytest.raises(binding.AghError) as e:
                ctx.find_handles(hands, 3, 0.005)
            assert e.value.code == binding.AGH_ERR_CAPACITY
        else:
            hd = _handles_equal(ctx, hands)
            assert int(hd["n_inliers"].max()) == big
    _handles_equal(ctx, cc.handle_hands(3000, 2048, seed=5048))
    _handles_equal(ctx, cc.handle_hands(600, 65, seed=665))


def _searches(ctx):
    """Timed handle searches since the previous look (profile level 1 records one event pair per queued search)."""
    return ctx.timing(counts=True)[1].get("handle_search", 0)


@pytest.mark.parametrize("H,big", cc.HANDLE_ROWS)
def test_handle_search_rows_around_kmaxrow(H, big):
    """127 / 128 hands in the longest row (k_handle_batch, two members per lane) and 129 (declined: k_handle_greedy, the LDS
    variant for H = 600), twice on one context: the second call starts with the sequential kernel queued or not as the first
    left it."""
    hands = cc.handle_hands(H, big, seed=H + big)
    ctx = _ctx()
    for _ in range(2):
        hd = _handles_equal(ctx, hands)
        assert int(hd["n_inliers"].max()) == big


@pytest.mark.parametrize("case", cc.HANDLE_ROW_SHAPES, ids=cc.row_shape_id)
def test_handle_search_two_slot_rows(case):
    """Rows of 128 and 100 hands in k_handle_batch's two-slot evaluation: a shortenHandle gap at the end of the first slot,
    across the slots, in the second and before the row's last hand; equal distances whose order the index decides across the
    slots; rows with more than 64 potential and fewer than 64 live members (tests/test_capacity_clouds.py proves each)."""
    hands = cc.row_shape_hands(case)
    ctx = _ctx()
    for _ in range(2):
        hd = _handles_equal(ctx, hands)
    H, big, opt = case
    if "gap_after" in opt:
        assert opt["gap_after"] in hd["n_inliers"]
    else:
        assert int(hd["n_inliers"].max()) == big - opt.get("dead", 0)


@pytest.mark.parametrize("H", [600, 1500])
def test_handle_search_decline_order_on_one_context(H):
    """Declined (129) -> not declined (128) -> declined (129) on one context, then 129 again: the sequential kernel not queued
    and needed (the search is repeated with it), queued and not needed, not queued and needed again, queued and needed.  The
    context is a profiling one and the count of timed handle searches shows each repeat: profile level 1 records one event
    pair per queued search and agh_get_timing_counts counts the pairs, so the counter is exact."""
    sets = {big: cc.handle_hands(H, big, seed=H + big) for big in (128, 129)}
    ctx = _ctx(profile=True)
    _searches(ctx)
    for big, want in ((129, 2), (129, 1), (128, 1), (129, 2), (129, 1), (128, 1), (128, 1)):
        hd = _handles_equal(ctx, sets[big])
        assert int(hd["n_inliers"].max()) == big
        assert _searches(ctx) == want, (big, want)
