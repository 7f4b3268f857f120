"""agh_remove_plane off its defaults, against the host restatement (tests/cpp/plane_ref.cpp) bit for bit: parameters up to
the candidate tables' room, the refit's inlier counts on k_plane_moments' chunk and tail edges, cloud sizes on the tile, score
and scan edges, clouds RANSAC does not leave early, non-finite points, the threshold rule on exact float neighbours, the
32-byte, camera-less and device-adopted layouts, buffer reuse on one context and the argument refusals.

Every case comes from tests/plane_clouds.py and goes through its `check`; tests/test_plane_clouds.py shows on the CPU that the
restatement -- and so a GPU that agrees with it -- is in the regime the case names.
"""
import numpy as np
import pytest

from tests import plane_clouds as pc

pytestmark = pytest.mark.gpu


def _ctx():
    from agile_grasp_amd import binding, synthetic

    return binding.Context(synthetic.camera_origins())


def _run(ctx, xyz, cam, by_position=True, **params):
    ctx.set_cloud(xyz, cam)
    return pc.check(ctx, xyz, cam, by_position, **params)


class _Sequence:
    """Cases that share one context: each runs whatever became of the ones before it, and the test fails at the end with the
    names of all that disagreed (an assertion leaves the context usable: the next case sets its own cloud)."""

    def __init__(self):
        self.failed = []

    def case(self, label, fn, *args, **kw):
        try:
            return fn(*args, **kw)
        except AssertionError:
            self.failed.append(label)
            return None

    def done(self):
        if self.failed:
            pytest.fail("%d case(s) disagree: %s" % (len(self.failed), ", ".join(str(c) for c in self.failed)))


def test_inlier_counts_on_the_chunk_and_tail_edges():
    """3 (no refit), 4 .. 7 (the scalar tail alone and behind one float4), 511 .. 513 and 1023 .. 1025 (one and two chunks and
    one element beyond) inliers on ONE context, large and small in turn: d_terms shrinks and grows in use."""
    ctx, seq = _ctx(), _Sequence()

    def one(m, rough, by_position):
        xyz, cam = pc.count_cloud(m, rough)
        res = _run(ctx, xyz, cam, by_position)
        assert res["found"] and res["n_inliers"] == m

    for i, m in enumerate(pc.COUNT_ORDER):
        for rough in (False, True):
            seq.case((m, "rough" if rough else "exact"), one, m, rough, bool((i + rough) % 2))
    seq.done()


def test_point_counts_on_the_tile_score_and_scan_edges():
    """262145 points first (1025 tiles: k_plane_scan sums two tiles per lane), then 3 on the same context (stale tile counts
    and offsets beyond nblk), then the 256-point tile, the 2048 points of a k_plane_score work-group and 1024 tiles exactly."""
    ctx, seq = _ctx(), _Sequence()

    def one(n, by_position):
        xyz, cam = pc.point_cloud(n)
        res = _run(ctx, xyz, cam, by_position)
        assert res["found"] and (res["n_remaining"] == 0 if n == 3 else 0 < res["n_inliers"] < n)

    for i, n in enumerate(pc.POINT_COUNTS):
        seq.case(n, one, n, bool(i % 2))
    seq.done()


def test_blob_parameter_sequence_on_one_context():
    """The uniform blob under every parameter, on one context: 1023 iterations (full candidate tables, four generator
    refills), then 0 (nothing drawn) and 100 with the longer run's candidates and counts lying behind them, 1, the two
    probabilities, no refit, threshold 0 (everything kept; the next case runs on that kept cloud and writes the other slot),
    another seed, and a threshold beyond the cloud: nothing kept."""
    ctx, seq = _ctx(), _Sequence()
    xyz, cam = pc.blob_cloud()

    def one(name, params):
        if name in pc.BLOB_ON_KEPT_CLOUD:
            # the cloud the case before left is the blob again, in the plane path's own buffers
            assert ctx.n == len(xyz) and np.array_equal(pc.bits(ctx.cloud()[0]), pc.bits(xyz))
            res = pc.check(ctx, xyz, cam, True, **params)
        else:
            res = _run(ctx, xyz, cam, by_position=name != "optimize_off", **params)
        if name == "max_iterations_1023":
            assert res["iterations"] == 1024 and len(ctx.plane_candidates()["counts"]) == 1024
        if name == "max_iterations_0":
            assert not res["found"] and len(ctx.plane_candidates()["counts"]) == 0
        if name == "threshold_10":
            kx, kc = ctx.cloud()
            assert res["found"] and res["n_inliers"] == len(xyz) and kx.shape == (0, 3) and kc.shape == (0,)

    for name, params in pc.BLOB_CASES:
        seq.case(name, one, name, params)
    assert name == "threshold_10"
    seq.case("defaults after the empty cloud", one, "defaults", {})
    seq.done()


@pytest.mark.parametrize("by_position", [True, False])
def test_nonfinite_blob(by_position):
    """NaN in every seventh row, +-inf elsewhere: NaN candidate planes score 0 before and after the chosen one, and no such
    point is an inlier; the kept cloud carries them on, bit for bit."""
    xyz, cam = pc.nonfinite_cloud()
    ctx = _ctx()
    res = _run(ctx, xyz, cam, by_position)
    assert res["found"] and np.isnan(ctx.plane_candidates()["planes"]).any()
    assert not np.isfinite(ctx.cloud()[0]).all()


@pytest.mark.parametrize("t", sorted(pc.PROBE_CASES))
def test_threshold_rule_on_exact_neighbours(t):
    """Points at distance float32(t) and its two float neighbours from the chosen plane (0, 0, +-1, +-0), no refit: PCL's
    fabsf(dot) < (double) t.  Then threshold 0 on the same cloud: the bound is negative, and points ON a plane are no inliers."""
    xyz, cam, probes = pc.probe_cloud(t)
    ctx = _ctx()
    res = _run(ctx, xyz, cam, threshold=t, optimize=False)
    inl = set(ctx.plane_inliers().tolist())
    assert res["found"] and set(probes["below"].tolist()) <= inl and not set(probes["above"].tolist()) & inl
    assert (set(probes["at"].tolist()) <= inl) if float(np.float32(t)) < t else not set(probes["at"].tolist()) & inl
    res = _run(ctx, xyz, cam, threshold=t)  # ... and with the refit, whose inliers are chosen by the same rule
    res = _run(ctx, xyz, cam, threshold=0.0)
    assert res["found"] and res["n_inliers"] == 0 and res["n_remaining"] == len(xyz)


def _layout_clouds():
    return [pc.count_cloud(513, rough=True), pc.blob_cloud()]


@pytest.mark.parametrize("by_position", [True, False])
def test_layout_32_bytes_per_point(by_position):
    """An (n, 8) array whose padding columns hold 7.0: the kernels read with the caller's stride, the kept cloud is packed."""
    ctx = _ctx()
    for xyz, cam in _layout_clouds():
        wide = pc.padded(xyz)
        ctx.set_cloud(wide, cam)
        pc.check(ctx, wide, cam, by_position)
        pc.check(ctx, *ctx.cloud(), by_position)  # the packed kept cloud, read with stride 3 on the same context


@pytest.mark.parametrize("by_position", [True, False])
def test_layout_without_camera_ids(by_position):
    ctx = _ctx()
    for xyz, _ in _layout_clouds():
        ctx.set_cloud(xyz, None)
        pc.check(ctx, xyz, None, by_position)
        assert not ctx.cloud()[1].any()


@pytest.mark.parametrize("wide", [False, True])
def test_layout_adopted_from_device_memory(wide):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch has no device: set_cloud_torch needs a device tensor")
    ctx = _ctx()
    for xyz, cam in _layout_clouds():
        host = pc.padded(xyz) if wide else xyz
        xyz_t, cam_t = torch.from_numpy(host).cuda(), torch.from_numpy(cam).cuda()
        torch.cuda.synchronize()
        ctx.set_cloud_torch(xyz_t, cam_t)
        pc.check(ctx, host, cam, not wide)
        assert np.array_equal(pc.bits(xyz_t.cpu().numpy()), pc.bits(host))  # the adopted tensor is read, never written
        ctx.set_cloud_torch(xyz_t, None)
        pc.check(ctx, host, None, wide)


def test_refusals_leave_the_cloud_and_the_context_usable():
    from agile_grasp_amd import binding

    ctx = _ctx()
    xyz, cam = pc.count_cloud(513, rough=True)
    ctx.set_cloud(xyz, cam)
    for params in pc.REFUSALS:
        p = {**pc.DEFAULTS, **params}
        with pytest.raises(binding.AghError) as e:
            ctx.remove_plane(max_iterations=p["max_iterations"], distance_threshold=p["threshold"],
                             probability=p["probability"], seed=p["seed"], optimize=p["optimize"])
        assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT, params
        vx, vc = ctx.cloud()
        assert np.array_equal(pc.bits(vx), pc.bits(xyz)) and np.array_equal(vc, cam), params
    pc.check(ctx, xyz, cam, True)
