"""The summation loop of k_taubin_moments at the edges of its 56-neighbour chunks and of its two term tiles, against the
oracle with exact equality: the frames carry the 37 sums (params, eigenvalue, n_nb), the hypotheses follow from them.

tests/moments_chunk_clouds.py builds the clouds, tests/test_moments_chunk_clouds.py checks their counts on the CPU, and each
test here also proves from the context's neighbour counts that it ran the sizes it names.
"""
import numpy as np
import pytest

from tests import capacity_clouds as cc
from tests import moments_chunk_clouds as mc
from tests.test_gpu_parity import assert_frames_equal, assert_hyps_equal

pytestmark = pytest.mark.gpu


def _ctx():
    from agile_grasp_amd import binding

    return binding.Context(cc.cams())


@pytest.fixture(scope="module")
def chunk_edges():
    """The chunk-edge cloud and the oracle's answer for its samples (read only)."""
    from oracle import oracle_py as O

    xyz, cam, s = mc.chunk_edge_cloud()
    return xyz, cam, s, O.find_hands(cc._params({}), xyz, cam, s)


def test_chunk_edges_and_tile_parity(chunk_edges):
    """One, two and three chunks minus one row, exact and plus one row (an even and an odd last tile), twenty full chunks,
    1151 and the 1152 class's cap.  The second call runs on the first call's buffers."""
    xyz, cam, s, ref = chunk_edges
    ctx = _ctx()
    ctx.set_cloud(xyz, cam)
    for _ in range(2):
        hyps = ctx.find_hands(s)
        assert ctx.neighbor_counts()[0].tolist() == list(mc.CHUNK_EDGES)
        assert_frames_equal(ctx.frames(), ref["frames"])
        assert len(hyps) > 0
        assert_hyps_equal(hyps, ref["hyps"])


def test_list_is_read_by_sample_slot(chunk_edges):
    """The producers read a sample's points back from its neighbour list, which lives at the sample's SLOT in the list (s *
    nbr_stride), not at its index in the cloud or its place in another call's list: 32-byte points, the sample list reversed."""
    from oracle import oracle_py as O

    xyz, cam, s, _ = chunk_edges
    wide = np.full((len(xyz), 8), 7.0, np.float32)
    wide[:, :3] = xyz
    rev = np.ascontiguousarray(s[::-1])
    ref = O.find_hands(cc._params({}), xyz, cam, rev)
    ctx = _ctx()
    ctx.set_cloud(wide, cam)
    hyps = ctx.find_hands(rev)
    assert ctx.neighbor_counts()[0].tolist() == list(mc.CHUNK_EDGES)[::-1]
    assert_frames_equal(ctx.frames(), ref["frames"])
    assert_hyps_equal(hyps, ref["hyps"])


def test_big_class_chunk_edges():
    """The 4096 class (its staging area is 64 KB): 1153, twenty-one chunks minus one row / exact / plus one row, 4095 and the
    cap.  A fresh context meets these sizes with the larger classes off; the call is run until they are on."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    xyz, cam, s = mc.big_edge_cloud()
    ref = O.find_hands(cc._params({}), xyz, cam, s)
    ctx = _ctx()
    ctx.set_cloud(xyz, cam)
    hyps = None
    for attempt in range(3):
        try:
            hyps = ctx.find_hands(s)
            break
        except binding.AghError as e:  # (an entry point that does not repeat by itself reports the switch once)
            assert e.code == binding.AGH_ERR_RETRY and attempt < 2
    for _ in range(2):
        assert ctx.neighbor_counts()[0].tolist() == list(mc.BIG_EDGES)
        assert_frames_equal(ctx.frames(), ref["frames"])
        assert_hyps_equal(hyps, ref["hyps"])
        hyps = ctx.find_hands(s)  # (again, every class on from the start)


def test_all_points_pass_chunk_edges():
    """calculates_antipodal: the r = 0.01 pass over every point runs the 256 class; balls of 55, 56 and 57 points.  Every
    point's normal against the oracle."""
    from oracle import oracle_py as O

    xyz, cam, s = mc.small_edge_cloud()
    p = cc._params({})
    fr = O.fit_frames(p, xyz, cam, np.arange(len(xyz), dtype=np.int32), 0.01)
    assert fr["n_nb"][s].tolist() == list(mc.SMALL_EDGES)
    ref = O.find_hands(p, xyz, cam, s, calculates_antipodal=True)
    ctx = _ctx()
    ctx.set_cloud(xyz, cam)
    hyps = ctx.find_hands(s, calculates_antipodal=True)
    assert_frames_equal(ctx.frames(), ref["frames"])
    assert_hyps_equal(hyps, ref["hyps"])
    exp = np.where(fr["valid"][:, None] != 0, fr["normal"], 0.0)
    exp[s] = np.where(ref["frames"]["valid"][:, None] != 0, ref["frames"]["normal"], exp[s])  # (hand_search.cpp:102)
    got = ctx.normals()
    assert np.array_equal(got, exp)
    assert np.abs(got[s]).sum() > 0
