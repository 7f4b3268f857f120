"""tests/plane_fit_batch_cases.py: every batch is in the regime it is named after, shown from the numpy models alone.  Needs no
GPU."""
import numpy as np
import pytest

from tests import plane_fit_batch_cases as PB
from tests import plane_fit_cases as PF

FIT_TILE = 512  # voxels per work-group of the scoring and moments kernels (plane_fit.hip, kFitTile)


@pytest.fixture(scope="module")
def small():
    batch = PB.small_batch()
    return batch, PB.models(batch)


def test_small_batch_is_every_case_within_64_lists(small):
    batch, models = small
    assert [n for n, _ in batch] == list(PF.cases()) and len(batch) == 22
    assert sum(c["cp"]["max_objects"] for _, c in batch) == 44 <= 64
    assert len({c["cell"] for _, c in batch}) == 1
    # the lowered max_objects is all that differs from the single cases
    for (n, c), (_n, single) in zip(batch, PF.cases().items()):
        assert c["fp"] == single["fp"] and np.array_equal(c["points"], single["points"]) and c["cp"] == dict(single["cp"], max_objects=2), n


def test_small_batch_mixes_no_plane_with_found(small):
    batch, models = small
    names = [n for n, _ in batch]
    N = {n: m["fit"]["n_voxels"] for n, m in zip(names, models)}
    assert [N["too_few_0"], N["too_few_1"], N["too_few_2"], N["too_few_3"], N["collinear"]] == [0, 1, 2, 3, 30]
    found = [m["fit"]["found"] for m in models]
    for n in ("too_few_0", "too_few_1", "too_few_2", "too_few_3", "collinear", "min_inliers_above"):
        k = names.index(n)
        assert not found[k] and models[k]["cluster"] is None and (models[k]["fit"]["plane"] == 0).all(), n
        assert found[k - 1] or found[k + 1] or n.startswith("too_few")  # (a found capture beside it, or the run of too_few cases)
    assert found[names.index("too_few_0") - 1] and found[names.index("too_few_3") + 1]
    assert sum(found) == len(batch) - 6
    # a found capture has objects
    assert all(m["cluster"]["n_objects"] >= 1 for n, m in zip(names, models) if m["fit"]["found"] and n.startswith("floor_blocks"))


def test_small_batch_mixes_candidate_counts_and_tile_counts(small):
    batch, models = small
    C = sorted({c["fp"]["n_candidates"] for _, c in batch})
    assert C == [1, 16, 128, 256]
    N = np.array([m["fit"]["n_voxels"] for m in models])
    raw = np.array([len(c["points"]) for _, c in batch])
    blocks = -(-raw.max() // FIT_TILE)  # the launch is sized from the largest capture's raw points
    assert blocks >= 4 and (N > 3 * FIT_TILE).any()  # captures of several tiles ...
    assert ((N > 0) & (N < 64)).any() and (N == 0).any()  # ... beside captures of one partial wave, and an empty one
    beyond = [(blocks - -(-int(n) // FIT_TILE)) for n in N]
    assert min(beyond) == 0 and sum(b > 0 for b in beyond) >= 20  # work-groups beyond their capture's N_k, in nearly every capture
    # a block that holds 256 candidates forwards holds 1 in the reversed batch (and the other way round)
    cs = [c["fp"]["n_candidates"] for _, c in batch]
    rev = cs[::-1]
    assert any(a == 256 and b < 256 for a, b in zip(cs, rev)) and any(a == 1 and b > 1 for a, b in zip(cs, rev))


def _joint_counts(batch, k):
    """capture k's candidates scored over BOTH clouds of a pair: what a count that crossed captures would be"""
    clouds = [PF.voxel_cloud(c)[0] for _, c in batch]
    fp = batch[k][1]["fp"]
    idx, planes, valid = PF.candidates(clouds[k], fp["n_candidates"], fp["seed"])
    return PF.counts(np.concatenate(clouds), planes, valid, fp["distance_threshold"])


def test_seed_pair_shares_coordinates_not_draws():
    batch = PB.seed_pair()
    a, b = PB.models(batch)
    assert np.array_equal(a["cloud"][0], b["cloud"][0]) and np.array_equal(a["cloud"][1], b["cloud"][1])
    assert (batch[0][1]["fp"]["seed"], batch[1][1]["fp"]["seed"]) == (1, 2)
    assert not np.array_equal(a["fit"]["idx"], b["fit"]["idx"]) and a["fit"]["found"] and b["fit"]["found"]
    for k, m in enumerate((a, b)):
        joint = _joint_counts(batch, k)
        assert np.array_equal(joint, 2 * m["fit"]["counts"]) and (m["fit"]["counts"] > 0).any()  # a joint count doubles
        assert joint.max() != m["fit"]["n_inliers"]
    # indices drawn over both clouds' voxels together are other indices
    N = len(a["cloud"][0])
    assert not np.array_equal(PF.draw(2 * N, 128, 1), PF.draw(N, 128, 1))


def test_lifted_pair_is_the_same_floor_five_centimetres_up():
    batch = PB.lifted_pair()
    a, b = PB.models(batch)
    xa, xb = a["cloud"][0], b["cloud"][0]
    # (the corner voxel that pins the lattice stays where it is: the lifted capture has it below its floor)
    za, zb = np.unique(xa[:, 2]), np.unique(xb[:, 2])
    assert abs(float(zb[1]) - float(za[0]) - 0.05) < 1e-6
    fa = xa[xa[:, 2] == za[0]]
    fb = xb[xb[:, 2] == zb[1]]
    assert len(fa) == len(fb) == 144 and np.array_equal(fa[:, :2], fb[:, :2])
    assert a["fit"]["found"] and b["fit"]["found"] and a["fit"]["n_inliers"] == b["fit"]["n_inliers"] == 144
    assert abs(float(b["fit"]["plane"][3] - a["fit"]["plane"][3]) + 0.05) < 1e-6  # each capture its own floor
    for k, m in enumerate((a, b)):
        joint = _joint_counts(batch, k)
        assert (joint != m["fit"]["counts"]).any(), k  # candidates that cut the other capture's voxels count them too


def test_origin_batch_flips_one_capture():
    batch = PB.origin_batch()
    table = PB.origin_table(batch)
    assert table.shape == (3, 2, 3) and table[1, 0, 2] == 0.0 and table[0, 0, 2] == table[2, 0, 2] == 2.0
    m = PB.models(batch)
    assert all(x["fit"]["found"] for x in m)
    assert np.array_equal(m[0]["fit"]["plane"], m[2]["fit"]["plane"]) and np.array_equal(m[1]["fit"]["plane"], -m[0]["fit"]["plane"])
    assert m[0]["fit"]["plane"][2] > 0 > m[1]["fit"]["plane"][2]
    # the heights change sign with the plane: the flipped capture has no voxel above its plane
    assert m[0]["cluster"]["n_objects"] == 2 and m[1]["cluster"]["n_foreground"] == 0
    # without a table every capture takes the context's own origin
    same = PB.models(batch, table=np.stack([batch[0][1]["origins"]] * 3))
    assert all(np.array_equal(x["fit"]["plane"], m[0]["fit"]["plane"]) for x in same)
