"""The batches of tests/voxel_filter_batch_cases.py are in the regimes that make tests/test_gpu_voxel_filter_batches.py able to
fail: conditions on the numpy models alone (no GPU)."""
import numpy as np

from tests import cluster_cases as CC
from tests import plane_fit_cases as PF
from tests import voxel_filter_batch_cases as VB
from tests import voxel_filter_cases as VF

WORDS_PER_BLOCK = 4096


def _lattice(name):
    return dict(VB.lattice_batch())[name]


def test_the_models_are_the_existing_ones_composed():
    """a capture's model is voxel_filter_cases' on its own points at the batch's filter; the masks and labels are made from it"""
    for name, c in VB.lattice_batch():
        assert (c["radius"], c["min_neighbors"], c["cell"], c["dense"]) == (2, 2, 0.01, True), name
        m = VF.case_model(c)
        assert np.array_equal(m["keep"], c["model"]["keep"]) and np.array_equal(m["counts"], c["model"]["counts"]), name
        pruned = VB.pruned_points(c["rows"], m["keep"])
        every_fourth = np.zeros(len(pruned), bool)
        every_fourth[::4] = True
        assert np.array_equal(c["mask"] != 0, pruned | every_fourth), name
        parity = 1 + np.arange(len(pruned)) % 2
        assert np.array_equal(c["labels"][~pruned], parity[~pruned]) and set(np.unique(c["labels"])) <= {1, 2}, name
        E, cloud = VB.masked_model(c)
        assert len(cloud[0]) == m["keep"].sum() and (len(E) == 0 or E.max() < len(cloud[0])), name
    assert [n for n, _ in VB.lattice_batch(True)] == list(VB.LATTICE_ORDER[::-1])
    assert [n for n, _ in VB.bridged_batch(True)] == list(VB.BRIDGED_ORDER[::-1])


def test_a_pruned_point_that_marked_would_change_the_lists():
    """Condition 1: every masked point of a pruned voxel marking the next surviving row instead of nothing gives another list than
    E -- 94 against 79 voxels for seams, 98 against 88 for cam1_seams, 40 against 39 for camera0_inside_camera1 -- and another
    list for at least one object of each; the labels of pruned points were chosen against the next row's in each of them."""
    sizes = {}
    for name in VB.LEAK_CASES:
        c = _lattice(name)
        keep = c["model"]["keep"]
        E, _ = VB.masked_model(c)
        leak = VB.leaky_eligible(c["rows"], keep, c["mask"])
        assert not np.array_equal(leak, E), name
        assert set(E) < set(leak), name  # (the surviving voxels' marks are all still there)
        sizes[name] = (len(leak), len(E))
        lists, _ = VB.labeled_model(c)
        leaks = [VB.leaky_eligible(c["rows"], keep, c["labels"] == j + 1) for j in range(2)]
        print(name, "E", len(E), "leaky", len(leak), "lists", [len(e) for e in lists], "leaky", [len(e) for e in leaks])
        assert any(not np.array_equal(a, b) for a, b in zip(leaks, lists)), name
    assert sizes == {"seams": (94, 79), "cam1_seams": (98, 88), "camera0_inside_camera1": (40, 39)}
    for name in ("seams", "cam1_seams"):  # (camera0_inside_camera1's pruned voxels have no surviving row of their camera behind)
        c = _lattice(name)
        pruned = VB.pruned_points(c["rows"], c["model"]["keep"])
        parity = 1 + np.arange(len(pruned)) % 2
        assert (c["labels"][pruned] != parity[pruned]).any(), name


def test_the_bridged_capture():
    """Condition 2: unfiltered one object of 49 voxels, filtered two of 27 and 16; counts (196, 0, 13, 0, 183, 0); 140 fit inliers
    filtered against 144; the plain floor_blocks_small loses its floor's four corners and keeps its objects."""
    batch = dict(VB.bridged_batch())
    for name in ("bridged", "bridged_lifted"):
        c = batch[name]
        plain = CC.cluster_model(VB.bridged_cloud(c, None)[0], c["cp"])
        filt = CC.cluster_model(VB.bridged_cloud(c)[0], c["cp"])
        assert (plain["n_objects"], plain["sizes"].tolist()) == (1, [49, 0, 0, 0]), name
        assert (filt["n_objects"], filt["sizes"].tolist()) == (2, [27, 16, 0, 0]), name
    c = batch["bridged"]
    assert VB.bridged_filter_model(c)["counts"].tolist() == [196, 0, 13, 0, 183, 0]
    origin = PF.origin_of(c)
    fits = [PF.fit_model(VB.bridged_cloud(c, fp)[0], c["fp"], origin) for fp in (VB.BRIDGED_FILTER, None)]
    assert [f["n_inliers"] for f in fits] == [140, 144] and all(f["found"] and PF.is_level(f["plane"]) for f in fits)
    for m in VB.cluster_models([("bridged", c)], fitted=True):
        assert (m["cluster"]["n_objects"], m["cluster"]["sizes"].tolist()) == (2, [27, 16, 0, 0])
    c = batch["floor_blocks_small"]
    m = VB.bridged_filter_model(c)
    assert m["counts"].tolist() == [187, 0, 4, 0, 183, 0]
    gone = m["ijk"][~m["keep"]]
    assert sorted(map(tuple, gone)) == [(0, 0, 0), (0, 11, 0), (11, 0, 0), (11, 11, 0)]
    plain = CC.cluster_model(VB.bridged_cloud(c, None)[0], c["cp"])
    filt = CC.cluster_model(VB.bridged_cloud(c)[0], c["cp"])
    assert plain["sizes"].tolist() == filt["sizes"].tolist() == [27, 16, 0, 0]


def _slot_bits(c, rows) -> set:
    """Where the bitmap slot of capture `c` holds the voxels `rows` of its unfiltered cloud: camera 0's lattice from bit 0, x-major
    and z fastest, camera 1's from the next boundary of 4096 words (the voxeliser's bitmap)."""
    m = c["model"]
    words0 = -(-int(np.prod(m["dims"][0])) // 32) if m["dims"][0] is not None else 0
    first = [0, -(-words0 // WORDS_PER_BLOCK) * WORDS_PER_BLOCK * 32]
    return {first[m["cam"][r]] + VF.bit_of(m["ijk"][r], m["dims"][m["cam"][r]]) for r in rows}


def _masked_survivors(c) -> np.ndarray:
    rows = c["rows"][(c["rows"] >= 0) & (c["mask"] != 0)]
    return np.unique(rows[c["model"]["keep"][rows]])


def test_a_kernel_that_reads_slot_0_for_every_capture_loses_voxels():
    """Condition 3.  Slot 0 holds three surviving voxels, forwards (last_word) and reversed (cam1_block_neighbours): a capture
    with more than three masked surviving voxels cannot find them all in it.  That is every non-empty, not wholly pruned capture
    but the other end's, which has three survivors itself; for it -- and for all the others too -- the statement is made bit by
    bit: some masked surviving voxel lies where slot 0's bitmap has no bit."""
    for reverse in (False, True):
        batch = VB.lattice_batch(reverse)
        name0, c0 = batch[0]
        assert name0 == ("cam1_block_neighbours" if reverse else "last_word") and c0["model"]["keep"].sum() == 3
        slot0 = _slot_bits(c0, np.flatnonzero(c0["model"]["keep"]))
        assert len(slot0) == 3
        checked = 0
        for name, c in batch[1:]:
            if c["model"]["keep"].sum() == 0:
                continue
            rows = _masked_survivors(c)
            assert len(rows) == len(VB.masked_model(c)[0])
            print(reverse, name, "masked surviving voxels", len(rows), "of them in slot 0's bitmap", len(_slot_bits(c, rows) & slot0))
            if c["model"]["keep"].sum() > 3:
                assert len(rows) > 3, name
            assert _slot_bits(c, rows) - slot0, name
            for j in range(2):  # ... and the same for both label lists
                lab = c["rows"][(c["rows"] >= 0) & (c["labels"] == j + 1)]
                lab = np.unique(lab[c["model"]["keep"][lab]])
                assert _slot_bits(c, lab) - slot0, (name, j)
            checked += 1
        assert checked == 5


def _mixed(m) -> bool:
    return 0 < m["keep"].sum() < len(m["keep"])


def test_coverage():
    """Condition 4."""
    from tests import test_gpu_voxel_filter_batches as G

    lattice, bridged = VB.lattice_batch(), VB.bridged_batch()
    assert sum(_mixed(c["model"]) for _, c in lattice) >= 3
    assert sum(_mixed(VB.bridged_filter_model(c)) for _, c in bridged) >= 3
    assert sum(c["model"]["counts"][1] > 0 for _, c in lattice) >= 2
    names = [n for n, _ in lattice]
    for name in ("empty", "one_voxel"):
        k = names.index(name)
        assert 0 < k < len(names) - 1 and lattice[k][1]["model"]["keep"].sum() == 0
        assert _mixed(lattice[k - 1][1]["model"]) and _mixed(lattice[k + 1][1]["model"]), name
    assert len(lattice[names.index("empty")][1]["points"]) == 0
    assert lattice[names.index("one_voxel")][1]["model"]["counts"].tolist() == [1, 0, 1, 0, 0, 0]
    # the lists the GPU file iterates over are the whole batches, in both directions
    for reverse in (False, True):
        assert [n for n, _ in G.LATTICE[reverse]] == [n for n, _ in VB.lattice_batch(reverse)] and len(G.LATTICE[reverse]) == 8
        assert [n for n, _ in G.BRIDGED[reverse]] == [n for n, _ in VB.bridged_batch(reverse)] and len(G.BRIDGED[reverse]) == 4
    # the capture of the life-cycle tests outgrows a slot sized by the largest lattice of lattice_batch, and is pruned in part
    big = VB.outgrowing_case()
    words = lambda m: sum(-(-(-(-int(np.prod(d)) // 32)) // WORDS_PER_BLOCK) * WORDS_PER_BLOCK for d in m["dims"] if d is not None)
    largest = max(words(c["model"]) for _, c in lattice)
    slot = ((largest + largest // 4) // WORDS_PER_BLOCK + 1) * WORDS_PER_BLOCK  # (the batch chain's rule: a quarter of slack, whole blocks)
    need = -(-int(np.prod(big["model"]["dims"][0])) // 32)
    print("largest lattice", largest, "words, slot", slot, "the outgrowing capture", need)
    assert need > slot and _mixed(big["model"]) and len(VB.masked_model(big)[0]) > 0
