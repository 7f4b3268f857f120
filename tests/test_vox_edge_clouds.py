"""The voxeliser's edge captures (tests/vox_edge_clouds.py) reach the paths they are named for, on the numpy model alone.

CPU only.  tests/test_gpu_vox_edges.py holds the GPU to the references on these captures by exact equality; what is asserted here
is that the captures are where the kernels branch -- the raw scan's second pass and its carry, k_vox_emit's list cap, a lattice of
exactly 2^28 words --, that every tested size_left is visible to one rank either way, and that the two references agree.
"""
import functools

import numpy as np
import pytest

from tests import ref_numpy
from tests import vox_edge_clouds as V

RAW = [(n, dense) for n in V.RAW_BIG + V.RAW_TWINS for dense in (False, True)]


def _same(a, b):
    return len(a[0]) == len(b[0]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


@functools.lru_cache(maxsize=64)
def _ref(n, dense, size_left):
    c = V.raw_scan_case(n, dense)
    return ref_numpy.preprocess(c["points"], size_left, c["workspace"], c["cell"], dense)


def _model(c, size_left=None):
    s = c["size_left"] if size_left is None else size_left
    return c["points"], s, c["workspace"], c["cell"], c["dense"]


# ---- (a) ----

@pytest.mark.parametrize("n,dense", RAW)
def test_raw_clouds_reach_the_scan_pass_they_are_named_for(n, dense):
    c = V.raw_scan_case(n, dense)
    p, sizes = c["points"], c["sizes"]
    assert p.shape == (n, 3)
    finite = V.raw_block_counts(p)  # what k_vox_count writes (dense = 0)
    assert len(finite) == {V.M20 - 1: 1024, V.M20: 1024, V.M20 + 1: 1025, V.M20 + 1025: 1026, V.M20 + 1324: 1026}.get(n, -(-n // 1024))
    assert finite.sum() == c["n_finite"] == np.isfinite(p).all(1).sum()
    assert 0.005 < 1 - c["n_finite"] / n < 0.04  # about 1 % of the records are dropped by the NaN removal
    assert {"zero", "all_left", "beyond"} <= set(sizes) and len(set(sizes.values())) == len(sizes)
    top = n if dense else c["n_finite"]
    assert sizes["zero"] == 0 and sizes["all_left"] == top and sizes["beyond"] > top
    carries = V.scan_carries(finite)
    assert len(carries) == (1 if n > V.M20 else 0)  # the second pass runs, once, above 2^20 points
    fin = np.isfinite(p).all(1)
    if n >= V.M20 - 1:
        assert tuple(sizes) == V.RAW_BIG_SIZES[n]
        assert finite[V.NAN_BLOCK] == 0 and finite[V.FULL_BLOCK] == 1024 and 0 < finite[1023] <= 1024
        if not dense:
            assert not fin[V.M20 - 1:V.M20 + 1].any()  # NaNs at the last point of the first pass and the first of the second
        if n > V.M20 + 1:
            first = V.M20 + int(np.argmax(fin[V.M20:]))  # the first finite point of raw block 1024
            assert first == V.M20 + (0 if dense else 1)
            assert sizes["carry"] == (first if dense else carries[0]) and fin[:first].sum() == carries[0]
            assert sizes["carry-1"] == sizes["carry"] - 1 and sizes["carry+1"] == sizes["carry"] + 1
        elif n == V.M20 + 1:  # block 1024 is one record: a NaN (count 0, carry = every finite point) or, dense, the last rank
            assert finite[1024] == (1 if dense else 0) and carries[0] == c["n_finite"] - finite[1024]
            assert sizes["carry-1"] == top - 1 and (dense or sizes["all_left"] == carries[0])
        if n <= V.M20 + 1:
            s = sizes["block1023"]
            assert s == (1023 * 1024 if dense else finite[:1023].sum()) and fin[1023 * 1024]
        if n == V.M20 + 1025:
            assert sizes["block1025"] == top - 1 and finite[1025] == 1
        if n == V.M20 + 1324:
            r = V.MID_WAVE
            assert r // 1024 == 1025 and r % 64 == 29 and r % 256 // 64 == 2 and fin[r]
            assert sizes["mid_wave"] == (r if dense else fin[:r].sum()) and sizes["mid_wave"] + 64 < top
    else:
        for r in (64, 256, 1024):
            if r < n:  # the first lane of a wave / round / block, with NaNs ahead of it
                assert fin[r] and sizes["raw%d" % r] == (r if dense else fin[:r].sum()) and fin[:r].sum() < r
        ranks = {s for s in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025) if s + 1 <= top}
        assert ranks <= set(sizes.values())
    # the markers: every finite point within 64 ranks of a tested size_left, each alone in its voxel whatever the lattice's origin
    order = np.arange(n) if dense else np.flatnonzero(fin)
    want = set()
    for s in sizes.values():
        want |= {int(i) for i in order[max(s - 64, 0):min(s + 64, len(order))] if fin[i]}
    assert want == {int(i) for i in c["markers"]}
    m = p[c["markers"]].astype(np.float64)
    assert (m[:, 0] > 0.09).all() and (np.abs(p[fin][:, 0]) < 0.3).all()
    d = np.abs(m[:, None, :2] - m[None, :, :2]).max(-1) + np.eye(len(m))
    assert d.min() > 1.99 * c["cell"]  # two cells apart on the sheet
    others = np.delete(p, c["markers"], axis=0)
    assert np.nanmax(others[np.isfinite(others).all(1)]) < 0.061  # ... and more than that away from the cube


@pytest.mark.parametrize("n,dense", RAW)
def test_every_size_left_is_visible_to_one_rank(n, dense):
    """ref_numpy.preprocess at size_left - 1 and at size_left + 1 each differ from the result at size_left: a rank off by one
    either way would fail the GPU test.  The exceptions are the ends, by construction: nothing lies below rank 0, and no point has
    the rank `all_left` or one beyond it, so there the neighbour that cannot differ is asserted to be equal instead."""
    c = V.raw_scan_case(n, dense)
    top = n if dense else c["n_finite"]
    for name, s in c["sizes"].items():
        lo, hi = V.moved_point_is_kept(c, s - 1), V.moved_point_is_kept(c, s)
        if name == "zero":
            assert hi and not lo
        elif s == top:
            assert lo and not hi, name
        elif s > top:
            assert not lo and not hi, name
        else:
            assert lo and hi, name
        here = _ref(n, dense, s)
        if s > 0:
            assert _same(_ref(n, dense, s - 1), here) == (not lo), name
        assert _same(_ref(n, dense, s + 1), here) == (not hi), name


# ---- (b) ----

def test_emit_cases_sit_at_the_list_cap():
    e = V.emit_cases()
    pop = {k: V.block_popcounts(*_model(c)) for k, c in e.items()}
    words = {k: V.lattice_words(*_model(c)) for k, c in e.items()}
    cap = V.LIST_CAP
    assert [list(pop["k%d" % k]) for k in (4095, 4096, 4097)] == [[cap - 1], [cap], [cap + 1]]
    assert list(pop["first_quarter"]) == [cap + 1] and list(pop["last_quarter"]) == [1, cap + 1]
    assert list(pop["two_cameras"]) == [cap + 1, 100] and list(pop["three_blocks_cap"]) == [50, cap, 62]
    assert list(pop["three_blocks"]) == [50, 5000, 62]
    assert all(words[k] == len(pop[k]) * V.WORDS_PER_BLOCK for k in e)
    for k in ("k4095", "k4096", "k4097"):  # 64 x 64 x 32: exactly one block, its first and its last bit set
        (_s, _c, pos, dim), = V.M.bit_positions(e[k]["points"], V.M.camera_ids(e[k]["points"], e[k]["size_left"], False),
                                                e[k]["workspace"], e[k]["cell"])
        assert list(dim) == [64, 64, 32] and pos.min() == 0 and pos.max() == V.BLOCK_BITS - 1
    # the quarters: the waves of k_vox_emit that count nothing (a wave reads 1024 of the block's words)
    for k, blk, wave in (("first_quarter", 0, 0), ("last_quarter", 1, 3)):
        (_s, _c, pos, dim), = V.M.bit_positions(e[k]["points"], np.zeros(len(e[k]["points"]), np.int32), e[k]["workspace"], e[k]["cell"])
        inblk = pos[pos // V.BLOCK_BITS == blk] % V.BLOCK_BITS
        assert set(inblk // (1024 * 32)) == {wave}
    c = e["two_cameras"]
    cams = V.M.camera_ids(c["points"], c["size_left"], False)
    assert (cams == 0).sum() == cap + 1 and (cams == 1).sum() == 100
    for k in ("three_blocks", "three_blocks_cap"):
        (_s, _c, pos, dim), = V.M.bit_positions(e[k]["points"], np.zeros(len(e[k]["points"]), np.int32), e[k]["workspace"], e[k]["cell"])
        assert list(dim) == [192, 64, 32] and {2 * V.BLOCK_BITS - 1, 2 * V.BLOCK_BITS, 3 * V.BLOCK_BITS - 1, 0} <= set(pos)


@pytest.mark.parametrize("name", sorted(V.emit_cases()))
def test_emit_cases_references_agree(name):
    from oracle import oracle_py as orc

    c = V.emit_cases()[name]
    a = ref_numpy.preprocess(*_model(c))
    assert _same(orc.preprocess(*_model(c)), a) and len(a[0]) == V.block_popcounts(*_model(c)).sum()


# ---- (c) ----

def test_limit_cases_sit_at_the_word_limit():
    L = V.limit_cases()
    words = {k: V.lattice_words(*_model(c)) for k, c in L.items()}
    assert words["fits_one"] == words["fits_two"] == V.MAX_WORDS == 1 << 28
    assert words["over_one"] > V.MAX_WORDS and words["over_two"] > V.MAX_WORDS
    dims = {k: [list(d) for _s, _c, _p, d in V.M.bit_positions(c["points"], V.M.camera_ids(c["points"], c["size_left"], False),
                                                               c["workspace"], c["cell"])] for k, c in L.items()}
    assert dims["fits_one"] == [[2048, 2048, 2048]] and dims["over_one"] == [[2049, 2048, 2048]]
    assert dims["fits_two"] == [[2048, 2048, 1024]] * 2 and dims["over_two"] == [[2048, 2048, 1024], [2048, 2048, 1025]]
    # over_two's cameras each pass vox_lattice's product check (below 2^33 bits): it is their sum that is refused
    assert 2048 * 2048 * 1025 < 1 << 33 < 2049 * 2048 * 2048
    pop = V.block_popcounts(*_model(L["fits_one"]))
    assert len(pop) == 1 << 16 and pop[0] >= 1 and pop[-1] == 2 and pop.sum() == len(L["fits_one"]["points"]) == 12
    (_s, _c, pos, _d), = V.M.bit_positions(L["fits_one"]["points"], np.zeros(12, np.int32), L["fits_one"]["workspace"], V.LIMIT_CELL)
    assert {0, (1 << 33) - 1, (1 << 33) - 2, 1 << 32, (1 << 32) + 1, (1 << 32) - 1} <= set(int(x) for x in pos)
    pop = V.block_popcounts(*_model(L["fits_two"]))
    assert len(pop) == 1 << 16 and pop[(1 << 15) - 1] == 2 and pop[1 << 15] >= 1 and pop[-1] == 2
    for k in ("fits_one", "over_one", "fits_two", "over_two"):  # every coordinate exact in float32 and in double
        p = L[k]["points"].astype(np.float64)
        assert np.array_equal(p * 512, np.round(p * 512)) and len(p) <= 26
    # after_big: small enough for the kept 2^28-word bitmap to be dropped after it (cap > 8 * last + 2^20)
    assert V.MAX_WORDS > 8 * words["after_big"] + (1 << 20) and words["after_big"] > 0


@pytest.mark.parametrize("name", sorted(V.limit_cases()))
def test_limit_cases_references_agree(name):
    from oracle import oracle_py as orc

    c = V.limit_cases()[name]
    a = ref_numpy.preprocess(*_model(c))
    assert _same(orc.preprocess(*_model(c)), a) and len(a[0]) > 0
    if name != "after_big":
        assert len(a[0]) == len(c["points"])  # every point is a voxel of its own


# ---- the references on (a) ----

@pytest.mark.parametrize("n,dense", [(n, d) for n in V.RAW_TWINS for d in (False, True)] + [(V.M20 + 1025, False)])
def test_raw_clouds_references_agree(n, dense):
    from oracle import oracle_py as orc

    c = V.raw_scan_case(n, dense)
    names = list(c["sizes"]) if n < V.M20 else ["carry"]  # (one large cloud: the oracle takes seconds on it)
    for name in names:
        s = c["sizes"][name]
        assert _same(orc.preprocess(*_model(c, s)), _ref(n, dense, s)), name


# ---- (d) ----

def test_batch_mixes():
    b = V.batch_mixes()
    assert set(b) == {"sizes", "emit"}
    for name, batch in b.items():
        assert len({c["cell"] for _n, c, _s in batch}) == 1, name  # cell_size must be equal across a batch
    sizes = {n: c for n, c, _s in b["sizes"]}
    assert [n for n, _c, _s in b["sizes"]] == ["big", "one_point", "empty", "all_nan", "dense", "twin"]
    assert len(sizes["big"]["points"]) == V.M20 + 1025 and len(sizes["one_point"]["points"]) == 1 and len(sizes["empty"]["points"]) == 0
    assert not np.isfinite(sizes["all_nan"]["points"]).all(1).any() and sizes["dense"]["dense"] and len(sizes["twin"]["points"]) == 1025
    assert dict((n, s) for n, _c, s in b["sizes"])["big"] == V.scan_carries(V.raw_block_counts(sizes["big"]["points"]))[0]
    # the emit batch: slots sized by the three-block lattice, so the one-block captures have empty blocks behind their lattice
    words = [V.lattice_words(*_model(c)) for _n, c, _s in b["emit"]]
    assert words == [V.WORDS_PER_BLOCK, V.WORDS_PER_BLOCK, 3 * V.WORDS_PER_BLOCK]
    assert [int(V.block_popcounts(*_model(c)).max()) for _n, c, _s in b["emit"]] == [4097, 4095, 5000]
