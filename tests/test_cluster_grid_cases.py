"""The cases of tests/cluster_grid_cases.py are in the regimes their names say, and the faults those regimes are there for would
change their labels: shown with the numpy models alone (no GPU)."""
import numpy as np
import pytest

from tests import cluster_cases as CC
from tests import cluster_grid_cases as G
from tests import grid_scale_clouds as gs

CASES = G.cases()


def _cold(name):
    """a case built cold: its model, descriptor and link regime"""
    mo = G.model(name)
    d = gs.desc_finish(gs.extrema(mo["xyz"]), gs.BASE_CELL)
    return mo, d, G.link_regime(mo["xyz"], d, mo["case"]["cp"])


def _changed(mo, d, fault):
    f = G.faulty_model(mo["xyz"], d, mo["case"]["cp"], fault)
    return f["n_components"] != mo["m"]["n_components"] or not np.array_equal(f["labels"], mo["m"]["labels"])


def test_every_case_is_named():
    assert set(CASES) == {"reach_three", "reach_two_edges", "reach_one_edges", "reach_two_exact", "owner_tiles", "big_component", "many_roots_min1_K64", "many_roots_min1_K1",
                          "many_roots_min2_K64", "many_roots_min2_K1", "doubled_cells_0.04_tol0.05", "doubled_cells_0.04_tol0.011",
                          "doubled_cells_0.08_tol0.05", "doubled_cells_0.08_tol0.011"}
    assert [n for n, _, _ in G.sequence()] == ["small_cold", "out_miss", "out_kept", "room_miss", "room_kept", "small_refit", "small_kept"]
    for c in list(CASES.values()) + [c for _, c, _ in G.sequence()]:
        assert 0 < c["cp"]["tolerance"] <= 0.05 and c["dense"] and np.array_equal(c["workspace"], G.M.WIDE)


def test_the_faster_union_step_is_the_union_find_it_replaced():
    """cluster_model's components against a plain union-find over the same pairs, on the old cases and on a large new one"""
    for c in list(CC.cases().values()) + [CASES["big_component"]]:
        xyz, _ = CC.voxel_cloud(c)
        fg, a, b = CC.adjacent_pairs(xyz, c["cp"])
        parent = list(range(len(fg)))

        def find(q):
            while parent[q] != q:
                parent[q] = parent[parent[q]]
                q = parent[q]
            return q

        for i, j in zip(a.tolist(), b.tolist()):
            i, j = find(i), find(j)
            if i != j:
                parent[max(i, j)] = min(i, j)
        assert np.array_equal(CC.component_roots(len(fg), a, b), [find(q) for q in range(len(fg))])


@pytest.mark.parametrize("name", sorted(CASES) + [n for n, _, _ in G.sequence()])
def test_no_adjacent_pair_lies_beyond_the_reach(name):
    """what k_cluster_link relies on, in every descriptor the tests use: the ends of an adjacent pair are at most `reach` cells
    apart along every axis -- also where an end is clamped into a border cell"""
    if name in CASES:
        mo, d, r = _cold(name)
    else:
        k = [n for n, _, _ in G.sequence()].index(name)
        mo, d = G.model(name), G.sequence_descs()[k][0]
        r = G.link_regime(mo["xyz"], d, mo["case"]["cp"])
    assert len(r["offsets"]) > 0 and np.abs(r["offsets"]).max() <= r["reach"]
    assert r["owners"].sum() == len(mo["xyz"]) and r["owners_fg"].sum() == mo["m"]["n_foreground"]


def _at_the_x_edges(r, span):
    """of the pairs `span` cells long along x: is the partner (the smaller index) in the first / in the last cell of the x run
    of the owner's group?"""
    fg, a, b = r["pairs"]
    long_x = np.abs(r["offsets"][:, 0]) == span
    ca, cb = r["cells"][fg[a[long_x]], 0], r["cells"][fg[b[long_x]], 0]
    lo, hi = G.x_window(cb, r["reach"])
    return ca == lo, ca == hi


@pytest.mark.parametrize("span", [1, 2, 3])
def test_bridges_of_reach_cells(span):
    name = G.BRIDGE_CASES[span]
    mo, d, r = _cold(name)
    m, cp = mo["m"], mo["case"]["cp"]
    n = len(G.bridges(span))
    size = 4 if G.BRIDGE_SETS[span]["buddy"] else 2
    assert d.cell == 0.02 and r["reach"] == span == G.reach_of(cp["tolerance"], 0.02) and n == (8 if span == 3 else 6)
    assert m["n_components"] == n and list(m["sizes"][:n]) == [size] * n
    # one pair per bridge is `span` cells long: along every axis (and at the corner), with the larger index on either side
    far = r["offsets"][np.abs(r["offsets"]).max(1) == span]
    want = [tuple(sgn * span * np.eye(3, dtype=int)[ax]) for ax in range(3) for sgn in (1, -1)]
    want += [(3, 2, 2), (-3, -2, -2)] if span == 3 else []
    assert sorted(map(tuple, far.tolist())) == sorted(want)
    fg, a, b = r["pairs"]
    d2 = CC.d2_f32(mo["xyz"][fg[a]], mo["xyz"][fg[b]]).diagonal()[np.abs(r["offsets"]).max(1) == span]
    assert d2.max() < 0.995 * CC.tol2(cp["tolerance"])  # (well inside the bound: at span 3, 49.8 mm at the corner)
    assert r["candidates"].max() <= 8  # (at span 3: 49 rows, nearly all of them empty)
    # along x the partner is the FIRST cell of the group's run where the larger index is on the + side, and the LAST where it
    # is on the - side: x and, at span 3, corner
    first, last = _at_the_x_edges(r, span)
    assert (first != last).all() and first.sum() == last.sum() == (2 if span == 3 else 1)
    # every bridge is needed; a window a cell short finds none of those on its side -- per axis, and on all axes
    x_and_corner = 2 if span == 3 else 1
    for fault in ("plus_side_short", "minus_side_short"):
        lost = [G.faulty_model(mo["xyz"], d, cp, fault, axes=(ax,))["n_components"] - n for ax in range(3)]
        assert lost == [x_and_corner, 1, 1]
        assert G.faulty_model(mo["xyz"], d, cp, fault)["n_components"] == n + n // 2
    if span == 3:
        assert G.faulty_model(mo["xyz"], d, cp, "two_cells")["n_components"] == 16


def test_reach_two_exact():
    """tolerance 0.04 = two cells exactly: floor(0.04 * 50 * 1.0001) + 1 = 3, the margin at work.  Of the 21 pairs ten voxels of
    4 mm apart, float32 puts some on or below the bound and some above it; none is more than two cells long."""
    mo, d, r = _cold("reach_two_exact")
    assert d.cell == 0.02 and r["reach"] == 3 == G.reach_of(0.04, 0.02)
    fg, a, b = r["pairs"]
    cam0 = mo["cams"][fg[a]] == 0  # (the lines of ten are camera 0's)
    n_ten = int(cam0.sum())
    assert 0 < n_ten < 21 and len(a) - n_ten == 8
    assert np.abs(r["offsets"]).max() == 2
    assert mo["m"]["n_components"] == 1 + (24 - n_ten)


def test_owner_tiles():
    mo, d, r = _cold("owner_tiles")
    assert d.dim == (2, 3, 1) and r["reach"] == 1
    g = {tuple(q): k for k, q in enumerate(r["groups"])}
    one, two = g[(0, 0, 0)], g[(0, 2, 0)]
    # group one: 1372 owners, five full tiles and one of 92; group two: 1008, its first cell 420 voxels of background
    assert r["owners"][one] == 1372 > 5 * G.TILE and r["owners"][one] % G.TILE == 92 and r["owners_fg"][one] == 392
    assert r["owners"][two] == 1008 > 3 * G.TILE and r["owners"][two] % G.TILE == 240
    assert r["first_cell"][two] == 420 >= G.TILE and r["first_cell_fg"][two] == 0 and r["owners_fg"][two] == 168
    assert r["candidates"].max() == 1372
    assert mo["m"]["n_components"] == 2 and list(mo["m"]["sizes"][:2]) == [392, 168]
    assert _changed(mo, d, "first_tile")
    # (the second group's foreground lies wholly behind the first tile: without the later tiles none of it is linked)
    f = G.faulty_model(mo["xyz"], d, mo["case"]["cp"], "first_tile")
    assert f["n_components"] > 168


def test_big_component():
    mo, d, r = _cold("big_component")
    m = mo["m"]
    assert d.dim == (23, 23, 2) and r["reach"] == 1
    assert m["n_components"] == 402 and list(m["sizes"][:3]) == [22500, 5251, 2] and m["sizes"][0] >= 20000
    assert (r["groups"][:, 2] == 0).sum() == 12 * 23  # (the sheet crosses every group of the lower layer of cells)
    # the snake's voxel indices rise and fall along the walk
    xyz = mo["xyz"].astype(np.float64)
    lookup = {tuple(q): i for i, q in enumerate(np.round((xyz - np.asarray(G.ORIGIN)) / G.M.CELL).astype(int).tolist())}
    steps = np.sign(np.diff([lookup[q] for q in G.big_snake_path()]))
    assert len(steps) + 1 == 5251 and (steps > 0).sum() > 1000 and (steps < 0).sum() > 1000
    # waves of k_cluster_flatten (64 consecutive voxels) with several roots
    fg, a, b = r["pairs"]
    roots = fg[CC.component_roots(len(fg), a, b)]
    per_wave = np.bincount(np.unique(roots) // 64)
    # (a slab x = 2 i holds 20 small roots in its first 40 columns of at most 4 voxels each: 160 indices, so a wave with 7)
    assert (per_wave >= 7).sum() >= 20


@pytest.mark.parametrize("mv,K", [(1, 64), (1, 1), (2, 64), (2, 1)])
def test_many_roots(mv, K):
    mo, d, r = _cold(f"many_roots_min{mv}_K{K}")
    m = mo["m"]
    assert m["n_components"] == 2025 and m["n_qualifying"] == (2025 if mv == 1 else 1350) > 1024
    assert m["n_objects"] == K and (m["sizes"] == 3).all() and (np.diff(m["ids"]) > 0).all()  # (675 ties at the top: by id)


@pytest.mark.parametrize("cell,tol,reach", [(0.04, 0.05, 2), (0.04, 0.011, 1), (0.08, 0.05, 1), (0.08, 0.011, 1)])
def test_doubled_cells(cell, tol, reach):
    mo, d, r = _cold(f"doubled_cells_{cell}_tol{tol}")
    m = mo["m"]
    assert d.cell == cell and d.dim == (105, 105, 76) and r["reach"] == reach == np.abs(r["offsets"]).max()
    assert m["n_foreground"] == 5329
    assert list(m["sizes"][:3]) == ([4920, 400, 1] if tol == 0.05 else [3920, 1000, 400])
    if cell == 0.04:
        assert r["owners"].max() == 450 > G.TILE and r["candidates"].max() == (4620 if reach == 2 else 2592) > 10 * G.TILE
    else:
        assert r["owners"].max() == 828 > 3 * G.TILE and r["candidates"].max() == 4920 > 19 * G.TILE


def test_sequence():
    seq, descs = G.sequence(), G.sequence_descs()
    assert [regime for _, regime, _ in descs] == [want for _, _, want in seq]
    assert [d.open for d, _, _ in descs] == [0, 63, 0, 63, 0, 0, 0]
    assert [d.cell for d, _, _ in descs] == [0.02, 0.02, 0.02, 0.02, 0.04, 0.04, 0.02]
    assert [d.dim for d, _, _ in descs] == [(16, 16, 16), (20, 20, 20), (28, 27, 27), (28, 27, 27), (109, 109, 80), (109, 109, 80),
                                            (20, 20, 20)]
    assert descs[-1][2] == {"builds": 7, "cold": 1, "misses": 2}
    # the first call sizes the voxel bitmap for all of them: no call runs its chain twice, and the bitmap is never dropped
    words = [G.lattice_words(c) for _, c, _ in seq]
    assert G.bitmap_chain_runs(words) == [1] * 7 and max(words) == words[0]
    assert G.bitmap_chain_runs([words[1], words[3]]) == [1, 2]  # (the rule does tell: the room after the small lattice)
    reaches = [G.reach_of(c["cp"]["tolerance"], d.cell) for (_, c, _), (d, _, _) in zip(seq, descs)]
    assert reaches == [1, 2, 2, 3, 2, 1, 1]


def test_the_miss_clamps_what_its_parts_say():
    name, c, _ = G.sequence()[1]
    mo, d = G.model(name), G.sequence_descs()[1][0]
    r = G.link_regime(mo["xyz"], d, c["cp"])
    m = mo["m"]
    parts = G.out_parts()
    assert m["n_components"] == len(parts) == 11
    xyz = mo["xyz"].astype(np.float64)
    at = {tuple(q): i for i, q in enumerate(np.round((xyz - np.asarray(G.OUT_ORIGIN)) / G.OUT_CELL).astype(int).tolist())}
    idx = {n: np.array([at[tuple(q)] for q in np.asarray(v).tolist()]) for n, (_, v) in parts.items()}
    comp = {n: set(m["labels"][i]) for n, i in idx.items()}
    assert all(len(s) == 1 and 0 not in s for s in comp.values()) and len(set.union(*comp.values())) == 11
    clamped, cells = r["clamped"], r["cells"]
    for n in ("beyond_high_x", "beyond_low_y", "beyond_low_z", "same_border_cell_1", "same_border_cell_2", "beyond_corner"):
        assert clamped[idx[n]].all(), n
    for n in ("across_high_x", "across_low_x", "across_high_y", "across_high_z"):
        assert clamped[idx[n]].any() and not clamped[idx[n]].all(), n
    assert not clamped[idx["inside"]].any()
    both = np.concatenate([idx["same_border_cell_1"], idx["same_border_cell_2"]])
    assert (cells[both] == (19, 4, 4)).all()
    raw = G.cell_coords(d, mo["xyz"], clamp=False)[idx["beyond_corner"]]
    assert (raw[:, :2] >= 20).all() and (cells[idx["beyond_corner"]][:, :2] == 19).all()
    # a pair with one end inside (in the last cell but one) and one end clamped, through four faces
    fg, a, b = r["pairs"]
    mixed = clamped[fg[a]] != clamped[fg[b]]
    assert mixed.sum() >= 4 and (np.abs(r["offsets"][mixed]).max(1) == 1).sum() >= 4
    f = G.faulty_model(mo["xyz"], d, c["cp"], "clamped_dropped")
    assert f["n_components"] > m["n_components"] and not np.array_equal(f["labels"], m["labels"])
    # the room's miss: every voxel is clamped (the whole room lies below the kept box), and the model is the cold case's
    room, dr = G.model("room_miss"), G.sequence_descs()[3][0]
    assert G.link_regime(room["xyz"], dr, room["case"]["cp"])["clamped"].all()


def test_depth_captures_reach_their_regimes():
    steps = G.depth_steps()
    g = gs.GridModel()
    clouds = {n: G.depth_cloud(images, cell)[0] for n, (images, _, cell) in steps.items()}
    (d0, r0), = g.build([clouds["small"]])
    (d1, r1), = g.build([clouds["out"]])
    assert (r0, r1) == ("cold", "miss") and d1.open == 63 and d1.cell == 0.02
    words = [G.lattice_words(points=G.D.deproject_ref(steps[n][0]), cams=G.D.image_index(steps[n][0]), cell=steps[n][2])
             for n in ("small", "out")]
    assert G.bitmap_chain_runs(words) == [1, 1]  # (the miss is the build whose results the call returns)
    m = CC.cluster_model(clouds["out"], steps["out"][1])
    assert m["n_objects"] == 6 and m["n_components"] >= 6
    r = G.link_regime(clouds["out"], d1, steps["out"][1])
    fg = r["pairs"][0]
    assert r["reach"] == 2 and 100 < r["clamped"][fg].sum() < len(fg)  # (the outer patches: components beyond the open faces)
    dd = gs.desc_finish(gs.extrema(clouds["doubled"]), gs.BASE_CELL)
    assert dd.cell == 0.04
    m = CC.cluster_model(clouds["doubled"], steps["doubled"][1])
    assert m["n_objects"] >= 3 and m["n_foreground"] < len(clouds["doubled"])
