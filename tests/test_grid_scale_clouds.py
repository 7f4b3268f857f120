"""The room-scale inputs (tests/grid_scale_clouds.py) reach the regimes of the grid build they are made for, and stay real
searchable scenes.

CPU only.  For every case the numpy model of desc_finish / desc_next must report the intended regime (scan tiles beyond the
work-groups of k_cell_scan, the cell cap, doubled cells, the transitions between cell sizes), the oracle must find more
than 10 hypotheses on the samples, and the oracle's time is printed: a mistargeted or too costly case fails here before any
GPU time is spent.  The constants the model restates are read out of the sources.
"""
import os
import re
import time

import numpy as np
import pytest

from tests import grid_scale_clouds as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "agile_grasp_amd", "csrc")
ORACLE_BUDGET_S = 20.0  # per case, on at most 16 threads


def _oracle(c, r_hands=gs.R_HANDS, xyz=None):
    from oracle import oracle_py as O

    p = O.default_params(c.cam_origins, num_threads=min(os.cpu_count() or 1, 16), nn_radius_hands=r_hands)
    t0 = time.perf_counter()
    ref = O.find_hands(p, c.xyz if xyz is None else xyz, c.cam, c.samples)
    dt = time.perf_counter() - t0
    print(f"oracle: {len(c.samples)} samples, {len(ref['hyps'])} hypotheses, {dt:.2f} s")
    assert len(ref["hyps"]) > 10
    assert dt < ORACLE_BUDGET_S
    return ref


def _extras_keep_clear(c):
    """every extra point keeps more than r_hands + r_taubin from every sample"""
    q = c.xyz[c.samples].astype(np.float64)
    for e in c.xyz[c.n_scene:].astype(np.float64):
        if np.isfinite(e).all():
            assert (((q - e) ** 2).sum(1) > (gs.R_HANDS + gs.R_TAUBIN) ** 2).all()


def test_the_model_restates_the_sources_constants():
    grid = open(os.path.join(CSRC, "grid.hip")).read()
    hdr = open(os.path.join(CSRC, "agh_internal.h")).read()
    assert re.search(r"constexpr int kCellCap = 1 << (\d+);", hdr).group(1) == "21" and gs.CELL_CAP == 1 << 21
    assert int(re.search(r"constexpr int kGridMargin = (\d+);", hdr).group(1)) == gs.GRID_MARGIN
    assert int(re.search(r"constexpr int kScanBlock = (\d+);", grid).group(1)) == gs.SCAN_BLOCK
    assert re.search(r"std::max\(0\.02, c->p\.nn_radius_hands / 4\.0\)", grid)
    assert re.search(r"dim3\(C == 1 \? (\d+) : (\d+), C\)", grid).groups() == (str(gs.SCAN_GROUPS_SINGLE), str(gs.SCAN_GROUPS_BATCH))
    assert "u.dim[a] - t.dim[a] <= 4 * kGridMargin" in grid


def test_model_on_the_known_boxes():
    """the boxes of the older suite, as the issue's table lists them"""
    for name, dims, tiles in (("tiny", (10, 11, 11), 1), ("small", (15, 11, 13), 1)):
        d = gs.desc_finish(gs.extrema(gs.scene(name).xyz), gs.BASE_CELL)
        assert (d.dim, d.tiles, d.cell) == (dims, tiles, 0.02)
    # an empty cloud, and one without a finite point: one cell at the origin
    for xyz in (np.zeros((0, 3), np.float32), np.full((4, 3), np.nan, np.float32)):
        d = gs.desc_finish(gs.extrema(xyz), gs.BASE_CELL)
        assert (d.mn, d.dim, d.cell) == ((0.0, 0.0, 0.0), (1, 1, 1), 0.02)


def test_case_a_second_pass_of_a_single_cloud():
    c = gs.case_a()
    (d, regime), = gs.GridModel().build([c.xyz])
    assert regime == "cold" and d.dim == gs.A_DIMS and d.cell == 0.02 and d.tiles == 469 > gs.SCAN_GROUPS_SINGLE
    tile = gs.cell_index(d, c.xyz) // gs.SCAN_BLOCK
    for t in (tile[:c.n_scene], tile[c.samples]):  # scene points and samples in tiles of the first and of the second pass
        assert (t < gs.SCAN_GROUPS_SINGLE).sum() > 10 and (t >= gs.SCAN_GROUPS_SINGLE).sum() > 10
    assert tile.max() == 468  # (the high corner: the last tile is not empty)
    _extras_keep_clear(c)
    _oracle(c)


def test_case_b_the_cap_edge():
    fit, over = gs.case_b("fit"), gs.case_b("over")
    m = gs.GridModel()
    (d, regime), = m.build([fit.xyz])
    assert regime == "cold" and d.dim == (128, 128, 128) and d.cell == 0.02 and d.ncell == gs.CELL_CAP and d.tiles == 512
    assert m.next[0].dim == (128, 128, 128) and m.next[0].mn == d.mn  # kept without padding: m = 0
    (d2, regime), = m.build([fit.xyz])
    assert regime == "kept" and d2.as_dict() == d.as_dict()
    (d3, regime), = m.build([over.xyz])
    assert regime == "miss" and d3.open == 2 and d3.dim == (128, 128, 128)  # the high x face
    assert m.next[0].cell == 0.04 and m.next[0].dim == (65 + 4, 64 + 4, 64 + 4)
    (d4, regime), = m.build([over.xyz])
    assert regime == "kept" and d4.cell == 0.04 and m.stats == {"builds": 4, "cold": 1, "misses": 1}
    (dc, regime), = gs.GridModel().build([over.xyz])
    assert regime == "cold" and dc.cell == 0.04 and dc.dim == (65, 64, 64)
    for c in (fit, over):
        _extras_keep_clear(c)
        _oracle(c)


@pytest.mark.parametrize("which", ["0.04", "0.08", "1.28-one", "1.28-two"])
def test_case_c_doubled_cells(which):
    c = gs.case_c(which)
    (d, regime), = gs.GridModel().build([c.xyz])
    assert regime == "cold" and d.cell == float(which[:4])
    q = c.xyz[c.samples]
    if which in gs.C_CELLS:
        assert d.dim == gs.C_DIMS
        assert gs.crosses_cell_face(d, q).sum() > 10 and (~gs.crosses_cell_face(d, q, 0.0)).all()
    else:
        cells = np.unique(gs.cell_index(d, c.xyz[:c.n_scene]))
        assert len(cells) == (1 if which == "1.28-one" else 2)  # the whole scene in one cell / in two
        assert max(d.dim) <= 128
        if which == "1.28-two":
            assert gs.crosses_cell_face(d, q).sum() > 10
            assert len(np.unique(gs.cell_index(d, q))) == 2  # samples on both sides of the face
    _extras_keep_clear(c)
    _oracle(c)


def test_case_d_transitions_between_cell_sizes():
    from tests.test_gpu_grid_kept import _near_open_faces

    table, room = gs.case_d()
    m = gs.GridModel()
    seq = [m.build([x])[0] for x in (table.xyz, room.xyz, room.xyz, table.xyz, table.xyz)]
    assert [r for _, r in seq] == ["cold", "miss", "kept", "refit", "kept"]
    assert [d.cell for d, _ in seq] == [0.02, 0.02, 0.04, 0.04, 0.02]
    assert seq[1][0].open == 63 and seq[3][0].open == 0  # the room leaves the table's box through all six faces
    assert seq[2][0].dim == tuple(v + 4 for v in gs.C_DIMS) and seq[4][0].dim == (19, 15, 17)
    assert m.stats == {"builds": 5, "cold": 1, "misses": 1}
    u = seq[1][0]
    near = _near_open_faces(room.xyz, np.array(u.mn), np.array(u.mn) + np.array(u.dim) * u.cell, 12)
    assert near.size == 24
    _oracle(table)
    room.samples = np.union1d(room.samples, near).astype(np.int32)
    _oracle(room)


def test_case_e_the_other_base_cell():
    c = gs.case_e()
    assert gs.base_cell(gs.E_R_HANDS) == 0.025
    (d, regime), = gs.GridModel(gs.E_R_HANDS).build([c.xyz])
    assert regime == "cold" and d.cell == 0.05 and d.dim == gs.C_DIMS
    (d2, _), = gs.GridModel().build([c.xyz])
    assert d2.cell == 0.08  # (the same room from the 0.02 base: another cell)
    _extras_keep_clear(c)
    _oracle(c, gs.E_R_HANDS)


@pytest.mark.parametrize("n", [2, 8])
def test_case_f_batches(n):
    clouds = gs.case_f(n)
    m = gs.GridModel()
    first = m.build([c.xyz for c in clouds])
    tiles = [d.tiles for d, _ in first]
    assert all(r == "cold" for _, r in first)
    assert max(tiles) > gs.SCAN_GROUPS_SINGLE and sum(gs.SCAN_GROUPS_BATCH < t <= gs.SCAN_GROUPS_SINGLE for t in tiles) >= (1 if n == 2 else 2)
    if n == 8:
        assert sorted(d.cell for d, _ in first) == [0.02] * 6 + [0.04, 1.28]
        assert min(tiles) == 1 and first[4][0].dim == (1, 1, 1) and len(clouds[4].xyz) == 0
    second = m.build([c.xyz for c in clouds])
    # (an empty cloud has no box to keep: its descriptor is decided anew every time)
    assert [r for _, r in second] == ["refit" if len(c.xyz) == 0 else "kept" for c in clouds]
    k = gs.F_MOVED[n]
    moved = [c.xyz + gs.F_MOVE if j == k else c.xyz for j, c in enumerate(clouds)]
    third = m.build(moved)
    assert [r for _, r in third] == ["miss" if j == k else r for j, (_, r) in enumerate(second)]
    assert third[k][0].tiles > gs.SCAN_GROUPS_BATCH and m.stats == {"builds": 3, "cold": 1, "misses": 1}
    t0 = time.perf_counter()
    for c in clouds:
        if len(c.samples):
            _extras_keep_clear(c)
            _oracle(c)
    assert time.perf_counter() - t0 < ORACLE_BUDGET_S


def test_case_g_raw_captures_for_the_chains():
    from oracle import oracle_py as O

    caps = gs.case_g()
    cells, tiles = [], []
    for rc in caps:
        vox, _cam = O.preprocess(rc.xyz, rc.size_left, rc.workspace)
        d = gs.desc_finish(gs.extrema(vox), gs.BASE_CELL)
        cells.append(d.cell)
        tiles.append(d.tiles)
    print("case G:", cells, tiles)
    assert cells == list(gs.G_CELLS)
    assert tiles[1] > gs.SCAN_GROUPS_SINGLE and tiles[2] > gs.SCAN_GROUPS_SINGLE and tiles[0] > gs.SCAN_GROUPS_BATCH


@pytest.mark.parametrize("which", ["1e6", "1e30", "mixed"])
def test_case_h_extreme_extents(which):
    c = gs.case_h(which)
    m = gs.GridModel()
    (d, regime), = m.build([c.xyz])
    assert regime == "cold" and max(d.dim) <= 128 and d.ncell <= gs.CELL_CAP
    assert d.cell == 0.02 * 2.0 ** {"1e6": 19, "1e30": 100, "mixed": 100}[which]
    assert len(np.unique(gs.cell_index(d, c.xyz[:c.n_scene][np.isfinite(c.xyz[:c.n_scene]).all(1)]))) == 1
    _oracle(c)
