"""The grid build at room scale (tests/grid_scale_clouds.py): scans of more tiles than k_cell_scan has work-groups, the cell cap,
doubled cells and the transitions between cell sizes, for single clouds, batches and the fused localize chains.  Every build
is held against the oracle bit for bit, and agh_get_grid_desc / agh_get_grid_stats against the numpy model of desc_finish /
desc_next -- so each test proves on the device that it reached the regime it is named after."""
import numpy as np
import pytest

from tests import grid_scale_clouds as gs
from tests.test_gpu_grid_kept import _assert_hyps_equal, _near_open_faces

pytestmark = pytest.mark.gpu

FRAME_FIELDS = ("valid", "n_nb", "majority_cam", "max_index", "params", "eigenvalue", "normal", "axis", "binormal")


def _params(cams, r_hands=gs.R_HANDS):
    from oracle import oracle_py as O

    return O.default_params(cams, nn_radius_hands=r_hands)


def _context(cams, r_hands=gs.R_HANDS):
    from agile_grasp_amd import binding

    return binding.Context(cams) if r_hands == gs.R_HANDS else binding.Context(cams, nn_radius_hands=r_hands)


def _search(ctx, c, samples, r_hands=gs.R_HANDS, antipodal=False):
    """The search of `samples` on the context's cloud (c's) against the oracle: frames, neighbour counts, hypotheses."""
    from oracle import oracle_py as O

    hyps = ctx.find_hands(samples, calculates_antipodal=antipodal)
    ref = O.find_hands(_params(c.cam_origins, r_hands), c.xyz, c.cam, samples, calculates_antipodal=antipodal)
    fr = ctx.frames()
    for f in FRAME_FIELDS:
        assert np.array_equal(fr[f], ref["frames"][f], equal_nan=True), f
    nt, nh = ctx.neighbor_counts()
    assert np.array_equal(nt, ref["frames"]["n_nb"]) and np.array_equal(nh, ref["nh"])
    _assert_hyps_equal(hyps, ref["hyps"])
    return len(hyps)


def _build(ctx, model, c, regime, samples=None, r_hands=gs.R_HANDS, antipodal=0):
    """One build of cloud `c` on `ctx`: the descriptor and the counters against the model, the search against the oracle."""
    (d, got), = model.build([c.xyz])
    assert got == regime
    ctx.set_cloud(c.xyz, c.cam)
    assert ctx.grid_desc() == d.as_dict()
    assert ctx.grid_stats() == model.stats
    s = c.samples if samples is None else samples
    n = _search(ctx, c, s, r_hands)
    if antipodal:  # the all-points normals pass walks the whole cloud, extra points included, through the same grid
        _search(ctx, c, s[:antipodal], r_hands, antipodal=True)
    assert ctx.grid_desc() == d.as_dict() and ctx.grid_stats() == model.stats  # (a search builds nothing)
    return d, n


def test_a_second_scan_pass_single_cloud():
    """160 x 120 x 100 cells at the base cell: 469 scan tiles for the 256 work-groups, samples in tiles of both passes; cold,
    then kept (without padding: 164 x 124 x 104 cells would pass the cap, so the kept descriptor is the box itself)."""
    c = gs.case_a()
    ctx, m = _context(c.cam_origins), gs.GridModel()
    d, n = _build(ctx, m, c, "cold", antipodal=24)
    assert d.tiles == 469 and n > 10
    d, _ = _build(ctx, m, c, "kept")
    assert d.tiles == 469 and d.dim == gs.A_DIMS and d.cell == 0.02


def test_b_cap_edge():
    """2^21 cells exactly (fits at the base cell, kept without padding), then one cell more along x on the same context: a
    miss through the high x face, refit at 0.04 m; and that cloud cold on a fresh context."""
    fit, over = gs.case_b("fit"), gs.case_b("over")
    ctx, m = _context(fit.cam_origins), gs.GridModel()
    d, n = _build(ctx, m, fit, "cold")
    assert d.ncell == gs.CELL_CAP and d.cell == 0.02 and n > 10
    d2, _ = _build(ctx, m, fit, "kept")
    assert d2.as_dict() == d.as_dict()
    d3, _ = _build(ctx, m, over, "miss")
    assert d3.open == 2 and m.stats == {"builds": 3, "cold": 1, "misses": 1}
    d4, _ = _build(ctx, m, over, "kept")
    assert d4.cell == 0.04 and d4.dim == (69, 68, 68)
    dc, _ = _build(_context(over.cam_origins), gs.GridModel(), over, "cold")
    assert dc.cell == 0.04 and dc.dim == (65, 64, 64)


@pytest.mark.parametrize("which", ["0.04", "0.08", "1.28-one", "1.28-two"])
def test_c_doubled_cells(which):
    """Cold builds at 0.04, 0.08 and 1.28 m: every hand ball spans few cells with thousands of candidates per row (at 1.28 m
    the whole scene is one or two cells)."""
    c = gs.case_c(which)
    d, n = _build(_context(c.cam_origins), gs.GridModel(), c, "cold", antipodal=16)
    assert d.cell == float(which[:4]) and n > 10


def test_d_transitions_between_cell_sizes():
    """table (cold) -> room (a miss through all six faces; the next descriptor doubles) -> room (kept, 0.04 m) -> table
    (covered, but another cell size: refit) -> table (kept, 0.02 m).  The miss is searched on samples among the room's dense
    points beyond the open y and z faces as well."""
    table, room = gs.case_d()
    ctx, m = _context(table.cam_origins), gs.GridModel()
    _build(ctx, m, table, "cold")
    u = m.next[0]
    near = _near_open_faces(room.xyz, np.array(u.mn), np.array(u.mn) + np.array(u.dim) * u.cell, 12)
    both = np.union1d(room.samples, near).astype(np.int32)
    d, n = _build(ctx, m, room, "miss", samples=both)
    assert d.open == 63 and d.cell == 0.02 and n > 10
    d, _ = _build(ctx, m, room, "kept", samples=both)
    assert d.cell == 0.04
    d, _ = _build(ctx, m, table, "refit")
    assert d.cell == 0.04 and d.open == 0
    d, _ = _build(ctx, m, table, "kept")
    assert d.cell == 0.02 and m.stats == {"builds": 5, "cold": 1, "misses": 1}


def test_e_other_base_cell():
    """nn_radius_hands = 0.1: the base cell is 0.025 m and the room doubles once, to 0.05 m."""
    c = gs.case_e()
    d, n = _build(_context(c.cam_origins, gs.E_R_HANDS), gs.GridModel(gs.E_R_HANDS), c, "cold", r_hands=gs.E_R_HANDS)
    assert d.cell == 0.05 and d.dim == gs.C_DIMS and n > 10


@pytest.mark.parametrize("n", [2, 8])
def test_f_batches(n):
    """Batches with clouds of more than 64 and more than 256 scan tiles for the 64 work-groups per cloud (and, of eight, a
    doubled cell, a far outlier, `tiny`, a plain scene and an empty cloud): cold, kept, and kept with one large cloud
    translated (a miss in that cloud only).  Every cloud's slice of the list against the oracle on that cloud alone."""
    from oracle import oracle_py as O

    clouds = gs.case_f(n)
    ctx, m = _context(clouds[0].cam_origins), gs.GridModel()

    def build(xyzs):
        descs = m.build(xyzs)
        off = ctx.set_cloud_batch(xyzs, [c.cam for c in clouds])
        for k, (d, _) in enumerate(descs):
            assert ctx.grid_desc(k) == d.as_dict(), k
        assert ctx.grid_stats() == m.stats
        return descs, off

    def search(xyzs, off, take=None, antipodal=False):
        samples = np.concatenate([c.samples[:take] + off[k] for k, c in enumerate(clouds)]).astype(np.int32)
        hyps = ctx.find_hands(samples, calculates_antipodal=antipodal)
        pos = base = 0
        for k, c in enumerate(clouds):
            s = c.samples[:take]
            if s.size:
                ref = O.find_hands(_params(c.cam_origins), xyzs[k], c.cam, s, calculates_antipodal=antipodal)["hyps"]
                part = hyps[pos:pos + len(ref)].copy()
                part["sample"] -= base
                _assert_hyps_equal(part, ref)
                pos += len(ref)
            base += s.size
        assert pos == len(hyps)
        return len(hyps)

    xyzs = [c.xyz for c in clouds]
    first, off = build(xyzs)
    assert max(d.tiles for d, _ in first) > gs.SCAN_GROUPS_SINGLE and search(xyzs, off) > 10
    _, off = build(xyzs)
    assert search(xyzs, off) > 10
    search(xyzs, off, take=10, antipodal=True)  # (the all-points pass walks every cloud of the batch through its own grid)
    k = gs.F_MOVED[n]
    xyzs[k] = xyzs[k] + gs.F_MOVE
    third, off = build(xyzs)
    assert [j for j, (d, _) in enumerate(third) if d.open] == [k] and m.stats == {"builds": 3, "cold": 1, "misses": 1}
    assert search(xyzs, off) > 10


def _replay(ctx, model, clouds):
    """A chain builds its capture's grid once, or twice when the call repeats itself once (a voxel bitmap or a capacity class
    that had to grow): the model replays as many builds of `clouds` as the context counts, and must end on the context's
    descriptors and counters."""
    todo = ctx.grid_stats()["builds"] - model.stats["builds"]
    assert 1 <= todo <= 2, todo
    for _ in range(todo):
        descs = model.build(clouds)
    for k, (d, _) in enumerate(descs):
        assert ctx.grid_desc(k) == d.as_dict(), k
    assert ctx.grid_stats() == model.stats


@pytest.mark.parametrize("classify", [False, True])
def test_g_fused_chains(svm_model, classify):
    """agh_localize and agh_localize_batch on three raw captures in a +-3 m workspace (voxelised boxes at 0.08 m, at the base
    cell with a second scan pass, at 0.04 m) against the stage-wise calls on the samples each chain reports."""
    from agile_grasp_amd import binding
    from tests.test_gpu_localize_batch import HYP_NAMES

    caps = gs.case_g()
    cams = caps[0].cam_origins
    one, batch, stage = (binding.Context(cams) for _ in range(3))
    for c in (one, batch, stage):
        c.load_svm(*svm_model)
    kw = dict(classify=classify, min_inliers=2)
    got_b = batch.localize_batch([c.xyz for c in caps], [c.size_left for c in caps], [c.workspace for c in caps],
                                 n_samples=[150, 150, 150], sample_seeds=[3, 4, 5], **kw)
    m_one, m_stage, voxs = gs.GridModel(), gs.GridModel(), []
    for k, rc in enumerate(caps):
        got = one.localize(rc.xyz, rc.size_left, rc.workspace, n_samples=150, sample_seed=3 + k, **kw)
        assert stage.preprocess(rc.xyz, rc.size_left, rc.workspace) == got["n_voxels"] == got_b[k]["n_voxels"]
        vox, _ = stage.cloud()
        voxs.append(vox.copy())
        d = gs.desc_finish(gs.extrema(vox), gs.BASE_CELL)
        assert d.cell == gs.G_CELLS[k] and d.tiles > gs.SCAN_GROUPS_BATCH
        _replay(one, m_one, [vox])
        _replay(stage, m_stage, [vox])
        hyps = stage.find_hands(got["samples"])
        h = hyps
        if classify:
            h = hyps[stage.classify().astype(bool)].copy()
            h["svm_keep"] = 1
        hd, idx = stage.find_handles(h, 2, 0.005)
        for res, what in ((got, "agh_localize"), (got_b[k], "agh_localize_batch")):
            assert np.array_equal(res["samples"], got["samples"]), what
            assert res["n_hypotheses"] == len(hyps) > 10 and len(res["hands"]) == len(h), what
            for f in HYP_NAMES:
                if classify or f != "svm_keep":
                    assert np.array_equal(res["hands"][f], h[f]), (what, k, f)
            assert len(res["handles"]) == len(hd) and np.array_equal(res["inlier_idx"], idx), what
            for f in hd.dtype.names:
                assert np.array_equal(res["handles"][f], hd[f]), (what, k, f)
    assert max(gs.desc_finish(gs.extrema(v), gs.BASE_CELL).tiles for v in voxs) > gs.SCAN_GROUPS_SINGLE
    _replay(batch, gs.GridModel(), voxs)


@pytest.mark.parametrize("which", ["1e6", "1e30", "mixed"])
def test_h_extreme_but_finite_extents(tiny_scene, which):
    """One point 1e6 m out; two points at +-1e30 m; the latter with 1 % non-finite rows: no error, the oracle's hypotheses, and
    a context that still works on `tiny` afterwards (a kept build whose descriptor has cells of 2e28 m, then a refit).

    Why this is safe for any finite float32 cloud.  desc_finish keeps the cell counts in double until their product fits
    kCellCap: floor(extent / cell) + 1 is at most 2^129 / 0.02 < 2^135, every doubling of the cell halves the quotient, so
    the loop ends after at most 135 doublings with each count in [1, 2^21] and only then converts to int (before this was
    written down, the count was converted first: 1e32 does not fit an int, the wrapped negative count made the product
    negative and ended the loop with dims of INT_MIN).  cell_coord clamps floor((v - mn) / cell) to [0, dim - 1] in double
    before it converts, so a point 1e30 m outside a KEPT 0.02 m descriptor (5e31 cells away) lands in a border cell, and a NaN
    in cell 0; (cz * dim_y + cy) * dim_x + cx is then below dim_x dim_y dim_z <= 2^21, inside the table.  desc_next compares
    the same quotients in double.  The float32 distance test of the searches sees (1e30)^2 = +Inf, which is not < r^2."""
    c = gs.case_h(which)
    ctx, m = _context(c.cam_origins), gs.GridModel()
    d, n = _build(ctx, m, c, "cold")
    assert max(d.dim) <= 128 and n > 10
    _build(ctx, m, c, "kept")
    plain = gs.plain(tiny_scene, tiny_scene.samples)
    _build(ctx, m, plain, "refit")
    d, n = _build(ctx, m, plain, "kept")
    assert d.cell == 0.02 and n > 10
    # ... and the far points on a kept descriptor of 0.02 m cells: a miss, clamped into border cells
    d, _ = _build(ctx, m, c, "miss")
    assert d.cell == 0.02 and d.open != 0
