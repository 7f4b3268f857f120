"""The cluster stage where the search grid changes shape (tests/cluster_grid_cases.py): a reach of three cells, owner runs and
candidate totals of several tiles, a component of 22 500 voxels, more than 1024 qualifying roots, doubled cells, and a sequence of
builds on one context with a miss through all six faces.  Labels, counts, ids and samples are held against the numpy model with
exact equality, and agh_get_grid_desc / agh_get_grid_stats against the grid model after every call -- so each test proves on
the device that it reached the regime tests/test_cluster_grid_cases.py proves from the models."""
import numpy as np
import pytest

from tests import cluster_cases as CC
from tests import cluster_grid_cases as G
from tests import grid_scale_clouds as gs
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

CASES = G.cases()
SKIP = -(1 << 31)


def _cp(fields):
    from agile_grasp_amd import binding

    return binding.cluster_params(**fields)


def _check_model(ctx, got, m, cp, S, seed, vox=None):
    """labels, info and samples of the last clustered call against the model `m` of the context's cloud"""
    from agile_grasp_amd.binding import labeled_samples

    if vox is not None:
        xyz, cams = ctx.cloud()
        assert np.array_equal(xyz, vox[0]) and np.array_equal(cams, vox[1])
    info = ctx.cluster_info()
    labels = ctx.cluster_labels()
    print("voxels", len(labels), "foreground", info["n_foreground"], "components", info["n_components"], "objects", info["n_objects"],
          "M", list(info["n_voxels"][:8]), "grid", ctx.grid_desc(), ctx.grid_stats())
    assert len(labels) == len(m["labels"]) and np.array_equal(labels, m["labels"])
    assert (info["n_foreground"], info["n_components"], info["n_objects"]) == (m["n_foreground"], m["n_components"], m["n_objects"])
    assert np.array_equal(info["n_voxels"], m["sizes"]) and np.array_equal(info["ids"], m["ids"])
    assert len(got) == cp["max_objects"] and all(g["n_voxels"] == len(labels) for g in got)
    want = labeled_samples(m["lists"], S, seed)
    assert np.array_equal(np.concatenate([g["samples"] for g in got]) if S else np.zeros(0, np.int32), want)
    for j in range(cp["max_objects"]):
        if m["sizes"][j] == 0 and S:
            assert (got[j]["samples"] == SKIP).all() and got[j]["n_hypotheses"] == 0 and len(got[j]["hands"]) == 0


def _call(ctx, c, S, seed=11):
    return ctx.localize_clustered(c["points"], c["size_left"], c["workspace"], _cp(c["cp"]), n_samples=S, sample_seed=seed,
                                  classify=False, dense=c["dense"], cell_size=c["cell"])


def _check_grid(ctx, d, stats):
    assert ctx.grid_desc() == d.as_dict()
    assert ctx.grid_stats() == stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_model(name):
    """every case cold on a fresh context, then once more with n_samples = 0 on the descriptor the first build kept"""
    from agile_grasp_amd import binding

    mo = G.model(name)
    c, m = mo["case"], mo["m"]
    ctx, g = binding.Context(np.zeros((2, 3))), gs.GridModel()
    S = 3 if name.startswith("doubled") else 5
    got = _call(ctx, c, S)
    (d, regime), = g.build([mo["xyz"]])
    _check_model(ctx, got, m, c["cp"], S, 11, (mo["xyz"], mo["cams"]))
    assert regime == "cold"
    _check_grid(ctx, d, g.stats)
    got = _call(ctx, c, 0)
    (d, regime), = g.build([mo["xyz"]])
    _check_model(ctx, got, m, c["cp"], 0, 11)
    assert regime == "kept" and g.stats == {"builds": 2, "cold": 1, "misses": 0}
    _check_grid(ctx, d, g.stats)
    ctx.close()


def test_sequence_on_one_context():
    """cold, a miss through all six faces, kept, the doubled room (a miss, then kept at 0.04 m), the small cloud again (a refit at
    0.04 m, then kept at 0.02 m): every call against the model, every build against the grid model -- seven calls, seven builds"""
    from agile_grasp_amd import binding

    ctx = binding.Context(np.zeros((2, 3)))
    descs = G.sequence_descs()
    for k, ((name, c, want), (d, regime, stats)) in enumerate(zip(G.sequence(), descs)):
        mo = G.model(name)
        S = 0 if name == "out_kept" else 4
        got = _call(ctx, c, S, seed=20 + k)
        print(name, regime)
        assert regime == want
        _check_model(ctx, got, mo["m"], c["cp"], S, 20 + k, (mo["xyz"], mo["cams"]))
        _check_grid(ctx, d, stats)
    assert ctx.grid_stats() == {"builds": 7, "cold": 1, "misses": 2}
    ctx.close()


def _depth_call(ctx, images, cp, cell, S, seed):
    return ctx.localize_depth_clustered(images, G.M.WIDE, _cp(cp), n_samples=S, sample_seed=seed, classify=False, cell_size=cell)


def _depth_equals_points(one, ref, g, step, seed):
    """one depth call on `one` against the model of its own cloud, against the grid model `g`, and against the points form of
    the deprojected capture on `ref`; returns the build's descriptor and regime"""
    images, cp, cell = G.depth_steps()[step]
    got = _depth_call(one, images, cp, cell, 6, seed)
    xyz, cams = one.cloud()
    vox = G.depth_cloud(images, cell)
    assert np.array_equal(xyz, vox[0]) and np.array_equal(cams, vox[1])
    (d, regime), = g.build([xyz])
    _check_model(one, got, CC.cluster_model(xyz, cp), cp, 6, seed)
    _check_grid(one, d, g.stats)
    pts = ref.deproject(images)
    want = ref.localize_clustered(pts, images[0]["data"].size, G.M.WIDE, _cp(cp), n_samples=6, sample_seed=seed, classify=False,
                                  dense=True, cell_size=cell)
    assert np.array_equal(one.cluster_labels(), ref.cluster_labels())
    _check_grid(ref, d, g.stats)
    for j, (a, b) in enumerate(zip(got, want)):
        _same(a, b, (step, j))
    return d, regime


def _depth_contexts():
    from agile_grasp_amd import binding

    origins = np.stack([im["pose"][:, 3] for im in G.depth_steps()["small"][0]])
    return binding.Context(origins), binding.Context(origins)


def test_depth_form_equals_points_form_on_a_miss():
    one, ref = _depth_contexts()
    g = gs.GridModel()
    _, regime = _depth_equals_points(one, ref, g, "small", 3)
    assert regime == "cold"
    d, regime = _depth_equals_points(one, ref, g, "out", 4)
    assert regime == "miss" and d.open == 63 and g.stats == {"builds": 2, "cold": 1, "misses": 1}
    one.close()
    ref.close()


def test_depth_form_equals_points_form_with_doubled_cells():
    one, ref = _depth_contexts()
    d, regime = _depth_equals_points(one, ref, gs.GridModel(), "doubled", 5)
    assert regime == "cold" and d.cell == 0.04
    one.close()
    ref.close()
