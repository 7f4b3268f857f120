"""agh_localize_batch_begin / _stage / _end (include/agh.h): the batch chain as two calls, with the next batch's captures staged
on a second stream meanwhile.  Every comparison is exact equality against the blocking agh_localize_batch on the same inputs, on
a second context: handles, inlier lists, hands (every field but the epoch), samples, results[k] and the bound batch."""
import ctypes as C

import numpy as np
import pytest

from agile_grasp_amd import synthetic
from tests.test_gpu_boundary_chain import _contexts, _crop, _scene
from tests.test_gpu_localize_batch import _same

pytestmark = pytest.mark.gpu

KW = dict(classify=True, min_inliers=2)


def _wide(xyz):
    """the capture with 32-byte rows"""
    out = np.zeros((xyz.shape[0], 8), np.float32)
    out[:, :3] = xyz
    return out


def _pinned(a):
    import torch

    return torch.from_numpy(np.array(a, np.float32)).pin_memory().numpy()


@pytest.fixture(scope="module")
def caps():
    """eight small raw captures (drop-outs in all but one), read-only"""
    out = [synthetic.make_raw_cloud(40_000 + 5_000 * k, 300 + k, nan_frac=0.0 if k == 1 else 0.01) for k in range(8)]
    for c in out:
        c.xyz.setflags(write=False)
    return out


def _batches(caps):
    """Three batches of 3, 1 and 4 captures: strides 12 and 32, a capture with NaNs (all but caps[1]), an empty capture, explicit
    and drawn sample lists.  Each: (captures, sizes_left, workspaces, keyword arguments)."""
    rng = np.random.default_rng(4)
    expl = lambda n: np.sort(rng.permutation(3000)[:n]).astype(np.int32)  # (every capture voxelises to more than 3000 points)
    empty = np.zeros((0, 3), np.float32)
    b0 = ([caps[0].xyz, _wide(caps[1].xyz), caps[2].xyz], [c.size_left for c in caps[:3]], [c.workspace for c in caps[:3]],
          dict(samples=[None, expl(48), None], n_samples=[64, 0, 32], sample_seeds=[5, 6, 7], dense=[False, True, False]))
    b1 = ([_wide(caps[3].xyz)], [caps[3].size_left], [caps[3].workspace], dict(n_samples=[64], sample_seeds=[8]))
    b2 = ([caps[4].xyz, empty, _wide(caps[5].xyz), caps[6].xyz], [caps[4].size_left, 0, caps[5].size_left, caps[6].size_left],
          [caps[4].workspace, caps[4].workspace, caps[5].workspace, caps[6].workspace],
          dict(samples=[expl(40), None, None, expl(33)], n_samples=[0, 16, 64, 0], sample_seeds=[1, 2, 3, 4]))
    return [b0, b1, b2]


def _blocking(ref, batch, **kw):
    xyz, sl, ws, bkw = batch
    got = ref.localize_batch(xyz, sl, ws, **bkw, **KW, **kw)
    return got, ref.last_batch_counts, ref.cloud()


def _equal(got, ctx, want, what=""):
    res, counts, cloud = want
    assert len(got) == len(res), what
    for k in range(len(res)):
        _same(got[k], res[k], f"{what} capture {k}")
    assert ctx.last_batch_counts == counts, what
    xyz, cam = ctx.cloud()
    assert np.array_equal(xyz, cloud[0]) and np.array_equal(cam, cloud[1]), what


@pytest.mark.parametrize("pinned", [False, True])
def test_streamed_equals_blocking(svm_model, caps, pinned):
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    batches = _batches(caps)
    want = [_blocking(ref, b) for b in batches]
    assert all(sum(r["n_hypotheses"] for r in w[0]) > 0 for w in want)
    assert sum(len(r["handles"]) for w in want for r in w[0]) > 0
    assert want[2][0][1]["n_voxels"] == 0  # (the empty capture)
    src = [[_pinned(x) if pinned else np.array(x) for x in b[0]] for b in batches]
    one.localize_batch_begin(src[0], batches[0][1], batches[0][2], **batches[0][3], **KW)
    staged = one.localize_batch_stage(src[1])
    _equal(one.localize_batch_end(), one, want[0], "batch 0")
    one.localize_batch_begin(staged, batches[1][1], batches[1][2], **batches[1][3], **KW)
    staged = one.localize_batch_stage(src[2])
    _equal(one.localize_batch_end(), one, want[1], "batch 1")
    one.localize_batch_begin(staged, batches[2][1], batches[2][2], **batches[2][3], **KW)
    _equal(one.localize_batch_end(), one, want[2], "batch 2")


def test_a_staged_set_that_is_not_adopted(svm_model, caps):
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    b0, b1, _ = _batches(caps)
    want0, want1 = _blocking(ref, b0), _blocking(ref, b1)
    # one pointer changed: the copy of a staged capture is another capture to the library
    staged = one.localize_batch_stage([np.array(x) for x in b0[0]])
    other = list(staged)
    other[2] = np.array(b0[0][2])
    one.localize_batch_begin(other, b0[1], b0[2], **b0[3], **KW)
    _equal(one.localize_batch_end(), one, want0, "pointer changed")
    # one count changed: a staged capture one point longer than the one begun
    longer = np.concatenate([b1[0][0], b1[0][0][:1]])
    one.localize_batch_stage([longer])
    one.localize_batch_begin([longer[:-1]], b1[1], b1[2], **b1[3], **KW)
    _equal(one.localize_batch_end(), one, want1, "count changed")
    # a single staged capture, then a batch begun from the same array; a staged batch, then a single capture begun from it
    x = np.array(b1[0][0])
    one.localize_stage(x)
    one.localize_batch_begin([x], b1[1], b1[2], **b1[3], **KW)
    _equal(one.localize_batch_end(), one, want1, "agh_localize_stage, then agh_localize_batch_begin")
    skw = dict(n_samples=64, sample_seed=8, **KW)
    single = ref.localize(x, b1[1][0], b1[2][0], **skw)
    (st,) = one.localize_batch_stage([x])
    one.localize_begin(st, b1[1][0], b1[2][0], **skw)
    _same(one.localize_end(), single, "agh_localize_batch_stage, then agh_localize_begin")
    assert len(single["hands"]) > 0 or single["n_hypotheses"] > 0


def test_sources_and_argument_arrays_may_go_when_the_calls_return(svm_model, caps):
    """Pageable staged captures are read when agh_localize_batch_stage returns; the pointer, stride and count arrays, the lp
    records and the explicit sample lists are copied by agh_localize_batch_begin."""
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    b0, _, b2 = _batches(caps)
    want0, want2 = _blocking(ref, b0), _blocking(ref, b2)

    def scribble():
        a = one._batch_pending
        for s in a["sample_arrays"]:
            s[:] = 2 ** 30
        n_arr = len(a["ptrs"])
        C.memset(a["lps"], 0xFF, C.sizeof(a["lps"]))
        C.memset(a["ptrs"], 0xFF, 8 * n_arr)
        C.memset(a["strides"], 0xFF, 8 * n_arr)
        C.memset(a["ns"], 0xFF, 8 * n_arr)

    kw0 = dict(b0[3], samples=[None if s is None else s.copy() for s in b0[3]["samples"]])
    kw2 = dict(b2[3], samples=[None if s is None else s.copy() for s in b2[3]["samples"]])
    one.localize_batch_begin([np.array(x) for x in b0[0]], b0[1], b0[2], **kw0, **KW)
    scribble()
    staged = one.localize_batch_stage([np.array(x) for x in b2[0]])
    addr = [(s.ctypes.data, s.shape) for s in staged]
    for s in staged:
        s[:] = 1.0e30  # the captures are on the device
    _equal(one.localize_batch_end(), one, want0, "batch 0")
    one.localize_batch_begin(staged, b2[1], b2[2], **kw2, **KW)  # (adopted by pointer, stride and count: the content is not read)
    assert [(s.ctypes.data, s.shape) for s in one._batch_pending["keep"]] == addr
    scribble()
    _equal(one.localize_batch_end(), one, want2, "batch 2")


def _outgrowing(cams):
    """(small crops whose lattices size a context's bitmap slots, the whole scenes whose lattices outgrow them)"""
    xyz, size_left, ws, _ = _scene()
    fin = xyz[np.isfinite(xyz).all(1)]
    lo, hi = np.percentile(fin, 30, axis=0), np.percentile(fin, 70, axis=0)
    lo[0], hi[0] = 0.7, 0.85
    small, small_sl = _crop(xyz, size_left, lo, hi)
    other = synthetic.make_raw_cloud(60_000, 41)
    kw = dict(n_samples=[64, 48], sample_seeds=[3, 4])
    first = ([small, small[: len(small) // 2]], [small_sl, min(small_sl, len(small) // 2)], [ws, ws], kw)
    second = ([xyz, other.xyz], [size_left, other.size_left], [ws, other.workspace], kw)
    return first, second


def test_the_outgrown_bitmap_repeat_reads_its_own_raw_buffer(svm_model, caps):
    _, _, _, cams = _scene()
    one, ref = _contexts(cams, svm_model)
    first, second = _outgrowing(cams)
    third = _batches(caps)[1]
    want1 = _blocking(ref, first)
    builds = ref.grid_stats()["builds"]
    want2 = _blocking(ref, second)
    assert ref.grid_stats()["builds"] - builds == 2  # (the blocking call ran the batch twice: the lattices outgrew the slots)
    want3 = _blocking(ref, third)
    one.localize_batch_begin(first[0], first[1], first[2], **first[3], **KW)
    _equal(one.localize_batch_end(), one, want1, "first")
    builds = one.grid_stats()["builds"]
    one.localize_batch_begin(second[0], second[1], second[2], **second[3], **KW)
    staged = one.localize_batch_stage([np.array(x) for x in third[0]])
    _equal(one.localize_batch_end(), one, want2, "second")
    assert one.grid_stats()["builds"] - builds == 2
    one.localize_batch_begin(staged, third[1], third[2], **third[3], **KW)
    _equal(one.localize_batch_end(), one, want3, "third")


def test_the_capacity_class_repeat_on_a_fresh_context(svm_model, caps):
    """With 1 mm voxels nearly every raw point of a capture is kept: the Taubin balls of the second capture hold more than the
    first capacity class's 1152 points, so the search's AGH_ERR_RETRY is repeated inside agh_localize_batch_end."""
    dense = synthetic.make_raw_cloud(60_000, 77, n_objects=2)
    batch = ([caps[0].xyz, dense.xyz], [caps[0].size_left, dense.size_left], [caps[0].workspace, dense.workspace],
             dict(n_samples=[32, 64], sample_seeds=[1, 2], cell_size=0.001))
    third = _batches(caps)[1]
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    want = _blocking(ref, batch)
    nt, _ = ref.neighbor_counts()
    assert int((nt > 1152).sum()) > 0
    want3 = _blocking(ref, third)
    one.localize_batch_begin(batch[0], batch[1], batch[2], **batch[3], **KW)
    staged = one.localize_batch_stage([np.array(x) for x in third[0]])
    _equal(one.localize_batch_end(), one, want, "dense")
    one.localize_batch_begin(staged, third[1], third[2], **third[3], **KW)
    _equal(one.localize_batch_end(), one, want3, "third")


def test_state_table(svm_model, caps, tiny_scene):
    from agile_grasp_amd import binding

    one, ref = _contexts(caps[0].cam_origins, svm_model)
    b0, b1, _ = _batches(caps)
    want0 = _blocking(ref, b0)
    with pytest.raises(binding.AghError) as e:
        one.localize_batch_end()  # no begin
    assert e.value.code == binding.AGH_ERR_STATE
    sc = tiny_scene
    one.set_cloud(sc.xyz, sc.cam)
    hyps = one.find_hands(sc.samples[:40])
    refused = {
        "agh_localize_batch_begin": lambda: one.localize_batch_begin(b1[0], b1[1], b1[2], **b1[3], **KW),
        "agh_localize_begin": lambda: one.localize_begin(b1[0][0], b1[1][0], b1[2][0], n_samples=8),
        "agh_localize_batch": lambda: one.localize_batch(b1[0], b1[1], b1[2], **b1[3], **KW),
        "agh_localize_end": lambda: one.localize_end(),
        "agh_set_cloud": lambda: one.set_cloud(sc.xyz, sc.cam),
        "agh_find_hands": lambda: one.find_hands(sc.samples[:40]),
        "agh_classify": lambda: one.classify(),
        "agh_get_cloud": lambda: one.cloud(),
        "agh_set_cloud_cam_origins": lambda: one.set_cloud_cam_origins(np.zeros((3, 2, 3))),
        "agh_remove_plane": lambda: one.remove_plane(),
    }
    assert len(hyps) > 0
    for name in sorted(refused):
        one.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], **KW)
        pending = one._batch_pending
        with pytest.raises(binding.AghError) as e:
            refused[name]()
        assert e.value.code == binding.AGH_ERR_STATE, name
        one._batch_pending = pending  # (a refused localize_batch_begin of the binding does not replace it; kept explicit)
        assert one.get_cloud_cam_origins() is None
        one.synchronize()
        assert isinstance(one.lib.agh_last_error(one._h), bytes)
        _equal(one.localize_batch_end(), one, want0, name)
    # AGH_ERR_CAPACITY from the collecting call: results filled, the chain over, a new begin accepted
    n_handles = sum(len(r["handles"]) for r in want0[0])
    n_hands = sum(len(r["hands"]) for r in want0[0])
    n_idx = sum(len(r["inlier_idx"]) for r in want0[0])
    assert n_hands > 0
    # (output buffers one record too small: the handles' if the batch has handles, else the hands')
    small = (n_handles - 1, n_idx, n_hands) if n_handles > 0 else (n_handles, n_idx, n_hands - 1)
    one.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], **KW)
    with pytest.raises(binding.AghError) as e:
        one.localize_batch_end(caps=small)
    assert e.value.code == binding.AGH_ERR_CAPACITY
    assert one.last_batch_counts == want0[1]
    one.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], **KW)
    _equal(one.localize_batch_end(), one, want0, "after AGH_ERR_CAPACITY")


def test_per_capture_camera_origins(svm_model, caps):
    from agile_grasp_amd import binding

    one, ref = _contexts(caps[0].cam_origins, svm_model)
    b0, _, _ = _batches(caps)
    tab = np.stack([np.asarray(caps[0].cam_origins, np.float64) + 0.05 * k for k in range(3)])
    ref.set_cloud_cam_origins(tab)
    one.set_cloud_cam_origins(tab)
    want = _blocking(ref, b0)
    one.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], **KW)
    assert np.array_equal(one.get_cloud_cam_origins(), tab)
    _equal(one.localize_batch_end(), one, want, "per-capture origins")
    one.set_cloud_cam_origins(tab[:2])  # two rows, three captures
    with pytest.raises(binding.AghError) as e:
        one.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], **KW)
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT
    with pytest.raises(binding.AghError) as e:
        one.localize_batch_end()  # no chain in flight
    assert e.value.code == binding.AGH_ERR_STATE
    one.set_cloud_cam_origins(tab)
    _equal(one.localize_batch(b0[0], b0[1], b0[2], **b0[3], **KW), one, want, "blocking, afterwards")


def test_argument_errors(svm_model, caps):
    from agile_grasp_amd import binding

    b0, _, _ = _batches(caps)
    plain = binding.Context(caps[0].cam_origins)
    with pytest.raises(binding.AghError) as e:
        plain.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], classify=True)
    assert e.value.code == binding.AGH_ERR_NO_SVM
    plain.close()
    one, ref = _contexts(caps[0].cam_origins, svm_model)
    bad = dict(b0[3], samples=[None, np.array([0, 10 ** 8], np.int32), None])
    one.localize_batch_begin(b0[0], b0[1], b0[2], **bad, **KW)
    with pytest.raises(binding.AghError) as e:
        one.localize_batch_end()
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "capture 1" in str(e.value)
    one.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], **KW)
    _equal(one.localize_batch_end(), one, _blocking(ref, b0), "after the error")


def test_bad_arguments_of_begin_and_stage(svm_model, caps):
    """AGH_ERR_INVALID_ARGUMENT with the texts of include/agh.h, nothing queued or staged, the context usable afterwards."""
    from agile_grasp_amd import binding

    one, ref = _contexts(caps[0].cam_origins, svm_model)
    b0, _, _ = _batches(caps)
    xyz = [np.array(caps[0].xyz), np.array(caps[2].xyz)]

    def arrays(strides=(12, 12), null=None, counts=None):
        ptrs = (C.c_void_p * 2)(*[None if k == null else x.ctypes.data for k, x in enumerate(xyz)])
        ns = (C.c_int64 * 2)(*(counts or [x.shape[0] for x in xyz]))
        lps = (binding.AghLocalizeParams * 2)()
        for k in range(2):
            lps[k].size_left, lps[k].classify, lps[k].cell_size, lps[k].min_inliers = caps[2 * k].size_left, 0, 0.003, 2
            lps[k].min_length, lps[k].n_samples = 0.005, 8
            for q in range(6):
                lps[k].workspace[q] = caps[2 * k].workspace[q]
        return ptrs, (C.c_int64 * 2)(*strides), ns, lps

    def begin(nc=2, lp=True, **kw):
        ptrs, strides, ns, lps = arrays(**kw)
        rc = one.lib.agh_localize_batch_begin(one._h, ptrs, strides, ns, lps if lp else None, C.c_int32(nc))
        return rc, one.lib.agh_last_error(one._h).decode()

    def stage(nc=2, **kw):
        ptrs, strides, ns, _ = arrays(**kw)
        rc = one.lib.agh_localize_batch_stage(one._h, ptrs, strides, ns, C.c_int32(nc))
        return rc, one.lib.agh_last_error(one._h).decode()

    bad = binding.AGH_ERR_INVALID_ARGUMENT
    for fn, name in ((begin, "agh_localize_batch"), (stage, "agh_localize_batch_stage")):
        for nc in (0, 65):
            rc, text = fn(nc=nc)
            assert rc == bad and text.startswith(name + ": bad arguments (1 <= n_captures <= 64"), (name, nc, text)
        rc, text = fn(strides=(12, 10))
        assert rc == bad and text.startswith(name + ": bad arguments for capture 1"), (name, text)
        rc, text = fn(null=0)
        assert rc == bad and text.startswith(name + ": bad arguments for capture 0"), (name, text)
        rc, text = fn(counts=[xyz[0].shape[0], -1])
        assert rc == bad and text.startswith(name + ": bad arguments for capture 1"), (name, text)
    rc, text = begin(lp=False)
    assert rc == bad and text.startswith("agh_localize_batch: bad arguments (1 <= n_captures <= 64"), text
    with pytest.raises(binding.AghError) as e:
        one.localize_batch_end()  # nothing was queued
    assert e.value.code == binding.AGH_ERR_STATE
    one.localize_batch_begin(b0[0], b0[1], b0[2], **b0[3], **KW)  # ... and nothing staged: this one uploads
    _equal(one.localize_batch_end(), one, _blocking(ref, b0), "after the refusals")


_BYSTANDER_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from agile_grasp_amd import binding, synthetic
from tests.test_gpu_localize_batch import _same
from tests.test_gpu_sharding import FIELDS, _group, _run_ranks, _run_ranks_codes

sc = synthetic.config("tiny")
z = np.load(os.path.join("tests", "golden", "svm_weights.npz"))
svm = (z["w"], float(z["rho"]))
raws = [synthetic.make_raw_cloud(40_000, 300 + k) for k in range(2)]
args = ([r.xyz for r in raws], [r.size_left for r in raws], [r.workspace for r in raws])
kw = dict(n_samples=[48, 32], sample_seeds=[1, 2], classify=True, min_inliers=2)
solo = binding.Context(sc.cam_origins)
solo.load_svm(*svm)
want = solo.localize_batch(*args, **kw)
want_counts = solo.last_batch_counts
solo.set_cloud(sc.xyz, sc.cam)
ref = solo.find_hands(sc.samples)
ctxs = _group(sc, 2)
for c in ctxs:
    c.load_svm(*svm)
out = {}
ctxs[1].localize_batch_begin(*args, **kw)
res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
out["codes"] = [code for _, code in res]
out["lists"] = [v is not None for v, _ in res]
got = ctxs[1].localize_batch_end()
for k in range(2):
    _same(got[k], want[k], "capture %d" % k)
out["chain_exact"] = ctxs[1].last_batch_counts == want_counts
out["hypotheses"] = sum(g["n_hypotheses"] for g in got)
ctxs[1].set_cloud(sc.xyz, sc.cam)
follow = _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
out["follow_same"] = [bool(len(h) == len(ref) and all(np.array_equal(h[f], ref[f]) for f in FIELDS)) for h in follow]
print(json.dumps(out))
"""


def test_a_rank_with_a_batch_chain_in_flight_is_a_bystander():
    """One in-process rank of two has a batch chain in flight: the sharded search returns an error on both ranks, the chain's
    results are the blocking call's, and the communicator works afterwards."""
    import json
    import os
    import subprocess
    import sys

    from agile_grasp_amd import binding

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AGH_LOCAL_BARRIER_TIMEOUT_S="60")
    p = subprocess.run([sys.executable, "-c", _BYSTANDER_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["codes"] == [binding.AGH_ERR_STATE] * 2 and not any(out["lists"]), out
    assert out["chain_exact"] and out["hypotheses"] > 0, out
    assert out["follow_same"] == [True, True], out
