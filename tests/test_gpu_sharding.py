"""The sample-sharded search (csrc/shard.hip) on the GPU.  A single-GPU box cannot host two RCCL ranks, so the G-rank
schedule runs on G contexts of one process, one host thread each, whose communicator exchanges through device copies
(agh_comm_init_local): kernels, offsets and buffers are exactly those of the RCCL path, only the transport differs.
RCCL itself (dlopen, ncclCommInitRank, ncclAllGather on the search's stream) is exercised as a one-rank communicator."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("sample", "orientation", "cam_source", "n_in_box", "half_antipodal", "full_antipodal", "finger_index", "depth_index",
          "axis", "approach", "binormal", "bottom", "surface", "width", "valid")


def _run_ranks(ctxs, fn):
    """fn(rank, ctx) on one thread per rank (the collectives block until every rank arrives)."""
    out, err = [None] * len(ctxs), [None] * len(ctxs)

    def work(r):
        try:
            out[r] = fn(r, ctxs[r])
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(len(ctxs))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in th), "a rank hangs in a collective"
    for e in err:
        if e is not None:
            raise e
    return out


def _group(sc, G, **kw):
    from agile_grasp_amd import binding

    ctxs = [binding.Context(sc.cam_origins, **kw) for _ in range(G)]
    for c in ctxs:
        c.set_cloud(sc.xyz, sc.cam)  # every rank holds the same cloud
    binding.comm_init_local(ctxs)
    return ctxs


def _same(a, b):
    assert len(a) == len(b)
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("G", [2, 3, 8])
def test_sharded_search_equals_single_gpu(small_scene, svm_model, G):
    from agile_grasp_amd import binding

    sc = small_scene
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    one.load_svm(*svm_model)
    ref_keep = one.classify()
    ctxs = _group(sc, G)
    for c in ctxs:
        c.load_svm(*svm_model)
    res = _run_ranks(ctxs, lambda r, c: (c.find_hands_sharded(sc.samples), c.classify_sharded()))
    for r, (hyps, (recs, keep)) in enumerate(res):
        _same(hyps, ref)  # every rank holds the complete list
        assert len(set(hyps["epoch"].tolist())) == 1 and hyps["epoch"][0] != 0
        _same(recs, ref)
        assert np.array_equal(keep, ref_keep) and np.array_equal(recs["svm_keep"], ref_keep)
        assert ctxs[r].comm_rank() == (r, G)
    # a rank's own getters describe its slice
    lo, hi = binding.shard_slice(sc.samples.size, 1, G)
    assert len(ctxs[1].frames()) == hi - lo
    assert int(ref_keep.sum()) > 0 and len(ref) > 50


def test_cloud_per_rank_is_the_same_sharded_call():
    """BASELINE config C5 as `bench.py --gpus N` runs it: the sample list of a BATCH of clouds sharded in cloud order, i.e.
    rank r holds cloud r and its slice of the concatenated list is that cloud's own samples (the other slices are never
    read by it).  Every rank ends with the concatenation of the clouds' lists, sample positions counted through the batch."""
    from agile_grasp_amd import binding, synthetic

    G, S = 3, 120
    scenes = [synthetic.make_scene(30_000, S, seed=60 + r, two_view=True, n_objects=5, name=f"batch_{r}") for r in range(G)]
    refs = []
    for sc in scenes:
        one = binding.Context(sc.cam_origins)
        one.set_cloud(sc.xyz, sc.cam)
        refs.append(one.find_hands(sc.samples))
    assert all(len(r) > 10 for r in refs)
    ctxs = [binding.Context(sc.cam_origins) for sc in scenes]
    for c, sc in zip(ctxs, scenes):
        c.set_cloud(sc.xyz, sc.cam)
    binding.comm_init_local(ctxs)

    def search(r, c):
        idx = np.zeros(G * S, np.int32)
        idx[r * S:(r + 1) * S] = scenes[r].samples
        return c.find_hands_sharded(idx)

    for hyps in _run_ranks(ctxs, search):
        assert len(hyps) == sum(len(r) for r in refs)
        at = 0
        for r, ref in enumerate(refs):
            part = hyps[at:at + len(ref)]
            at += len(ref)
            assert np.array_equal(part["sample"], ref["sample"] + r * S)
            for f in FIELDS:
                if f != "sample":
                    assert np.array_equal(part[f], ref[f]), (r, f)


def test_cloud_per_rank_with_an_empty_cloud_on_one_rank():
    """A rank whose own cloud is empty still joins every collective of the call (it used to return early and leave the others
    waiting in the all-gather): it contributes an empty slice."""
    from agile_grasp_amd import binding, synthetic

    G, S = 3, 64
    scenes = [synthetic.make_scene(30_000, S, seed=80 + r, two_view=True, n_objects=5, name=f"e_{r}") for r in range(G)]
    refs = []
    for r, sc in enumerate(scenes):
        one = binding.Context(sc.cam_origins)
        one.set_cloud(sc.xyz, sc.cam)
        refs.append(one.find_hands(sc.samples) if r != 1 else one.find_hands(sc.samples)[:0])
    ctxs = [binding.Context(sc.cam_origins) for sc in scenes]
    for r, (c, sc) in enumerate(zip(ctxs, scenes)):
        if r == 1:
            c.set_cloud(np.zeros((0, 3), np.float32), np.zeros(0, np.int32))
        else:
            c.set_cloud(sc.xyz, sc.cam)
    binding.comm_init_local(ctxs)

    def search(r, c):
        idx = np.zeros(G * S, np.int32)
        if r != 1:
            idx[r * S:(r + 1) * S] = scenes[r].samples
        return c.find_hands_sharded(idx)

    for hyps in _run_ranks(ctxs, search):
        assert len(hyps) == sum(len(r) for r in refs) > 0
        at = 0
        for r, ref in enumerate(refs):
            part = hyps[at:at + len(ref)]
            at += len(ref)
            assert np.array_equal(part["sample"], ref["sample"] + r * S)
            for f in FIELDS:
                if f != "sample":
                    assert np.array_equal(part[f], ref[f]), (r, f)


def test_batch_per_rank_is_the_same_sharded_call():
    """BASELINE config C5 to the letter on fewer GPUs than clouds (`bench.py`'s key c5_batch_sharded): the cloud-major sample list
    of a batch of FOUR clouds sharded over TWO ranks -- rank r holds clouds 2r, 2r + 1 as one batch in its context
    (agh_set_cloud_batch) and its slice of the list is their samples, as positions in its own point array."""
    from agile_grasp_amd import binding, synthetic

    G, per, S = 2, 2, 120
    scenes = [synthetic.make_scene(30_000, S, seed=70 + k, two_view=True, n_objects=5, name=f"batch_{k}") for k in range(G * per)]
    refs = []
    for sc in scenes:
        one = binding.Context(sc.cam_origins)
        one.set_cloud(sc.xyz, sc.cam)
        refs.append(one.find_hands(sc.samples))
    assert all(len(r) > 10 for r in refs)
    ctxs = [binding.Context(scenes[0].cam_origins) for _ in range(G)]
    offs = []
    for r, c in enumerate(ctxs):
        mine = scenes[r * per:(r + 1) * per]
        c.set_cloud_batch([sc.xyz for sc in mine], [sc.cam for sc in mine])
        offs.append(np.concatenate([[0], np.cumsum([sc.n for sc in mine])]))
    binding.comm_init_local(ctxs)

    def search(r, c):
        idx = np.zeros(G * per * S, np.int32)
        mine = scenes[r * per:(r + 1) * per]
        idx[r * per * S:(r + 1) * per * S] = np.concatenate([sc.samples + offs[r][k] for k, sc in enumerate(mine)])
        return c.find_hands_sharded(idx)

    for hyps in _run_ranks(ctxs, search):
        assert len(hyps) == sum(len(r) for r in refs)
        at = 0
        for k, ref in enumerate(refs):
            part = hyps[at:at + len(ref)]
            at += len(ref)
            assert np.array_equal(part["sample"], ref["sample"] + k * S)
            for f in FIELDS:
                if f != "sample":
                    assert np.array_equal(part[f], ref[f]), (k, f)


def test_sharded_antipodal_pass(tiny_scene):
    """calculates_antipodal: the all-points normals pass sharded by point range, cloud_normals_ and the samples' own
    normals all-gathered before the hand search (hand_search.cpp:13-26, 102)."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples, calculates_antipodal=True)
    ref_normals = one.normals()
    assert ref["half_antipodal"].sum() > 0
    ctxs = _group(sc, 3)
    res = _run_ranks(ctxs, lambda r, c: (c.find_hands_sharded(sc.samples, calculates_antipodal=True), c.normals()))
    for hyps, normals in res:
        _same(hyps, ref)
        assert np.array_equal(normals, ref_normals)


def test_sharded_rand50_mode(small_scene):
    """The reference's production mode draws 50 x rand() % n per neighbourhood in sample order (quadric.cpp:177-193): a
    rank's first draw offset is what the earlier slices consume."""
    from agile_grasp_amd import binding

    sc = small_scene
    one = binding.Context(sc.cam_origins, normals_mode=binding.NORMALS_RAND50, rand_seed=5)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    ctxs = _group(sc, 4, normals_mode=binding.NORMALS_RAND50, rand_seed=5)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        _same(hyps, ref)
    with pytest.raises(binding.AghError) as e:  # the offline all-points pass is not sharded in this mode: loud
        _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples, calculates_antipodal=True))
    assert e.value.code == -8
    # ... and recoverable: every rank returned the same error before any collective, so the communicator is still usable
    # (the abort wrapper used to poison the in-process group on this return)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        assert len(hyps) == len(ref)
    with pytest.raises(binding.AghError) as e:  # classify without a model: the same on every rank, the same recoverable kind
        _run_ranks(ctxs, lambda r, c: c.classify_sharded())
    assert e.value.code == -6
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        assert len(hyps) == len(ref)


def test_segment_overflow_switches_every_rank_to_full_segments(small_scene):
    from agile_grasp_amd import binding

    sc = small_scene
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    ctxs = _group(sc, 2)
    for c in ctxs:
        c.comm_set_segment_records(8)  # far too small: a rank finds ~50
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):  # the host variant retries by itself
        _same(hyps, ref)


def test_sharded_edge_cases(tiny_scene):
    """More ranks than samples (empty slices), an empty sample list, a communicator of one."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    few = sc.samples[:3]
    ref = one.find_hands(few)
    ctxs = _group(sc, 5)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(few)):
        _same(hyps, ref)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(np.zeros(0, np.int32))):
        assert len(hyps) == 0
    solo = _group(sc, 1)
    _same(solo[0].find_hands_sharded(sc.samples), one.find_hands(sc.samples))
    with pytest.raises(binding.AghError):
        one.find_hands_sharded(sc.samples)  # no communicator


@pytest.mark.parametrize("name", ["C2", "C4"])
def test_full_size_eight_way_sharded_search_against_oracle(svm_model, name):
    """BASELINE configs C2 and C4 sharded eight ways (the in-process communicator: the RCCL schedule with device copies):
    the merged list of EVERY rank against the ORACLE's list -- not against the single-GPU HIP list."""
    from agile_grasp_amd import synthetic
    from oracle import oracle_py as O

    sc = synthetic.config(name)
    w, rho = svm_model
    ref = O.find_hands(O.default_params(sc.cam_origins), sc.xyz, sc.cam, sc.samples, want_images=True)
    okeep, _ = O.classify(ref["images"], w, rho)
    ctxs = _group(sc, 8)
    for c in ctxs:
        c.load_svm(w, rho)
    res = _run_ranks(ctxs, lambda r, c: (c.find_hands_sharded(sc.samples), c.classify_sharded()))
    for hyps, (recs, keep) in res:
        assert len(hyps) == len(ref["hyps"]) > sc.samples.size // 10
        for f in FIELDS:
            if f != "valid":
                assert np.array_equal(hyps[f], ref["hyps"][f]), f
        assert np.array_equal(keep, okeep)


def test_full_size_c5_cloud_per_rank_against_oracle(svm_model):
    """BASELINE config C5 at full size the way `bench.py --gpus 8` issues it: a communicator of EIGHT ranks,
    rank r holds cloud C5_r (300 000 points) and searches its own 2000 samples -- its slice of the concatenated 16 000-entry
    list -- through the sharded call, with the device-resident entry points and the classify exchange bench.py uses.  The
    merged list of EVERY rank is compared with the ORACLE's eight lists laid end to end, not with a HIP list."""
    import torch

    from agile_grasp_amd import binding, synthetic
    from oracle import oracle_py as O

    G = 8
    w, rho = svm_model
    scenes = [synthetic.config(f"C5_{r}") for r in range(G)]
    S = scenes[0].samples.size
    assert all(sc.samples.size == S and sc.n == 300_000 for sc in scenes)
    refs, okeeps = [], []
    for sc in scenes:
        ref = O.find_hands(O.default_params(sc.cam_origins), sc.xyz, sc.cam, sc.samples, want_images=True)
        keep, _ = O.classify(ref["images"], w, rho)
        refs.append(ref["hyps"])
        okeeps.append(np.asarray(keep, np.uint8))
    total = sum(len(r) for r in refs)
    assert total > G * S // 10
    dev = torch.device("cuda", 0)
    ctxs = [binding.Context(sc.cam_origins) for sc in scenes]
    for c in ctxs:
        c.load_svm(w, rho)
    binding.comm_init_local(ctxs)

    def search(r, c):
        sc = scenes[r]
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            xyz_t, cam_t = torch.from_numpy(sc.xyz).to(dev), torch.from_numpy(sc.cam).to(dev)
            s_all = torch.zeros(G * S, dtype=torch.int32, device=dev)
            s_all[r * S:(r + 1) * S] = torch.from_numpy(sc.samples).to(dev)
            out_t = torch.zeros(8 * S * G * 160, dtype=torch.uint8, device=dev)
            nout_t = torch.zeros(1, dtype=torch.int64, device=dev)
            keep_t = torch.zeros(8 * S * G, dtype=torch.uint8, device=dev)
        st.synchronize()
        for attempt in range(3):  # (AGH_ERR_RETRY: capacity classes / segment size, learnt by every rank from the same headers)
            c.set_cloud_torch(xyz_t, cam_t, stream=st.cuda_stream)
            c.find_hands_sharded_torch(s_all, out_t, nout_t, stream=st.cuda_stream)
            c.classify_sharded_torch(keep_t, stream=st.cuda_stream)
            st.synchronize()
            try:
                c.synchronize()
                break
            except binding.AghError as e:
                if e.code != binding.AGH_ERR_RETRY or attempt == 2:
                    raise
        n = int(nout_t.item())
        recs = np.frombuffer(out_t.cpu().numpy().tobytes(), dtype=binding.HYP_DTYPE)[:n].copy()
        return recs, keep_t.cpu().numpy()[:n].copy()

    for hyps, keep in _run_ranks(ctxs, search):
        assert len(hyps) == total
        at = 0
        for r, ref in enumerate(refs):
            part = hyps[at:at + len(ref)]
            assert np.array_equal(part["sample"], ref["sample"] + r * S), r
            for f in FIELDS:
                if f not in ("sample", "valid"):
                    assert np.array_equal(part[f], ref[f]), (r, f)
            assert np.array_equal(keep[at:at + len(ref)], okeeps[r]), r
            assert np.array_equal(part["svm_keep"], okeeps[r]), r
            at += len(ref)


def test_solo_communicator_runs_the_all_points_pass_in_the_production_mode(tiny_scene):
    """A communicator of one may combine RAND50 with calculates_antipodal (the rand() stream runs through all N points, then
    the samples -- ADVICE r2: the draw table was sized for the samples only)."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    sc = tiny_scene
    solo = _group(sc, 1, normals_mode=binding.NORMALS_RAND50, rand_seed=7)
    got = solo[0].find_hands_sharded(sc.samples, calculates_antipodal=True)
    one = binding.Context(sc.cam_origins, normals_mode=binding.NORMALS_RAND50, rand_seed=7)
    one.set_cloud(sc.xyz, sc.cam)
    _same(got, one.find_hands(sc.samples, calculates_antipodal=True))
    ref = O.find_hands(O.default_params(sc.cam_origins, normals_mode=O.NORMALS_RAND50, rand_seed=7), sc.xyz, sc.cam, sc.samples,
                       calculates_antipodal=True)["hyps"]
    assert len(got) == len(ref)
    for f in FIELDS:
        if f != "valid":
            assert np.array_equal(got[f], ref[f]), f
    assert got["half_antipodal"].sum() > 0


def test_rccl_communicator_of_one(tiny_scene, svm_model):
    """RCCL bound at run time, ncclCommInitRank on the context's device, ncclAllGather on the search's stream."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    ctx = binding.Context(sc.cam_origins)
    ctx.set_cloud(sc.xyz, sc.cam)
    ref = ctx.find_hands(sc.samples)
    ctx.load_svm(*svm_model)
    ref_keep = ctx.classify()
    ctx.comm_init(0, 1, binding.comm_unique_id())
    assert ctx.comm_rank() == (0, 1)
    hyps = ctx.find_hands_sharded(sc.samples)
    _same(hyps, ref)
    recs, keep = ctx.classify_sharded()
    assert np.array_equal(keep, ref_keep)
    anti = ctx.find_hands_sharded(sc.samples, calculates_antipodal=True)
    ctx.comm_destroy()
    _same(anti, ctx.find_hands(sc.samples, calculates_antipodal=True))
    # ONE RCCL image in the process: the library binds the copy torch mapped (RTLD_NOLOAD) instead of loading a second one
    import torch  # noqa: F401  (maps torch/lib/librccl.so if it was not mapped yet -- it is, by the session's fixtures)

    images = {line.split()[-1] for line in open("/proc/self/maps") if "librccl" in line}
    assert len(images) == 1, images
    assert binding.comm_rccl_origin().startswith(("already mapped", "loaded"))


def test_cpp_adapter_sharded_search(tmp_path, small_scene, svm_model):
    """The C++ host side: HandSearch::joinLocalCommunicator / findHands / Learning::classify as collectives (one host thread
    per rank), against the single-GPU C ABI."""
    import os
    import subprocess

    from agile_grasp_amd import binding, build
    from tests.test_cpp_adapter import GOLD, ROOT, _dump

    build.build()
    sc = small_scene
    exe = str(tmp_path / "sharded_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sharded_test.cpp"), "-o", exe, "-L" + libdir, "-lagile_grasp_hip",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    cloud = str(tmp_path / "cloud.bin")
    _dump(sc, cloud)
    out = subprocess.run([exe, cloud, os.path.join(GOLD, "svm_032015_linear_20_20_same"), "3"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    ctx = binding.Context(sc.cam_origins)
    ctx.set_cloud(sc.xyz, sc.cam)
    hyps = ctx.find_hands(sc.samples)
    ctx.load_svm(*svm_model)
    keep = ctx.classify()
    exp = [[float(h["surface"][0]), float(h["bottom"][1]), float(h["approach"][2]), float(h["width"])] for h in hyps]
    for g in range(3):
        assert f"RANK {g} {len(hyps)} {int(keep.sum())}" in lines
        assert [[float(v) for v in l.split()[1:]] for l in lines if l.startswith(f"H{g} ")] == exp
        assert [int(l.split()[1]) for l in lines if l.startswith(f"K{g} ")] == list(np.nonzero(keep)[0])
    # the lazy point getters: one owner per hypothesis, its points are the single-GPU search's, the other ranks return none
    plines = [l.split() for l in lines if l.startswith("P ")]
    assert len(plines) == (len(hyps) + 4) // 5
    for _p, i, owners, cols, n_box, foreign, total in plines:
        pts, _cam = ctx.learning_points(int(i))
        assert int(owners) == 1 and int(cols) == int(n_box) == pts.shape[1] and int(foreign) == 0
        assert float(total) == (float(np.cumsum(pts.T.reshape(-1))[-1]) if pts.size else 0.0)  # sequential sum, point-major


# ---- round 5: every rank takes the same branch (the table of early returns) ----
def _run_ranks_codes(ctxs, fn):
    """Like _run_ranks, but returns (result or None, AghError code or 0) per rank instead of raising the first error."""
    from agile_grasp_amd import binding

    def wrapped(r, c):
        try:
            return fn(r, c), 0
        except binding.AghError as e:
            return None, e.code

    return _run_ranks(ctxs, wrapped)


def test_bad_sample_index_in_one_slice_fails_on_every_rank_alike(tiny_scene):
    """the host variant used to range-check only the rank's own slice BEFORE the collectives, so one rank alone
    returned while the others went into the all-gather (a hang under RCCL, an aborted in-process communicator).  Now the
    kernels validate, the finding travels in the segment header, and every rank returns AGH_ERR_INVALID_ARGUMENT after the
    exchange -- and the communicator is still usable."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    ctxs = _group(sc, 4)
    bad = sc.samples.copy()
    bad[-1] = sc.xyz.shape[0] + 5  # only the LAST rank's slice holds it
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(bad))
    assert [code for _, code in res] == [binding.AGH_ERR_INVALID_ARGUMENT] * 4
    bad[-1] = -3
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(bad))
    assert [code for _, code in res] == [binding.AGH_ERR_INVALID_ARGUMENT] * 4
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):  # the communicator survived
        _same(hyps, ref)


def test_too_small_output_buffer_is_recoverable(tiny_scene):
    """`n > cap` is reported after the collectives with *n_out set so that the caller can come back with a larger
    buffer -- which needs a communicator that was not aborted on the way out."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    assert len(ref) > 4
    ctxs = _group(sc, 3)
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples, cap=4))
    assert [code for _, code in res] == [binding.AGH_ERR_CAPACITY] * 3
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        _same(hyps, ref)


def test_ranks_with_different_capacity_class_state_decide_alike(small_scene):
    """One context of the communicator has launched the larger Taubin capacity classes before (it searched a dense cloud on its
    own), the others have not.  The retry must be every rank's decision or nobody's: it is taken from the gathered segment
    headers (which say whether the reporting rank had the classes on), not from a rank's own big_classes."""
    from agile_grasp_amd import binding

    sc = small_scene  # over-dense: its neighbourhoods need the 4096 class
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)  # (the host entry point repeats by itself after AGH_ERR_RETRY)
    ctxs = [binding.Context(sc.cam_origins) for _ in range(3)]
    for c in ctxs:
        c.set_cloud(sc.xyz, sc.cam)
    ctxs[1].find_hands(sc.samples)  # rank 1 switches its larger classes on, alone
    binding.comm_init_local(ctxs)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        _same(hyps, ref)


def test_contexts_with_different_parameters_cannot_form_a_communicator(tiny_scene):
    from agile_grasp_amd import binding

    sc = tiny_scene
    a = binding.Context(sc.cam_origins)
    b = binding.Context(sc.cam_origins, normals_mode=binding.NORMALS_RAND50)  # would issue one more collective per call
    with pytest.raises(binding.AghError) as e:
        binding.comm_init_local([a, b])
    assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT
    c = binding.Context(sc.cam_origins, finger_width=0.012)
    with pytest.raises(binding.AghError):
        binding.comm_init_local([a, c])
    binding.comm_init_local([a, binding.Context(sc.cam_origins)])  # the same parameters: fine


def test_antipodal_pass_refuses_clouds_of_different_sizes_on_every_rank(tiny_scene):
    """calculates_antipodal shards the all-points pass by POINT range: it needs the same cloud on every rank.  With clouds of
    different sizes the normals' all-gather would carry different byte counts per rank; the sizes are exchanged first and every
    rank refuses alike, leaving the communicator usable for the plain search (where a cloud per rank is a supported mode)."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    ctxs = [binding.Context(sc.cam_origins) for _ in range(3)]
    ctxs[0].set_cloud(sc.xyz, sc.cam)
    ctxs[1].set_cloud(sc.xyz[:-7], sc.cam[:-7])
    ctxs[2].set_cloud(sc.xyz, sc.cam)
    binding.comm_init_local(ctxs)
    few = sc.samples[sc.samples < sc.xyz.shape[0] - 7]
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(few, calculates_antipodal=True))
    assert [code for _, code in res] == [binding.AGH_ERR_STATE] * 3
    res = _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(few))  # still usable
    assert len({len(h) for h in res}) == 1 and len(res[0]) > 0


# ---- round 6: no rank leaves alone ----
@pytest.mark.parametrize("site, host", [(1, False), (2, False), (2, True), (16, True)])
def test_a_rank_that_fails_on_its_own_takes_part_and_every_rank_returns(tiny_scene, site, host):
    """VERDICT r5 item 7.  Rank 1 of three fails on its own after the argument checks -- its per-call buffers cannot be allocated
    (sites 1 / 16), its Taubin launch fails (2).  It used to return at once and leave its peers inside the all-gather (raw RCCL: for
    ever; in-process: the group aborted).  Now it takes part with an empty segment whose header says so: the failing rank returns its
    own error, the others AGH_ERR_STATE, nobody hangs, and the communicator is usable for the next call."""
    import torch

    from agile_grasp_amd import binding

    sc = tiny_scene
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    ctxs = _group(sc, 3)
    ctxs[1].comm_inject_fault(site)
    if host:
        res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
    else:
        S = sc.samples.size
        s_t = torch.from_numpy(sc.samples).cuda()
        bufs = [(torch.zeros(8 * S * 160, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
                for _ in ctxs]

        def dev(r, c):
            c.find_hands_sharded_torch(s_t, bufs[r][0], bufs[r][1])
            c.synchronize()  # (device variants report the merged flags here)

        res = _run_ranks_codes(ctxs, dev)
    codes = [code for _, code in res]
    assert codes[1] == binding.AGH_ERR_HIP and codes[0] == codes[2] == binding.AGH_ERR_STATE, codes
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):  # the communicator survived
        _same(hyps, ref)


def test_a_rank_without_a_cloud_fails_the_call_on_every_rank(tiny_scene):
    """`!has_cloud` on ONE rank (a caller's bug) used to be that rank's early return and its peers' hang.  The rank now takes part
    like one with an empty cloud and flags its header: AGH_ERR_NO_CLOUD on every rank, communicator usable."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    ctxs = [binding.Context(sc.cam_origins) for _ in range(3)]
    ctxs[0].set_cloud(sc.xyz, sc.cam)
    ctxs[2].set_cloud(sc.xyz, sc.cam)
    binding.comm_init_local(ctxs)
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
    assert [code for _, code in res] == [binding.AGH_ERR_NO_CLOUD] * 3
    ctxs[1].set_cloud(sc.xyz, sc.cam)
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        _same(hyps, ref)


def test_exchange_buffer_growth_is_agreed_on(tiny_scene):
    """The buffers the collectives themselves need are grown first and the outcome is agreed on (8 bytes per rank, only on a call
    that grows one): a rank that is out of memory makes EVERY rank return AGH_ERR_HIP before the first variable-size collective,
    and the next call grows them again on every rank."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    ref = one.find_hands(sc.samples)
    ctxs = _group(sc, 3)
    ctxs[2].comm_inject_fault(4)
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
    assert [code for _, code in res] == [binding.AGH_ERR_HIP] * 3
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        _same(hyps, ref)
    # the same in the offline all-points pass (its cloud sizes travel with the same words)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples, calculates_antipodal=True)):
        assert len(hyps) == len(ref)


def test_a_rank_that_cannot_classify_fails_the_call_on_every_rank(tiny_scene, svm_model):
    """agh_classify_sharded: no SVM on one rank, or its HOG / SVM launch fails -- the rank still joins the label exchange."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    ctxs = _group(sc, 3)
    for r in (0, 2):
        ctxs[r].load_svm(*svm_model)
    _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
    res = _run_ranks_codes(ctxs, lambda r, c: c.classify_sharded())
    codes = [code for _, code in res]
    assert codes[1] == binding.AGH_ERR_NO_SVM and codes[0] == codes[2] == binding.AGH_ERR_STATE, codes
    ctxs[1].load_svm(*svm_model)
    _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
    ctxs[0].comm_inject_fault(8)
    res = _run_ranks_codes(ctxs, lambda r, c: c.classify_sharded())
    codes = [code for _, code in res]
    assert codes[0] == binding.AGH_ERR_HIP and codes[1] == codes[2] == binding.AGH_ERR_STATE, codes
    _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
    keeps = [k for _, k in _run_ranks(ctxs, lambda r, c: c.classify_sharded())]
    assert all(np.array_equal(k, keeps[0]) for k in keeps) and keeps[0].size > 0


# ---- a peer failure in a call that would repeat: every rank returns with that call ----
# Run in a child process: were a rank to go on into the next attempt's all-gathers alone, its peers would wait in the in-process
# barrier, whose timeout is read once per process (AGH_LOCAL_BARRIER_TIMEOUT_S).  The child reports what every rank returned.
_PEER_FAILURE_CHILD = r"""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
from agile_grasp_amd import binding, synthetic
from tests.test_gpu_sharding import FIELDS, _group, _run_ranks, _run_ranks_codes

case, site = sys.argv[1], int(sys.argv[2])
sc = synthetic.config("small")  # over-dense: its neighbourhoods need the 4096 class, so its first sharded call repeats
one = binding.Context(sc.cam_origins)
one.set_cloud(sc.xyz, sc.cam)
ref = one.find_hands(sc.samples)
same = lambda h: len(h) == len(ref) and all(np.array_equal(h[f], ref[f]) for f in FIELDS)
ctxs = _group(sc, 3)
out = {}
if case == "overflow":  # the classes are on everywhere; then segments far too small: the call would repeat with full segments
    out["warm"] = all(same(h) for h in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)))
    for c in ctxs:
        c.comm_set_segment_records(8)
ctxs[1].comm_inject_fault(site)
t0 = time.time()
if case == "device":
    import torch

    S = sc.samples.size
    s_t = torch.from_numpy(sc.samples).cuda()
    bufs = [(torch.zeros(8 * S * 160, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
            for _ in ctxs]

    def dev(r, c):
        c.find_hands_sharded_torch(s_t, bufs[r][0], bufs[r][1])
        c.synchronize()  # (device variants report the merged flags here)

    res = _run_ranks_codes(ctxs, dev)
else:
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
out["seconds"] = time.time() - t0
out["codes"] = [code for _, code in res]
if case == "classify":  # after that failed search: classify_sharded fails on every rank too, and returns no list
    for c in ctxs:
        c.load_svm(np.ones(3528, np.float32), 0.0)
        c.shard_n = 0  # (no list came back)
    t0 = time.time()
    res = _run_ranks_codes(ctxs, lambda r, c: c.classify_sharded())
    out["classify_seconds"] = time.time() - t0
    out["classify_codes"] = [code for _, code in res]
    out["classify_lists"] = [v is not None for v, _ in res]
follow = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
out["follow_codes"] = [code for _, code in follow]
out["follow_same"] = [bool(code == 0 and same(h)) for h, code in follow]
out["segment_bytes"] = [c.comm_last_exchange()[0] for c in ctxs]
print(json.dumps(out))
"""


@pytest.mark.parametrize("case, site", [("host", 1), ("host", 2), ("host", 16), ("device", 2), ("overflow", 2),
                                        ("classify", 16)])
def test_a_peer_failure_in_a_call_that_would_repeat_returns_on_every_rank(case, site):
    """ADVICE r6 item 1.  Rank 1 fails on its own in the same call where the others' slices ask for a larger capacity class
    (small_scene's first sharded call) or for full segments ("overflow").  The peer failure is checked before the repeat: every
    rank returns with this call -- rank 1 its own AGH_ERR_HIP, the others AGH_ERR_STATE -- none switches big_classes or
    shard_full_exchange on it, and the next call agrees on everything and returns the single-context list on every rank.
    ("classify": after such a failed search, agh_classify_sharded fails on every rank too, with rank 1 taking part.)"""
    import json
    import os
    import subprocess
    import sys

    from agile_grasp_amd import binding

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AGH_LOCAL_BARRIER_TIMEOUT_S="60")
    p = subprocess.run([sys.executable, "-c", _PEER_FAILURE_CHILD, case, str(site)], cwd=root, env=env, capture_output=True,
                       text=True, timeout=400)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out.get("warm", True)
    assert out["codes"][1] == binding.AGH_ERR_HIP and out["codes"][0] == out["codes"][2] == binding.AGH_ERR_STATE, out
    assert out["seconds"] < 30, out  # (returned together, not released by the 60 s barrier timeout)
    if case == "classify":
        assert all(code != 0 for code in out["classify_codes"]) and not any(out["classify_lists"]), out
        assert out["classify_seconds"] < 30, out
    assert out["follow_codes"] == [0, 0, 0] and all(out["follow_same"]), out
    assert len(set(out["segment_bytes"])) == 1, out


# ---- agh_classify_sharded after a classification that failed on one rank ----
def _classify_ref(sc, svm_model):
    from agile_grasp_amd import binding

    one = binding.Context(sc.cam_origins)
    one.set_cloud(sc.xyz, sc.cam)
    one.load_svm(*svm_model)
    ref = one.find_hands(sc.samples)
    return ref, one.classify()


@pytest.mark.parametrize("how", ["no_svm", "site8"])
def test_a_failed_classification_leaves_no_stale_failure_behind(tiny_scene, svm_model, how):
    """A classification that failed on one rank marks that rank's segment header; the in-place all-gather never rewrites a
    rank's own segment, so the mark used to outlive the call and fail every later classification of the same search.  A
    corrected repeat -- with no search in between -- returns the single-context labels on every rank."""
    from agile_grasp_amd import binding

    sc = tiny_scene
    ref, keep_ref = _classify_ref(sc, svm_model)
    assert keep_ref.any() and not keep_ref.all()
    ctxs = _group(sc, 3)
    for r in (0, 2):
        ctxs[r].load_svm(*svm_model)
    if how == "site8":
        ctxs[1].load_svm(*svm_model)
        ctxs[1].comm_inject_fault(8)
    for hyps in _run_ranks(ctxs, lambda r, c: c.find_hands_sharded(sc.samples)):
        _same(hyps, ref)
    res = _run_ranks_codes(ctxs, lambda r, c: c.classify_sharded())
    codes = [code for _, code in res]
    want = binding.AGH_ERR_NO_SVM if how == "no_svm" else binding.AGH_ERR_HIP
    assert codes[1] == want and codes[0] == codes[2] == binding.AGH_ERR_STATE, codes
    if how == "no_svm":
        ctxs[1].load_svm(*svm_model)
    for recs, keep in _run_ranks(ctxs, lambda r, c: c.classify_sharded()):  # no search in between
        _same(recs, ref)
        assert np.array_equal(keep, keep_ref)


# ---- a localize chain in flight on one rank (include/agh.h: only agh_localize_stage between begin and end) ----
def test_a_rank_with_a_localize_chain_in_flight_takes_part_without_touching_it(tiny_scene, svm_model):
    """Rank 1 has a localize chain in flight.  The sharded search and classification may not return on it before their
    collectives: it takes part without searching (its flags and count in scratch of its own), every rank returns an error,
    the chain's results are those of an uninterrupted agh_localize, and the communicator works afterwards."""
    from agile_grasp_amd import binding, synthetic

    sc = tiny_scene
    raw = synthetic.make_raw_cloud(40_000, seed=5)
    kw = dict(n_samples=60, sample_seed=7, classify=True, min_inliers=2)
    solo = binding.Context(sc.cam_origins)
    solo.load_svm(*svm_model)
    chain_ref = solo.localize(raw.xyz, raw.size_left, raw.workspace, **kw)
    ref, keep_ref = _classify_ref(sc, svm_model)

    ctxs = _group(sc, 3)
    for c in ctxs:
        c.load_svm(*svm_model)
    for recs, keep in _run_ranks(ctxs, lambda r, c: (c.find_hands_sharded(sc.samples), c.classify_sharded())[1]):
        _same(recs, ref)
    ctxs[1].localize_begin(raw.xyz, raw.size_left, raw.workspace, **kw)
    res = _run_ranks_codes(ctxs, lambda r, c: c.classify_sharded())  # (of the search before the chain)
    assert all(v is None for v, _ in res) and [code for _, code in res] == [binding.AGH_ERR_STATE] * 3, res
    res = _run_ranks_codes(ctxs, lambda r, c: c.find_hands_sharded(sc.samples))
    assert all(v is None for v, _ in res) and [code for _, code in res] == [binding.AGH_ERR_STATE] * 3, res
    got = ctxs[1].localize_end()
    for k in ("handles", "inlier_idx", "samples"):
        assert np.array_equal(got[k], chain_ref[k]), k
    _same(got["hands"], chain_ref["hands"])  # (every field but the call's stamp)
    assert len(got["hands"]) > 0
    assert got["n_hypotheses"] == chain_ref["n_hypotheses"]
    ctxs[1].set_cloud(sc.xyz, sc.cam)  # (the chain searched its own cloud)
    for recs, keep in _run_ranks(ctxs, lambda r, c: (c.find_hands_sharded(sc.samples), c.classify_sharded())[1]):
        _same(recs, ref)
        assert np.array_equal(keep, keep_ref)
