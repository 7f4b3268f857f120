"""The return codes and error texts of the localize chains' argument checks, and what the twelve agh_get_* getters of the chains
answer after every kind of chain, held against tests/golden/localize_error_texts.json.

The golden file is a recording, not a model: generate() below (not run by pytest) replays the same tables on the commit named in
the file's "parent" field and writes what the library answered there.  The tests replay the tables on the checked-out code and
want the same code and the same string, byte for byte -- the texts are behaviour (include/agh.h names them), and which of two
faults a call reports pins the order of the rules.

Every invalid call fails in argument checking, before anything is queued; the chains of the getter sequence run the `tiny`
scene with 8 samples (2 captures for the batch forms)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "localize_error_texts.json")
S, NC, CAP = 8, 2, 512
KINDS = {"plain": "", "masked": "_masked", "labeled": "_labeled", "clustered": "_clustered", "fit": "_clustered_fit"}


def entry_points():
    """Every agh_localize* entry point that starts a chain: name -> (batch, depth, kind)."""
    out = {}
    for batch in (False, True):
        for depth in (False, True):
            for kind, ks in KINDS.items():
                if batch:
                    suffixes = ("", "_device", "_begin", "_begin_device")
                else:  # (the single chain has a begin for its plain and masked forms only, and none for device memory)
                    suffixes = ("", "_device", "_begin") if kind in ("plain", "masked") else ("", "_device")
                for sfx in suffixes:
                    out["agh_localize" + ("_depth" if depth else "") + ("_batch" if batch else "") + ks + sfx] = (batch, depth, kind)
    return out


ENTRY = entry_points()


# ---- the invalid calls: (case name, applies(batch, depth, kind), mutation of the valid arguments) ----

def _last(a, field):
    return a[field][a["C"] - 1]


def _null_source(a):
    a["mrecs" if a["depth"] else "masks"] = None


def _null_source_capture_1(a):
    if a["depth"]:
        a["mrecs"][2].data = a["mrecs"][3].data = None
    else:
        a["masks"][1] = None


def _set(field, **values):
    def f(a):
        for k, v in values.items():
            setattr(_last(a, field), k, v)
    return f


def _sample_idx(a):
    _last(a, "lp").sample_idx = a["idx"].ctypes.data_as(C.POINTER(C.c_int32))


def _objects(*values):
    def f(a):
        for k in range(a["C"]):
            v = values[k] if a["batch"] else values[-1]
            if a["kind"] == "labeled":
                a["n_objects"][k] = v
            else:
                a["cp"][k].max_objects = v
    return f


def _too_many_samples(a):
    _objects(1, 60)(a)  # (61 lists in a batch: below the limit of the lists)
    _last(a, "lp").n_samples = (1 << 24) // 60 + 1


def _plane(*p):
    def f(a):
        for q in range(4):
            _last(a, "cp").plane[q] = p[q]
    return f


def _nan(field, index=None):
    def f(a):
        if index is None:
            setattr(_last(a, "cp"), field, float("nan"))
        else:
            _last(a, "cp").plane[index] = float("nan")
    return f


def _stride_below_width(a):
    a["mrecs"][len(a["mrecs"]) - 1].row_stride_bytes = 8  # (image 1 of the last capture; the images are 16 wide)


def _every_image_null(a):
    for r in a["mrecs"]:
        r.data = None


def _out(index, value):
    def f(a):
        a["outs"][index] = value
    return f


def _over_limit_samples_and_null(a):
    for k in range(a["C"]):
        a["lp"][k].n_samples = 1 << 24
    a["masks"][1] = None


def _over_limit_points_and_null(a):
    for k in range(a["C"]):
        a["n"][k] = 1 << 29
    a["masks"][1] = None


def _all(f, g):
    def h(a):
        f(a)
        g(a)
    return h


def _none(field):
    def f(a):
        a[field] = None
    return f


BYTES = ("masked", "labeled")
OBJECTS = ("labeled", "clustered", "fit")
CLUSTERS = ("clustered", "fit")
BASE = ("agh_localize_clustered", "agh_localize_batch_clustered", "agh_localize_depth_clustered_fit_device",
        "agh_localize_depth_batch_clustered_fit_begin")  # (the entry points that run every cluster fault)

# (name, predicate over (entry point, batch, depth, kind), mutation)
CASES = [
    ("source NULL", lambda n, b, d, k: k in BYTES, _null_source),
    ("source NULL for capture 1 only", lambda n, b, d, k: b and k in BYTES, _null_source_capture_1),
    ("n_objects array NULL", lambda n, b, d, k: b and k == "labeled", _none("n_objects")),
    ("cp NULL", lambda n, b, d, k: k in CLUSTERS, _none("cp")),
    ("fp NULL", lambda n, b, d, k: k == "fit", _none("fp")),
    ("sample_idx given", lambda n, b, d, k: k != "plain", _sample_idx),
    ("objects 0", lambda n, b, d, k: k in OBJECTS, _objects(2, 0)),
    ("objects 65", lambda n, b, d, k: k in OBJECTS, _objects(2, 65)),
    ("more than 64 lists at capture 1", lambda n, b, d, k: b and k in OBJECTS, _objects(40, 40)),
    ("objects x n_samples above 2^24", lambda n, b, d, k: k in OBJECTS, _too_many_samples),
    ("two faults: source NULL and sample_idx", lambda n, b, d, k: k in BYTES, _all(_null_source, _sample_idx)),
    ("two faults: objects x n_samples above 2^24 and sample_idx", lambda n, b, d, k: k in OBJECTS, _all(_too_many_samples, _sample_idx)),
    ("two faults: objects 65 and source NULL", lambda n, b, d, k: k == "labeled", _all(_objects(2, 65), _null_source)),
    ("plane not unit", lambda n, b, d, k: n in BASE, _plane(0.0, 0.0, 2.0, 0.0)),
    ("min_height >= max_height", lambda n, b, d, k: n in BASE, _set("cp", min_height=0.5, max_height=0.5)),
    ("tolerance 0", lambda n, b, d, k: k in CLUSTERS, _set("cp", tolerance=0.0)),
    ("tolerance 0.06", lambda n, b, d, k: n in BASE, _set("cp", tolerance=0.06)),
    ("min_voxels 0", lambda n, b, d, k: n in BASE, _set("cp", min_voxels=0)),
    ("plane[0] NaN", lambda n, b, d, k: n in BASE, _nan(None, 0)),
    ("plane[1] NaN", lambda n, b, d, k: n in BASE, _nan(None, 1)),
    ("plane[2] NaN", lambda n, b, d, k: n in BASE, _nan(None, 2)),
    ("plane[3] NaN", lambda n, b, d, k: n in BASE, _nan(None, 3)),
    ("min_height NaN", lambda n, b, d, k: n in BASE, _nan("min_height")),
    ("max_height NaN", lambda n, b, d, k: n in BASE, _nan("max_height")),
    ("tolerance NaN", lambda n, b, d, k: n in BASE, _nan("tolerance")),
    ("fit: n_candidates 0", lambda n, b, d, k: k == "fit", _set("fp", n_candidates=0)),
    ("fit: min_inliers 2 and a cluster fault", lambda n, b, d, k: k == "fit", _all(_set("fp", min_inliers=2), _set("cp", tolerance=0.0))),
    ("fit: the caller's plane is garbage (accepted)", lambda n, b, d, k: n in ("agh_localize_clustered_fit", "agh_localize_batch_clustered_fit"),
     _plane(float("nan"), 5.0, 7.0, float("inf"))),
    ("mask stride below width, last image", lambda n, b, d, k: d and k in BYTES, _stride_below_width),
    ("every image mask NULL", lambda n, b, d, k: d and k in BYTES, _every_image_null),
    ("outputs: negative capacity", lambda n, b, d, k: "_begin" not in n and "_device" not in n and k in ("plain", "masked", "clustered"),
     _out(1, C.c_int64(-1))),
    ("outputs: NULL with a capacity", lambda n, b, d, k: "_begin" not in n and "_device" not in n and k in ("plain", "masked", "clustered"),
     _out(2, None)),
    ("two faults: samples over the limit and a NULL source", lambda n, b, d, k: b and not d and k in BYTES, _over_limit_samples_and_null),
    ("two faults: points over the limit and a NULL source", lambda n, b, d, k: b and not d and k in BYTES, _over_limit_points_and_null),
]


def cases_of(name):
    b, d, k = ENTRY[name]
    return [(cn, mut) for cn, pred, mut in CASES if pred(name, b, d, k)]


# ---- the arguments ----

class Env:
    """One context, the tiny scene as a raw capture on the host and on the device, two tiny depth images per capture."""

    def __init__(self):
        import torch

        from agile_grasp_amd import binding as B
        from agile_grasp_amd import synthetic
        from tests import depth_captures as D

        self.B = B
        sc = synthetic.config("tiny")
        self.ctx = B.Context(sc.cam_origins)
        self.lib, self.h = self.ctx.lib, self.ctx._h
        self.xyz = np.ascontiguousarray(sc.xyz, np.float32)
        self.n = self.xyz.shape[0]
        self.size_left = int((sc.cam == 0).sum())
        lo, hi = self.xyz.min(0).astype(np.float64) - 0.05, self.xyz.max(0).astype(np.float64) + 0.05
        self.workspace = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]
        normal = synthetic._tilt() @ np.array([0.0, 0.0, 1.0])
        self.plane = [*normal, -float(normal @ synthetic._PIVOT)]  # (the table of the tilted scene: it passes through the pivot)
        self.labels = (np.arange(self.n) % 2 + 1).astype(np.uint8)
        self.d_xyz = torch.from_numpy(self.xyz).cuda()
        self.d_labels = torch.from_numpy(self.labels).cuda()
        rng = np.random.default_rng(5)
        self.images = [D._random_image(rng, 16, 12, D.F32, cam=j % 2) for j in range(2 * NC)]
        self.d_images = [dict(im, data=torch.from_numpy(np.ascontiguousarray(im["data"])).cuda()) for im in self.images]
        self.image_masks = [np.ones((12, 16), np.uint8) for _ in range(2 * NC)]
        self.d_image_masks = [torch.from_numpy(m).cuda() for m in self.image_masks]
        self.idx = np.arange(S, dtype=np.int32)
        self.bufs = (np.zeros(CAP, B.HANDLE_DTYPE), np.zeros(CAP, np.int32), np.zeros(CAP, B.HYP_DTYPE), np.zeros(4096, np.int32))
        torch.cuda.synchronize()

    def args(self, name):
        B = self.B
        batch, depth, kind = ENTRY[name]
        dev = name.endswith("_device")
        Cn = NC if batch else 1
        a = dict(name=name, batch=batch, depth=depth, kind=kind, begin="_begin" in name, C=Cn, idx=self.idx, keep=[])
        a["lp"] = (B.AghLocalizeParams * Cn)()
        for p in a["lp"]:
            p.size_left, p.dense, p.classify = (0, 1, 0) if depth else (self.size_left, 0, 0)
            for q in range(6):
                p.workspace[q] = (-10.0, 10.0)[q % 2] if depth else float(self.workspace[q])
            p.cell_size, p.sample_idx, p.n_samples, p.sample_seed = 0.003, None, S, 1
            p.min_inliers, p.filters_boundaries, p.min_length = 2, 0, 0.005
        if depth:
            images = (self.d_images if dev else self.images)[:2 * Cn]
            a["images"], keep, _ = B.depth_image_records(images)
            a["n_images"] = (C.c_int32 * Cn)(*([2] * Cn))
            a["mrecs"], mkeep = B.sample_mask_records((self.d_image_masks if dev else self.image_masks)[:2 * Cn], dev)
            a["keep"] += [keep, mkeep]
        else:
            ptr = self.d_xyz.data_ptr() if dev else self.xyz.ctypes.data
            bytes_ptr = self.d_labels.data_ptr() if dev else self.labels.ctypes.data  # (1 or 2: a mask of all points, or labels)
            a["xyz"] = (C.c_void_p * Cn)(*([ptr] * Cn))
            a["stride"] = (C.c_int64 * Cn)(*([12] * Cn))
            a["n"] = (C.c_int64 * Cn)(*([self.n] * Cn))
            a["masks"] = (C.c_void_p * Cn)(*([bytes_ptr] * Cn))
        a["n_objects"] = (C.c_int32 * Cn)(*([2] * Cn))
        a["cp"] = (B.AghClusterParams * Cn)()
        a["fp"] = (B.AghPlaneFitParams * Cn)()
        for k in range(Cn):
            a["cp"][k] = B.cluster_params(plane=self.plane, max_objects=2, min_voxels=20)
            a["fp"][k] = B.plane_fit_params(n_candidates=16)
        handles, idx, hands, samples = self.bufs
        a["outs"] = [C.c_void_p(handles.ctypes.data), C.c_int64(CAP), C.c_void_p(idx.ctypes.data), C.c_int64(CAP),
                     C.c_void_p(hands.ctypes.data), C.c_int64(CAP), C.c_void_p(samples.ctypes.data)]
        a["result"] = B.AghLocalizeResult() if (not batch and kind in ("plain", "masked")) else (B.AghLocalizeBatchResult * 64)()
        return a

    def call(self, a):
        """The call the record describes: (return code, the context's error text if it failed)."""
        batch, kind = a["batch"], a["kind"]
        first = lambda arr, ct: ct(arr[0]) if arr is not None else ct()
        if a["depth"]:
            v = [a["images"]]
            if kind in BYTES:
                v.append(a["mrecs"])
            v.append(a["n_images"] if batch else first(a["n_images"], C.c_int32))
        else:
            v = [a["xyz"], a["stride"], a["n"]] if batch else [first(a["xyz"], C.c_void_p), first(a["stride"], C.c_int64), first(a["n"], C.c_int64)]
            if kind in BYTES:
                v.append(a["masks"] if batch else first(a["masks"], C.c_void_p))
        if kind == "labeled":
            v.append(a["n_objects"] if batch else first(a["n_objects"], C.c_int32))
        if kind == "fit":
            v.append(a["fp"])
        if kind in CLUSTERS:
            v.append(a["cp"])
        v.append(a["lp"])
        if batch:
            v.append(C.c_int32(a["C"]))
        if not a["begin"]:
            v += a["outs"] + [C.byref(a["result"]) if not isinstance(a["result"], C.Array) else a["result"]]
        rc = int(getattr(self.lib, a["name"])(self.h, *v))
        err = self.lib.agh_last_error(self.h).decode() if rc < 0 else ""
        if a["begin"] and rc == 0:  # (a begin that went through: collect the chain, so that the next case starts clean)
            self.end(batch)
        return rc, err

    def end(self, batch, mutate=None):
        a = self.args("agh_localize_batch" if batch else "agh_localize")
        if mutate:
            mutate(a)
        fn = self.lib.agh_localize_batch_end if batch else self.lib.agh_localize_end
        return int(fn(self.h, *a["outs"], a["result"] if batch else C.byref(a["result"])))

    def run_cases(self, name):
        out = []
        for case, mutate in cases_of(name):
            a = self.args(name)
            mutate(a)
            rc, err = self.call(a)
            out.append({"entry": name, "case": case, "rc": rc, "err": err})
        return out

    def run_in_flight(self, batch):
        """Every entry point, refused while a plain chain is in flight (a single capture's, or a batch's)."""
        out = []
        opener = "agh_localize_batch_begin" if batch else "agh_localize_begin"
        rc = int(getattr(self.lib, opener)(self.h, *self._begin_args(opener)))
        out.append({"entry": opener, "case": "opens the chain", "rc": rc, "err": ""})
        for name in ENTRY:
            r, err = self.call(self.args(name))
            out.append({"entry": name, "case": "a batch chain in flight" if batch else "a single chain in flight", "rc": r, "err": err})
        out.append({"entry": "end", "case": "collects the chain", "rc": self.end(batch), "err": ""})
        # ... and the ends themselves: the other chain's end, bad outputs (which end the chain), no chain at all
        rc = int(getattr(self.lib, opener)(self.h, *self._begin_args(opener)))
        out.append({"entry": opener, "case": "opens a second chain", "rc": rc, "err": ""})
        for case, b, mutate in (("the other kind's end", not batch, None), ("end: negative capacity", batch, _out(3, C.c_int64(-1))),
                                ("end: nothing to collect", batch, None)):
            r = self.end(b, mutate)
            out.append({"entry": "end", "case": case, "rc": r, "err": self.lib.agh_last_error(self.h).decode() if r < 0 else ""})
        return out

    def _begin_args(self, name):
        a = self.args(name)
        self._open = a  # (the arrays stay alive until the end)
        if a["batch"]:
            return [a["xyz"], a["stride"], a["n"], a["lp"], C.c_int32(a["C"])]
        return [C.c_void_p(a["xyz"][0]), C.c_int64(12), C.c_int64(self.n), a["lp"]]

    # ---- the getters ----
    def getters(self):
        """All twelve, in a fixed order: the code, and the text of a refusal or the numbers of an answer."""
        B, lib, h = self.B, self.lib, self.h
        out = []

        def rec(fn, rc, answer):
            rc = int(rc)
            out.append({"fn": fn, "rc": rc, "err": lib.agh_last_error(h).decode()} if rc < 0 else {"fn": fn, "rc": rc, "out": answer()})

        ints = lambda arr: [int(x) for x in arr]
        hexes = lambda arr: [float(x).hex() for x in arr]
        fit = lambda r: {"plane": hexes(r.plane), "counts": [r.n_voxels, r.n_inliers, r.n_refit, r.best_candidate, r.found, r.refined]}
        m1 = C.c_int64(-7)
        rec("agh_get_sample_mask_count", lib.agh_get_sample_mask_count(h, C.byref(m1)), lambda: m1.value)
        m = np.full(64, -7, np.int64)
        rec("agh_get_label_counts", lib.agh_get_label_counts(h, B._p(m, C.c_int64), C.c_int32(64)), lambda: ints(m))
        info, nv, ids = B.AghClusterInfo(), np.full(64, -7, np.int64), np.full(64, -7, np.int32)
        rec("agh_get_cluster_info", lib.agh_get_cluster_info(h, C.byref(info), B._p(nv, C.c_int64), B._p(ids, C.c_int32), C.c_int32(64)),
            lambda: [info.n_foreground, info.n_components, info.n_objects, ints(nv), ints(ids)])
        lab = np.zeros(4 * self.n, np.uint8)
        rec("agh_get_cluster_labels", lib.agh_get_cluster_labels(h, C.c_void_p(lab.ctypes.data), C.c_int64(lab.size)),
            lambda: ints(np.bincount(lab, minlength=4)))
        r = B.AghPlaneFitResult()
        rec("agh_get_plane_fit", lib.agh_get_plane_fit(h, C.byref(r)), lambda: fit(r))
        cnt = np.full(256, -7, np.int64)
        rec("agh_get_plane_fit_candidates", lib.agh_get_plane_fit_candidates(h, None, None, B._p(cnt, C.c_int64), C.c_int32(256)), lambda: ints(cnt))
        m2 = np.full(64, -7, np.int64)
        rec("agh_get_batch_mask_counts", lib.agh_get_batch_mask_counts(h, B._p(m2, C.c_int64), C.c_int32(64)), lambda: ints(m2))
        m3 = np.full(64, -7, np.int64)
        rec("agh_get_batch_label_counts", lib.agh_get_batch_label_counts(h, B._p(m3, C.c_int64), C.c_int32(64)), lambda: ints(m3))
        infos, nv2, ids2 = (B.AghClusterInfo * 64)(), np.full(64, -7, np.int64), np.full(64, -7, np.int32)
        rec("agh_get_batch_cluster_info",
            lib.agh_get_batch_cluster_info(h, infos, B._p(nv2, C.c_int64), B._p(ids2, C.c_int32), C.c_int32(64), C.c_int32(64)),
            lambda: [[[q.n_foreground, q.n_components, q.n_objects] for q in infos[:NC]], ints(nv2), ints(ids2)])
        lab2 = np.zeros(4 * self.n, np.uint8)
        rec("agh_get_batch_cluster_labels", lib.agh_get_batch_cluster_labels(h, C.c_void_p(lab2.ctypes.data), C.c_int64(lab2.size)),
            lambda: ints(np.bincount(lab2, minlength=4)))
        rs = (B.AghPlaneFitResult * 64)()
        rec("agh_get_batch_plane_fit", lib.agh_get_batch_plane_fit(h, rs, C.c_int32(64)), lambda: [fit(q) for q in rs[:NC]])
        cnt2 = np.full(256, -7, np.int64)
        rec("agh_get_batch_plane_fit_candidates",
            lib.agh_get_batch_plane_fit_candidates(h, C.c_int32(1), None, None, B._p(cnt2, C.c_int64), C.c_int32(256)), lambda: ints(cnt2))
        return out

    def run_getter_sequence(self):
        out = [{"after": "nothing", "rc": 0, "getters": self.getters()}]
        for name in SEQUENCE:
            rc, err = self.call(self.args(name))
            out.append({"after": name, "rc": rc, "err": err, "getters": self.getters()})
        return out


SEQUENCE = ["agh_localize_masked", "agh_localize_labeled", "agh_localize_clustered", "agh_localize_clustered_fit", "agh_localize",
            "agh_localize_batch_masked", "agh_localize_batch_labeled", "agh_localize_batch_clustered", "agh_localize_batch_clustered_fit",
            "agh_localize_batch", "agh_localize_clustered_fit", "agh_localize_batch_clustered"]


def generate(path=GOLDEN, parent="unknown"):
    """The recording (run by hand on the parent commit, never by pytest): every table above, as the library answers there."""
    env = Env()
    rec = {"parent": parent, "errors": [], "in_flight": {}, "getters": []}
    for name in ENTRY:
        rec["errors"] += env.run_cases(name)
    for batch in (False, True):
        rec["in_flight"]["batch" if batch else "single"] = env.run_in_flight(batch)
    env.ctx.close()
    env = Env()  # (a fresh context, as the test's)
    rec["getters"] = env.run_getter_sequence()
    env.ctx.close()
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return rec


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        print(g)
        assert g == w, (g, w)


@pytest.mark.parametrize("name", [n for n in ENTRY if cases_of(n)])
def test_invalid_calls_answer_as_recorded(env, golden, name):
    want = [r for r in golden["errors"] if r["entry"] == name]
    assert want, name
    _same(env.run_cases(name), want)


@pytest.mark.parametrize("which", ["single", "batch"])
def test_every_begin_is_refused_while_a_chain_is_in_flight(env, golden, which):
    got = env.run_in_flight(which == "batch")
    refused = [r for r in got if r["case"].endswith("chain in flight")]
    assert len(refused) == len(ENTRY) and all(r["rc"] == env.B.AGH_ERR_STATE for r in refused), refused
    _same(got, golden["in_flight"][which])


def test_getters_after_every_kind_of_chain(golden):
    """single masked, labelled, clustered, fitted, plain; batch the same; then single fitted and batch clustered -- on one fresh
    context, all twelve getters after each."""
    e = Env()
    got = e.run_getter_sequence()
    e.ctx.close()
    assert [g["rc"] for g in got] == [0] * len(got), [(g["after"], g["rc"], g.get("err")) for g in got]
    assert len(got) == len(golden["getters"])
    for g, w in zip(got, golden["getters"]):
        assert g["after"] == w["after"] and g["rc"] == w["rc"]
        for a, b in zip(g["getters"], w["getters"]):
            print(g["after"], a)
            assert a == b, (g["after"], a, b)
