"""CvSVM::train on the device (k_svm_init, k_svm_select, k_svm_update, k_svm_compress, k_svm_gather and the host loop of
svm_train; csrc/train.hip) off the defaults of Learning::convertData: C, eps, step limits around the host loop's looks at the
stop flag, first-step ties across k_svm_select's strides and waves, degenerate sets and one-instance classes, against the
oracle with exact equality on the whole model.

The cases come from tests/svm_train_cases.py; tests/test_svm_train_cases.py proves on the CPU that each one sits in the regime
it is named after, and checks the oracle against an independent numpy transcription, libsvm and the KKT conditions.  The
oracle's answers are computed once for the module (svm_train_cases.oracle)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import svm_train_cases as S

pytestmark = pytest.mark.gpu

CASES = S.cases()


def _ctx():
    from agile_grasp_amd import binding, synthetic

    return binding.Context(synthetic.camera_origins())


@functools.lru_cache(maxsize=None)
def _packed(name):
    from agile_grasp_amd import binding

    return binding.pack_images(CASES[name]["images"])


def _train(ctx, name, **override):
    case = CASES[name]
    kw = dict(C_=case["C"], eps=case["eps"], max_iter=case["max_iter"], kernel=case["kernel"])
    kw.update(override)
    return ctx.train_svm(_packed(name), case["labels"], **kw)


def _assert_model(got, ref, case, what=""):
    """the whole model, bit for bit: step and support-vector counts, rho, class sizes, w (LINEAR) or sv and alpha (POLY2)"""
    labels = case["labels"]
    assert got["iterations"] == ref["iterations"], (what, got["iterations"], ref["iterations"])
    assert got["n_sv"] == ref["n_sv"], (what, got["n_sv"], ref["n_sv"])
    assert got["rho"] == ref["rho"], (what, got["rho"], ref["rho"])
    assert got["n_pos"] == int((labels > 0).sum()) and got["n_neg"] == int((labels <= 0).sum()), what
    _, rsv, ralpha, _ = ref["model"]
    if case["kernel"] == S.LINEAR:
        assert np.array_equal(got["w"], ref["w"]), (what, np.nonzero(got["w"] != ref["w"])[0][:8])
    else:
        assert got["sv"].shape == rsv.shape and got["alpha"].shape == ralpha.shape, (what, got["sv"].shape, rsv.shape)
        assert np.array_equal(got["alpha"], ralpha), (what, np.nonzero(got["alpha"] != ralpha)[0][:8])
        assert np.array_equal(got["sv"], rsv), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(name):
    case = CASES[name]
    _, ref = S.oracle(name)
    _assert_model(_train(_ctx(), name), ref, case, name)


@pytest.mark.parametrize("eps", [0.0, -1.0])
def test_eps_not_positive_is_accepted_and_runs_to_the_step_limit(eps):
    """The gap test `gap < eps` can never fire: 60 steps, one look past the first 50."""
    name = f"eps{eps:g}"
    case = CASES[name]
    assert case["eps"] == eps and case["max_iter"] == 60
    got = _train(_ctx(), name)
    assert got["iterations"] == 60
    _assert_model(got, S.oracle(name)[1], case, name)
    _assert_model(got, S.solve(case, eps=S.FLT_EPSILON), case, "the default eps takes the same 60 steps")


@pytest.mark.parametrize("name", ["C0.002_n257_linear", "C0.05_n65_poly2"])
@pytest.mark.parametrize("cache_rows", [2, 3])
def test_row_cache_under_a_tight_C(name, cache_rows, monkeypatch):
    """Two or three cached kernel rows: nearly every step evicts, and with most alphas at C the pairs return to rows that
    were just dropped.  The values are the same floats, cached or recomputed."""
    case = CASES[name]
    ctx = _ctx()
    full = _train(ctx, name)
    monkeypatch.setenv("AGH_SVM_CACHE_ROWS", str(cache_rows))
    small = _train(ctx, name)
    monkeypatch.delenv("AGH_SVM_CACHE_ROWS")
    assert small["rows_computed"] > full["rows_computed"]
    assert small["rows_computed"] + small["rows_reused"] == 2 * small["iterations"] == 2 * full["iterations"]
    _, ref = S.oracle(name)
    _assert_model(full, ref, case, "whole cache")
    _assert_model(small, ref, case, f"{cache_rows} rows")


def test_trained_off_default_model_predicts(tmp_path):
    """The POLY2 model of a C = 0.05 case: saved, loaded, and run on its own training images."""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    name = "C0.05_n257_poly2"
    case = CASES[name]
    ctx = _ctx()
    got = _train(ctx, name)
    _, ref = S.oracle(name)
    _assert_model(got, ref, case, name)
    path = str(tmp_path / "poly_c005.yaml")
    binding.save_svm_file(path, got["sv"], got["rho"], kernel=binding.SVM_POLY2, alpha=got["alpha"])
    ctx.load_svm_file(path)
    keep, sums = ctx.classify_images(_packed(name))
    okeep, osums = O.classify_model(case["images"], ref["model"])
    assert np.array_equal(sums, osums) and np.array_equal(keep, okeep)
    assert 0 < int(keep.sum()) < keep.size
    # the file holds what was trained
    model = O.load_svm_model(path)
    assert model[0] == 1 and np.array_equal(model[1], ref["model"][1]) and np.array_equal(model[2], ref["model"][2])
    assert model[3] == ref["rho"]


# ---- agh_train_svm called directly: capacity and refusals ----------------------------------------------------------------
class _Raw:
    """agh_train_svm's arguments for one case, each replaceable; absent outputs go in as NULL"""

    def __init__(self, ctx, name, sv_cap=None):
        from agile_grasp_amd import binding

        self.ctx, self.case = ctx, CASES[name]
        self.lib = binding.load_library()
        self.packed = _packed(name)
        self.labels = np.ascontiguousarray(np.where(self.case["labels"] > 0, 1, -1), np.int8)
        self.n = len(self.labels)
        self.cap = self.n if sv_cap is None else sv_cap
        self.sv = np.full((max(self.cap, 1), 3528), np.nan, np.float32)
        self.alpha = np.full(max(self.cap, 1), np.nan, np.float64)
        self.n_sv, self.rho = C.c_int32(-7), C.c_double(np.nan)
        self.info = np.full(6, -7, np.int32)

    def call(self, **kw):
        from agile_grasp_amd.binding import _p

        case = self.case
        a = dict(images=_p(self.packed, C.c_uint32), labels=_p(self.labels, C.c_int8), n=self.n, kernel=case["kernel"],
                 C=case["C"], max_iter=case["max_iter"], eps=case["eps"], sv=_p(self.sv, C.c_float), sv_cap=self.cap,
                 alpha=_p(self.alpha, C.c_double), n_sv=C.byref(self.n_sv), rho=C.byref(self.rho),
                 info=_p(self.info, C.c_int32))
        a.update(kw)
        return self.lib.agh_train_svm(self.ctx._h, a["images"], a["labels"], C.c_int64(a["n"]), C.c_int32(a["kernel"]),
                                      C.c_double(a["C"]), C.c_int32(a["max_iter"]), C.c_double(a["eps"]), a["sv"],
                                      C.c_int64(a["sv_cap"]), a["alpha"], a["n_sv"], a["rho"], a["info"])

    def error(self):
        return self.lib.agh_last_error(self.ctx._h).decode()


def test_sv_cap_on_both_sides():
    from agile_grasp_amd import binding

    name = "limit50_poly2"
    case = CASES[name]
    _, ref = S.oracle(name)
    n_sv = ref["n_sv"]
    assert 1 < n_sv < len(case["labels"])
    ctx = _ctx()
    short = _Raw(ctx, name, sv_cap=n_sv - 1)
    assert short.call() == binding.AGH_ERR_CAPACITY
    assert short.n_sv.value == n_sv and f"{n_sv} support vectors, room for {n_sv - 1}" in short.error()
    assert list(short.info[:4]) == [ref["iterations"], n_sv, int((case["labels"] <= 0).sum()), int((case["labels"] > 0).sum())]
    assert short.info[4] + short.info[5] == 2 * ref["iterations"]
    assert short.rho.value == ref["rho"]  # (written before the count is known to be too large)
    assert np.isnan(short.sv).all() and np.isnan(short.alpha).all()  # nothing is copied into too small a buffer
    exact = _Raw(ctx, name, sv_cap=n_sv)
    assert exact.call() == 0
    assert exact.n_sv.value == n_sv and exact.rho.value == ref["rho"] and exact.info[0] == ref["iterations"]
    assert np.array_equal(exact.sv, ref["model"][1]) and np.array_equal(exact.alpha, ref["model"][2])
    _assert_model(_train(ctx, name), ref, case, "after a capacity error")
    # LINEAR writes one compacted vector whatever the count of support vectors
    lin = "limit50"
    one = _Raw(ctx, lin, sv_cap=1)
    assert one.call() == 0
    lref = S.oracle(lin)[1]
    assert one.n_sv.value == 1 and one.alpha[0] == 1.0 and one.info[1] == lref["n_sv"] > 1
    assert np.array_equal(one.sv[0], lref["w"]) and one.rho.value == lref["rho"]


REFUSALS = {
    "C_zero": (dict(C=0.0), "C > 0"),
    "C_negative": (dict(C=-1.0), "C > 0"),
    "C_nan": (dict(C=float("nan")), "C > 0"),
    "max_iter_negative": (dict(max_iter=-1), "max_iter >= 0"),
    "n_zero": (dict(n=0), "0 < n <= 2000000"),
    "n_too_large": (dict(n=2_000_001), "0 < n <= 2000000"),  # arguments only: refused before anything is read or allocated
    "kernel_unknown": (dict(kernel=2), "a supported kernel"),
    "sv_cap_zero": (dict(sv_cap=0), "sv_cap >= 1"),
    "no_images": (dict(images=None), "images"),
    "no_labels": (dict(labels=None), "labels"),
    "no_sv_out": (dict(sv=None), "the outputs"),
    "no_alpha_out": (dict(alpha=None), "the outputs"),
    "no_n_sv_out": (dict(n_sv=None), "the outputs"),
    "no_rho_out": (dict(rho=None), "the outputs"),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusals(which):
    from agile_grasp_amd import binding

    name = "limit49"
    kw, rule = REFUSALS[which]
    ctx = _ctx()
    raw = _Raw(ctx, name)
    assert raw.call(**kw) == binding.AGH_ERR_INVALID_ARGUMENT
    assert raw.error().startswith("agh_train_svm: need ") and rule in raw.error(), raw.error()
    assert raw.n_sv.value == -7 and (raw.info == -7).all() and np.isnan(raw.sv).all()  # nothing was written
    _assert_model(_train(ctx, name), S.oracle(name)[1], CASES[name], "after a refusal")


@pytest.mark.parametrize("label", [-1, 1])
def test_single_class_set_is_refused(label):
    from agile_grasp_amd import binding

    name = "limit49"
    ctx = _ctx()
    raw = _Raw(ctx, name)
    one_class = np.full(raw.n, label, np.int8)
    assert raw.call(labels=one_class.ctypes.data_as(C.POINTER(C.c_int8))) == binding.AGH_ERR_INVALID_ARGUMENT
    assert "single class" in raw.error()
    assert raw.n_sv.value == -7 and (raw.info == -7).all()
    with pytest.raises(binding.AghError, match="single class"):
        ctx.train_svm(_packed(name), one_class)
    _assert_model(_train(ctx, name), S.oracle(name)[1], CASES[name], "after a refusal")
    # info_out is optional
    assert raw.call(info=None) == 0 and raw.rho.value == S.oracle(name)[1]["rho"]
