"""What tests/svm_train_cases.py promises, on the CPU: every case sits in the regime it is named after (from the oracle's result
alone), the oracle's solver equals the independent numpy transcription bit for bit off C = 1 and off eps = FLT_EPSILON, and at
its fixed point it agrees with libsvm and with the KKT conditions of the dual at C = 0.05 and C = 20.  Descriptors and the
oracle's solves are computed once for the module (svm_train_cases.oracle)."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import ref_numpy as R
from tests import svm_train_cases as S
from tests.test_training import _toy_problem

CASES = S.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_sits_in_its_regime(name):
    case = CASES[name]
    _, res = S.oracle(name)
    got = S.regime(res, case["C"], case["max_iter"])
    assert case["expect"] or name.startswith("C"), "a case names its regime"
    for key, want in case["expect"].items():
        if key == "at_upper_min":
            assert got["at_upper"] >= want, (name, got)
        elif key == "rho":
            assert res["rho"] == want, (name, res["rho"])
        else:
            assert got[key] == want, (name, key, got)
    if got["at_lower"] == len(case["labels"]):  # nothing moved: rho is the midpoint of the two classes' untouched gradients
        assert res["rho"] == 0.0 and res["n_sv"] == 0


def test_small_C_puts_a_quarter_at_the_upper_bound_and_large_C_fewer_than_C_1():
    """The `C off 1` cases: LINEAR with C <= 0.05 ends with at least a quarter of the instances at the upper bound (the clip
    branches and the `status = 1` assignments act throughout), and every C = 20 case with fewer there than its C = 1 twin."""
    seen = 0
    for n in S.C_SIZES:
        for kernel, kname in ((S.LINEAR, "linear"), (S.POLY2, "poly2")):
            for C in S.C_OFF_ONE:
                name = f"C{C:g}_n{n}_{kname}"
                case = CASES[name]
                got = S.regime(S.oracle(name)[1], C, case["max_iter"])
                assert case["C"] == C and case["kernel"] == kernel and len(case["labels"]) == n and case["max_iter"] == 1000
                assert CASES[name + "_nostep"]["max_iter"] == 0
                if kernel == S.LINEAR and C <= 0.05:
                    assert 4 * got["at_upper"] >= n, (name, got)
                if C == 20.0:
                    twin = S.regime(S.solve(case, C_=1.0), 1.0, 1000)
                    assert got["at_upper"] < twin["at_upper"], (name, got, twin)
                seen += 1
    assert seen == 18


def test_stops_by_eps_under_a_huge_limit_and_at_step_zero():
    for kname in ("linear", "poly2"):
        zero = S.regime(S.oracle(f"eps2.5_{kname}")[1], 1.0, 1000)
        assert zero["iterations"] == 0 and zero["n_sv"] == 0 and zero["at_lower"] == 90 and zero["rho_branch"] == "bounds"
        assert zero["stopped_by"] == "eps"
    huge = [n for n, c in CASES.items() if c["max_iter"] == S.HUGE]
    assert len(huge) >= 4 + 4 + len(S.NATURAL_STOPS)
    for name in huge:
        its = S.oracle(name)[1]["iterations"]
        assert 0 < its < 1000, (name, its)  # stopped by the gap, and a short solve on the device
    assert {CASES[n]["eps"] for n in huge} >= {0.5, 0.1, 1e-3}
    assert {CASES[n]["C"] for n in huge if CASES[n]["eps"] == 1e-3} == {0.05, 1.0, 20.0}
    assert S.oracle("eps0.5_linear")[1]["iterations"] > S.oracle("eps2.5_linear")[1]["iterations"]
    assert S.oracle("eps0.1_linear")[1]["iterations"] > S.oracle("eps0.5_linear")[1]["iterations"]


def test_step_counts_on_both_sides_of_a_look():
    """svm_train copies the solver state back once per 50 steps: step limits and natural stops one short of a look, on it and
    one past it."""
    for max_iter in S.LOOK_LIMITS:
        res = S.oracle(f"limit{max_iter}")[1]
        assert res["iterations"] == max_iter
        assert S.solve(CASES[f"limit{max_iter}"], max_iter=S.HUGE)["iterations"] > max_iter  # the limit is what stopped it
    found = {}
    for steps, kernel, seed, eps in S.NATURAL_STOPS:
        kname = "linear" if kernel == S.LINEAR else "poly2"
        case = CASES[f"natural{steps}_{kname}"]
        assert case["max_iter"] == S.HUGE and case["eps"] == eps and case["kernel"] == kernel
        assert S.oracle(f"natural{steps}_{kname}")[1]["iterations"] == steps
        found.setdefault(kernel, set()).add(steps)
    assert found[S.LINEAR] >= {49, 50, 51} and found[S.POLY2] >= {49, 50, 51}
    # eps <= 0 can never stop a solve
    assert np.array_equal(S.oracle("eps0")[1]["alpha"], S.oracle("eps-1")[1]["alpha"])
    assert S.oracle("eps0")[1]["iterations"] == S.oracle("eps-1")[1]["iterations"] == 60


@pytest.mark.parametrize("name", sorted(S.TIE_SETS))
def test_first_tie_has_the_reversed_wave_order(name):
    """Step 0: every gradient is -1, both selections are ties over a whole class.  k_svm_select strides 1024 threads over n, so
    with the winner of the second selection at solver index n_neg >= 64 and a tied class-1 index in wave 0's part of a later
    stride, the lower index sits in the HIGHER wave (n = 2049: in the higher lane of wave 0): the arrangement no set of
    n <= 1024 instances gives."""
    n, n_neg = S.TIE_SETS[name]
    images, labels = S.tie_set(name)
    assert labels.shape == (n,) and int((labels < 0).sum()) == n_neg and n > 1024
    order = np.concatenate([np.nonzero(labels < 0)[0], np.nonzero(labels > 0)[0]])  # cvSortSamplesByClasses
    assert (order != np.arange(n)).mean() > 0.5  # scattered: the class sort moves most instances
    winner = n_neg  # solver index of the first class-1 instance
    tied = np.arange(n_neg + 1, n)  # the other class-1 instances, all with the same gradient
    wave = lambda k: (k % 1024) // 64
    if name == "n2049":  # the same reversal one level down: the winner is lane 1's second element, lane 0's third is tied
        assert (winner // 1024, winner % 1024) == (1, 1) and 2048 in tied and 2048 % 1024 == 0
    else:
        assert wave(winner) > 0 and (wave(tied) == 0).any(), "wave 0 holds a tied candidate with a higher index"
    if name == "n2100":
        assert winner == 1724 and winner % 1024 == 700 and set(range(2048, 2100)) <= set(tied[wave(tied) == 0])
    one = S.oracle(f"tie_{name}_onestep")[1]
    assert one["iterations"] == 1 and one["n_sv"] == 2
    pair = S.first_pair(labels)
    assert pair == (int(order[0]), int(order[n_neg]))
    assert list(np.nonzero(one["alpha"])[0]) == sorted(pair) and list(one["sv_order"]) == list(pair)
    assert one["alpha"][pair[0]] > 0 > one["alpha"][pair[1]] and one["alpha"][pair[0]] == -one["alpha"][pair[1]]


def _denominator(desc, i, j, poly):
    """Q_ii + Q_jj + 2 Q_ij of two instances with opposite labels (Q_ij = -K_ij), as the solver forms it in float, from the
    transcription's kernel row"""
    row = R._kernel_row(desc, i, poly)
    kjj = R._kernel_row(desc, j, poly)[j]
    return np.float32(np.float32(row[i] + kjj) - np.float32(2) * row[j])


def test_degenerate_sets_have_zero_denominators():
    # duplicates with opposite labels, and blanks
    for mixed in (False, True):
        images, labels = S.duplicates_and_blanks(mixed)
        desc = S.descriptors(images)
        assert np.array_equal(images[:10], images[10:20]) and np.array_equal(labels[:10], -labels[10:20])
        assert len({im.tobytes() for im in images[:10]}) == 10 and desc[:10].any(axis=1).all()
        assert not images[20:].any() and not desc[20:].any() and sorted(labels[20:]) == [-1, -1, 1, 1]
        for poly in (False, True):
            for k in range(10):
                assert _denominator(desc, k, 10 + k, poly) == 0 and R._kernel_row(desc, k, poly)[k] > 0
            assert _denominator(desc, 20, 21, poly) == 0 and R._kernel_row(desc, 20, poly)[20] == 0
    assert (S.duplicates_and_blanks()[1][:10] == 1).all() and len(set(S.duplicates_and_blanks(True)[1][:10])) == 2
    # a full image and a blank one: no gradient anywhere, both descriptors are zero
    case = CASES["full_blank_linear"]
    assert (case["images"][0] == 255).all() and not case["images"][1].any() and list(case["labels"]) == [1, -1]
    assert not S.descriptors(case["images"]).any()
    # images that differ only where no HOG window reads
    images, labels = S.unread_region_set()
    im = images.reshape(-1, 80, 100)
    assert len({x.tobytes() for x in images}) == len(images) == 12
    assert (im[:, :65, :97] == im[0, :65, :97]).all()  # the same wherever a window's gradient reads
    assert (im[:, 65:, :] != im[0, 65:, :]).any() and (im[:, :, 97:] != im[0, :, 97:]).any()
    desc = O.hog_many(images)
    assert desc[0].any() and all(np.array_equal(desc[0], d) for d in desc)
    assert _denominator(desc, 0, 1, False) == 0 and _denominator(desc, 0, 1, True) == 0
    assert list(labels[:4]) == [1, -1, 1, -1]
    # two instances at a small C: one step takes both to the bound
    assert len(CASES["n2_C0.001_linear"]["labels"]) == 2 and CASES["n2_C0.001_poly2"]["C"] == 1e-3
    # every such case: all alphas at C, none free, rho from the bounds branch with members at the upper bound
    names = [n for n in CASES if n.split("_")[0] in ("dup24", "dupmixed", "n2", "full", "unread") and "step" not in n]
    assert len(names) == 4 + 2 + 3 + 2 + 2 + 2
    for name in names:
        case = CASES[name]
        got = S.regime(S.oracle(name)[1], case["C"], case["max_iter"])
        n = len(case["labels"])
        assert got["at_upper"] == n and got["free"] == 0 and got["rho_branch"] == "bounds" and got["stopped_by"] == "eps", name
        assert (np.abs(S.oracle(name)[1]["alpha"]) == case["C"]).all()
    assert {CASES[n]["C"] for n in names if n.startswith("dup24")} == {1.0, 0.25, 1e8}
    # C = 1e8: the clamped step is not clipped, its size is the clamp's: 2 / FLT_EPSILON = 2^24 per step on the first pair
    for name, steps in (("dup24_C1e8_onestep", 1), ("dup24_C1e8_fivesteps", 5)):
        a = S.oracle(name)[1]["alpha"]
        assert list(np.nonzero(a)[0]) == [0, 10] and a[10] == steps * 2.0 ** 24 == -a[0] and steps * 2.0 ** 24 < 1e8
    assert 6 * 2.0 ** 24 > 1e8 and S.oracle("dup24_C1e8_linear")[1]["iterations"] == 6 * 12
    # the bounds branch with upper-bound members beside lower-bound ones, under a step limit
    got = S.regime(S.oracle("tie_n2100_C0.02")[1], 0.02, 200)
    assert got["rho_branch"] == "bounds" and got["at_upper"] >= 200 and got["at_lower"] >= 200


def test_one_instance_classes():
    for tag, which in (("one_positive", 1), ("one_negative", -1)):
        for kname in ("linear", "poly2"):
            case = CASES[f"{tag}_{kname}"]
            assert int((case["labels"] == which).sum()) == 1 and len(case["labels"]) == 90 and case["C"] == 0.05
            res = S.oracle(f"{tag}_{kname}")[1]
            assert 0 < res["iterations"] < 1000 and res["alpha"][case["labels"] == which][0] != 0
            assert abs(res["alpha"].sum()) < 1e-12  # the lone instance balances all its opponents


TRANSCRIBED = sorted(n for n, c in CASES.items() if len(c["labels"]) <= 257)


@pytest.mark.parametrize("name", TRANSCRIBED)
def test_oracle_matches_transcription(name):
    """Bit for bit, for every case of at most 257 instances.  The transcription is a Python loop over n per step: above 100
    instances both run under a limit of 250 steps (the oracle again, at the same limit)."""
    case = CASES[name]
    desc = S.descriptors(case["images"])
    max_iter = case["max_iter"] if len(case["labels"]) <= 100 else min(case["max_iter"], 250)
    a = S.oracle(name)[1] if max_iter == case["max_iter"] else S.solve(case, max_iter=max_iter)
    b = R.train_svm(desc, case["labels"], C=case["C"], max_iter=max_iter, eps=case["eps"], poly=bool(case["kernel"]))
    assert a["iterations"] == b["iterations"] and a["n_sv"] == b["n_sv"]
    assert np.array_equal(a["alpha"], b["alpha"]) and np.array_equal(a["sv_order"], b["sv_order"])
    assert a["rho"] == b["rho"]
    if case["kernel"] == S.LINEAR:
        assert np.array_equal(a["w"], b["w"])


@pytest.mark.parametrize("kernel", [S.LINEAR, S.POLY2])
@pytest.mark.parametrize("C", [0.05, 20.0])
def test_oracle_solver_fixed_point_matches_libsvm_off_C_1(C, kernel):
    """test_training.test_oracle_solver_fixed_point_matches_libsvm with C off 1, at that test's own bounds."""
    from sklearn.svm import SVC

    X, y = _toy_problem(400, 11, overlap=0.6)
    r = O.train_svm(X, y, C_=C, max_iter=400000, eps=1e-6, kernel=kernel)
    assert 0 < r["iterations"] < 400000
    kw = dict(kernel="linear") if kernel == 0 else dict(kernel="poly", degree=2, gamma=1.0, coef0=0.0)
    m = SVC(C=C, tol=1e-6, shrinking=False, cache_size=500, **kw).fit(X.astype(np.float64), y)
    Xd = X.astype(np.float64)
    K = Xd @ Xd.T if kernel == 0 else (Xd @ Xd.T) ** 2
    dec_orc = K @ r["alpha"] - r["rho"]              # CvSVM::predict: sum > 0 <=> label -1
    dec_lib = m.decision_function(Xd)                # libsvm: > 0 <=> label +1
    al = np.zeros(len(y))
    al[m.support_] = m.dual_coef_[0]                 # y_i alpha_i
    print(f"C = {C}, kernel = {kernel}: {r['iterations']} steps, |d alpha| <= {np.abs(al + r['alpha']).max():.3g}, "
          f"|d rho| = {abs(m.intercept_[0] - r['rho']):.3g}, |d dec| <= {np.abs(dec_lib + dec_orc).max():.3g}")
    assert np.abs(dec_lib + dec_orc).max() < 2e-5
    assert np.array_equal(np.sign(dec_lib), -np.sign(dec_orc))
    assert np.abs(al + r["alpha"]).max() < 1e-5 and abs(m.intercept_[0] - r["rho"]) < 1e-5
    assert set(np.nonzero(np.abs(r["alpha"]) > 1e-9)[0]) == set(m.support_.tolist())
    if C < 1:
        assert np.abs(r["alpha"]).max() == C  # the box binds (at C = 20 no alpha of this problem reaches it)


@pytest.mark.parametrize("C", [0.05, 20.0])
def test_oracle_solver_satisfies_kkt_off_C_1(C):
    """test_training.test_oracle_solver_satisfies_kkt_when_run_to_convergence with the box |a| <= C."""
    X, y = _toy_problem(400, 11, overlap=0.6)
    r = O.train_svm(X, y, C_=C, max_iter=200000, eps=1e-4)
    assert r["iterations"] < 200000
    a = r["alpha"]  # signed: alpha * y_solver, y_solver = +1 for label -1
    ys = np.where(y > 0, -1.0, 1.0)
    assert np.all(a * ys >= 0) and np.all(np.abs(a) <= C) and abs(a.sum()) < 1e-9  # box + equality constraint
    dec = X.astype(np.float64) @ (X.astype(np.float64).T @ a) - r["rho"]
    m = ys * dec  # functional margin
    tol = 2e-3
    free = (np.abs(a) > 0) & (np.abs(a) < C)
    at_c = np.abs(a) == C
    assert free.any() and (at_c.any() if C < 1 else (a == 0).any())  # (C = 0.05: no alpha is 0; C = 20: none is at C)
    assert np.all(np.abs(m[free] - 1) < tol)
    assert np.all(m[a == 0] > 1 - tol) and np.all(m[at_c] < 1 + tol)
    dec_w = X.astype(np.float64) @ r["w"].astype(np.float64) - r["rho"]
    assert np.abs(dec_w - dec).max() < 1e-4
