"""Training sets and solver parameters that put CvSVM::train's HIP path (k_svm_init, k_svm_select, k_svm_update, k_svm_compress,
k_svm_gather and the host loop of svm_train; csrc/train.hip) off the defaults that Learning::convertData leaves it at (numpy
only).  tests/test_svm_train_cases.py proves on the CPU that each case sits in the regime it is named after,
tests/test_gpu_svm_train.py runs every case on the device against the oracle, bit for bit.

A case is a dict(images (n, 8000) uint8, labels (n,) of -1 / +1, kernel, C, eps, max_iter, expect).  `expect` names the
regime: keys of regime() with the value the oracle's result must give, `at_upper_min` (a lower bound on the count of
instances at the upper bound) or `rho`.  Building the cases computes no descriptor and runs no solver.

  stroke_images      the "few random strokes" generator of test_training.test_solver_sizes_around_the_tile_boundaries
  stroke_set         images and labels as that test draws them from one seed
  regime             which regime a solve was in, from the oracle's result alone
  cases()            name -> case, built once
  oracle(name)       (descriptors, oracle_py.train_svm's result) of a case, computed once per process for both test files

Not among the cases: CvSVMKernel::calc's clamp to FLT_MAX * 1e-3.  A HOG block is L2-Hys normalised, so a descriptor's 98
blocks have norm about 1 at most, K(x, x') <= 98 and K^2 < 1e4: no image reaches the clamp in training.  (Prediction reaches
it with scaled support vectors: tests/svm_model_cases.clamp_models.)
"""
import functools

import numpy as np

LINEAR, POLY2 = 0, 1
FLT_EPSILON = 1.1920928955078125e-07
HUGE = 1_000_000  # a step limit no case reaches: "train to convergence"


def stroke_images(n, rng):
    """(n, 80, 100) uint8 images, 0 / 255: a few random strokes each, descriptors with many exact zeros, like real grasp
    images.  Draws from `rng`, so a caller's later draws follow on."""
    images = np.zeros((n, 80, 100), np.uint8)
    for im in images:
        for _ in range(int(rng.integers(1, 6))):
            r, c = int(rng.integers(0, 80)), int(rng.integers(0, 100))
            im[r:r + int(rng.integers(1, 30)), c:c + int(rng.integers(1, 4))] = 255
    return images


def stroke_set(n, seed=None):
    """(images (n, 8000), labels): about 40 % positives, image 0 positive and image 1 negative; the seed defaults to n."""
    rng = np.random.default_rng(n if seed is None else seed)
    images = stroke_images(n, rng)
    labels = np.where(rng.random(n) < 0.4, 1, -1)
    labels[0], labels[1] = 1, -1
    return images.reshape(n, 8000), labels


def regime(result, C, max_iter):
    """The regime of a solve, from oracle_py.train_svm's result (signed alphas in input order, step count) alone.
    An update that clips sets alpha to C itself, so `== C` is exact."""
    a = np.abs(result["alpha"])
    at_upper, at_lower = int((a == C).sum()), int((a == 0).sum())
    free = a.size - at_upper - at_lower
    assert ((a == 0) | (a == C) | ((a > 0) & (a < C))).all()
    return {"at_upper": at_upper, "free": free, "at_lower": at_lower, "iterations": result["iterations"],
            "n_sv": result["n_sv"], "stopped_by": "eps" if result["iterations"] < max_iter else "max_iter",
            "rho_branch": "free" if free > 0 else "bounds"}


def first_pair(labels):
    """The pair of the first step: every gradient is -1, so both arg-max reductions are ties and the lowest solver index of
    each class wins.  Solver order is label -1 first (cvSortSamplesByClasses); returned as input indices."""
    labels = np.asarray(labels)
    return int(np.nonzero(labels <= 0)[0][0]), int(np.nonzero(labels > 0)[0][0])


def _case(images, labels, kernel=LINEAR, C=1.0, eps=FLT_EPSILON, max_iter=1000, **expect):
    images = np.ascontiguousarray(images, np.uint8).reshape(-1, 8000)
    labels = np.asarray(labels).astype(np.int64)
    assert images.shape[0] == labels.shape[0] and set(np.unique(labels)) == {-1, 1}
    return {"images": images, "labels": labels, "kernel": kernel, "C": C, "eps": eps, "max_iter": max_iter, "expect": expect}


# ---- the sets ---------------------------------------------------------------------------------------------------------
C_OFF_ONE = (0.002, 0.05, 20.0)
C_SIZES = (65, 257, 600)
# the seed of each size's stroke_set.  65 instances take seed 5: with seed 65, the set of test_training, POLY2 leaves two
# instances at the upper bound at C = 1 and at C = 20 alike, which would say nothing about C.
C_SEEDS = {65: 5, 257: 257, 600: 600}
LOOK_LIMITS = (49, 50, 51, 99, 100, 101)  # svm_train looks at the stop flag once per 50 steps

# Natural stops (gap < eps under a step limit that is never reached) after exactly 49, 50 and 51 steps: one step short of the
# host loop's first look, on it, and one past it.  Found on the CPU with the oracle: for stroke_set(90, seed), seed = 0, 1, ...
# and both kernels, the eps at which the step count first drops to the target (the count is a non-increasing step function of
# eps; a target is reachable where the gap of that step is a new minimum).  Seeds 0 .. 21 gave every target for both
# kernels, and a stop on the second look (100 steps) as well; tests/test_svm_train_cases.py asserts each count.
# (steps, kernel, seed, eps)
NATURAL_STOPS = ((49, LINEAR, 3, 1.81), (50, LINEAR, 15, 1.64), (51, LINEAR, 21, 1.92), (100, LINEAR, 0, 0.9843),
                 (49, POLY2, 1, 1.8), (50, POLY2, 0, 1.731), (51, POLY2, 0, 1.7), (100, POLY2, 1, 0.8))

TIE_SETS = {"n2100": (2100, 1724), "n1025": (1025, 400), "n2049": (2049, 1025)}  # name -> (n, instances of label -1)


def tie_set(name):
    """Stroke images with a fixed count of label -1, scattered over the input order (so that agh_train_svm's class sort moves
    nearly every instance).  In solver order the first class-1 instance is index n_neg: with n_neg >= 1024 or n > 1024 that is
    some thread's second element of k_svm_select's stride, while wave 0 holds tied class-1 indices from the last stride
    (2048 .. n - 1, or 1024)."""
    n, n_neg = TIE_SETS[name]
    rng = np.random.default_rng(n)
    images = stroke_images(n, rng).reshape(n, 8000)
    labels = np.ones(n, np.int64)
    labels[rng.permutation(n)[:n_neg]] = -1
    return images, labels


def duplicates_and_blanks(mixed=False):
    """10 stroke images, the same 10 again with the opposite labels, and 4 blank images (2 + 2).  A duplicate pair has
    Q_ii + Q_jj + 2 Q_ij = 0 exactly (Q_ij = -K(x, x)): the clamp's FLT_EPSILON is the denominator, the step is 2 / FLT_EPSILON
    and both alphas clip to C.  A blank pair has Kdiag = 0 and a zero kernel row, with the same outcome.
    Plain: the first ten are all positive, so the k-th instance of either class is the other's duplicate; a step's two
    gradient terms cancel exactly (Q_j = -Q_i), every gradient stays -1 and the solve pairs the duplicates off in order: 10 + 2
    steps.  Mixed: random labels on the first ten, so that duplicates meet after other steps have moved the gradient."""
    images, labels = stroke_set(10, 1000)  # (ten distinct non-zero descriptors)
    if not mixed:
        labels = np.ones(10, np.int64)
    blank = np.zeros((4, 8000), np.uint8)
    return np.concatenate([images, images, blank]), np.concatenate([labels, -labels, [1, -1, 1, -1]])


def unread_region_set(n=12, seed=77):
    """One stroke image n times, each copy with random pixels of its own in rows 65 .. 79 and in columns 97 .. 99 only.
    Learning's HOGDescriptor takes 64 x 64 windows at a stride of 32 from the 80 x 100 image: two windows, at columns 0 and 32
    of row 0.  They cover rows 0 .. 63 and columns 0 .. 95, and a gradient reads one pixel further: rows <= 64, columns <= 96.
    So the images differ and their descriptors do not (tests/test_svm_train_cases.py asserts both).  Labels alternate: every
    pair of opposite labels has a zero denominator with Kdiag > 0."""
    rng = np.random.default_rng(seed)
    base = stroke_images(1, rng)[0]
    unread = np.zeros((80, 100), bool)
    unread[65:, :] = True
    unread[:, 97:] = True
    images = np.repeat(base[None], n, axis=0)
    for k, im in enumerate(images):
        im[unread] = (rng.random(int(unread.sum())) < 0.5) * 255
        im[65 + k, 0], im[79, 1 + k] = 255, 0  # (no two alike, whatever the draw)
    return images.reshape(n, 8000), np.where(np.arange(n) % 2 == 0, 1, -1)


def one_instance_class(which):
    """90 stroke images with exactly one positive (which = +1) or exactly one negative (which = -1), in the middle."""
    images, _ = stroke_set(90)
    labels = np.full(90, -which, np.int64)
    labels[44] = which
    return images, labels


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    kname = {LINEAR: "linear", POLY2: "poly2"}

    # C off 1: the eight clip branches and both status lines of k_svm_select see a C that is not 1
    for n in C_SIZES:
        images, labels = stroke_set(n, C_SEEDS[n])
        for C in C_OFF_ONE:
            for kernel in (LINEAR, POLY2):
                expect = {}
                if kernel == LINEAR and C <= 0.05:
                    expect["at_upper_min"] = -(-n // 4)  # at least a quarter at the upper bound
                out[f"C{C:g}_n{n}_{kname[kernel]}"] = _case(images, labels, kernel, C, max_iter=1000, **expect)
                out[f"C{C:g}_n{n}_{kname[kernel]}_nostep"] = _case(images, labels, kernel, C, max_iter=0, iterations=0,
                                                                  n_sv=0, at_lower=n, rho_branch="bounds")

    # eps off FLT_EPSILON
    images, labels = stroke_set(90)
    for kernel in (LINEAR, POLY2):
        out[f"eps2.5_{kname[kernel]}"] = _case(images, labels, kernel, eps=2.5, max_iter=1000, iterations=0, n_sv=0,
                                               at_lower=90, rho_branch="bounds", stopped_by="eps")
        for eps in (0.5, 0.1):
            out[f"eps{eps:g}_{kname[kernel]}"] = _case(images, labels, kernel, eps=eps, max_iter=HUGE, stopped_by="eps")
    for C in (0.05, 1.0, 20.0):
        out[f"eps0.001_C{C:g}"] = _case(images, labels, LINEAR, C, eps=1e-3, max_iter=HUGE, stopped_by="eps")
    out["eps0.001_C0.05_poly2"] = _case(images, labels, POLY2, 0.05, eps=1e-3, max_iter=HUGE, stopped_by="eps")
    for eps in (0.0, -1.0):  # accepted: the gap test can never fire
        out[f"eps{eps:g}"] = _case(images, labels, LINEAR, eps=eps, max_iter=60, iterations=60, stopped_by="max_iter")

    # the host loop's looks, from the step limit's side ...
    for max_iter in LOOK_LIMITS:
        out[f"limit{max_iter}"] = _case(images, labels, LINEAR, max_iter=max_iter, iterations=max_iter, stopped_by="max_iter")
    out["limit50_poly2"] = _case(images, labels, POLY2, max_iter=50, iterations=50, stopped_by="max_iter")
    # ... and from the gap's
    for steps, kernel, seed, eps in NATURAL_STOPS:
        im, lab = stroke_set(90, seed)
        out[f"natural{steps}_{kname[kernel]}"] = _case(im, lab, kernel, eps=eps, max_iter=HUGE, iterations=steps,
                                                       stopped_by="eps")

    # ties across strides and waves
    for name in TIE_SETS:
        im, lab = tie_set(name)
        out[f"tie_{name}_onestep"] = _case(im, lab, LINEAR, max_iter=1, iterations=1, n_sv=2)
        out[f"tie_{name}"] = _case(im, lab, LINEAR, max_iter=200, iterations=200)
    im, lab = tie_set("n2100")
    out["tie_n2100_C0.02"] = _case(im, lab, LINEAR, 0.02, max_iter=200, iterations=200, at_upper_min=2100 // 8)
    out["tie_n2100_poly2"] = _case(im, lab, POLY2, max_iter=200, iterations=200)

    # degenerate sets: all of them end with every alpha at C, none free, rho from the bounds branch
    im, lab = duplicates_and_blanks()
    for C in (1.0, 0.25):
        for kernel in (LINEAR, POLY2):
            out[f"dup24_C{C:g}_{kname[kernel]}"] = _case(im, lab, kernel, C, at_upper=24, free=0, rho_branch="bounds",
                                                        stopped_by="eps", iterations=12, rho=0.0)
    im, lab = duplicates_and_blanks(mixed=True)
    for C, kernel, steps in ((1.0, LINEAR, 64), (0.25, LINEAR, 28), (0.25, POLY2, 465)):
        out[f"dupmixed_C{C:g}_{kname[kernel]}"] = _case(im, lab, kernel, C, at_upper=24, free=0, rho_branch="bounds",
                                                        stopped_by="eps", iterations=steps)
    im2, lab2 = stroke_set(2)
    for kernel in (LINEAR, POLY2):
        out[f"n2_C0.001_{kname[kernel]}"] = _case(im2, lab2, kernel, 1e-3, at_upper=2, free=0, rho_branch="bounds",
                                                  stopped_by="eps", iterations=1)
    full_blank = np.stack([np.full(8000, 255, np.uint8), np.zeros(8000, np.uint8)])
    for kernel in (LINEAR, POLY2):  # both descriptors are zero: Kdiag = 0, the denominator is the clamp's FLT_EPSILON
        out[f"full_blank_{kname[kernel]}"] = _case(full_blank, [1, -1], kernel, at_upper=2, free=0, rho_branch="bounds",
                                                   stopped_by="eps", iterations=1)
    im, lab = unread_region_set()
    for kernel in (LINEAR, POLY2):
        out[f"unread_{kname[kernel]}"] = _case(im, lab, kernel, at_upper=12, free=0, rho_branch="bounds", stopped_by="eps",
                                               iterations=6)
    # The clamp's value itself.  At C <= 1 a clamped step (2 / FLT_EPSILON = 2^24) is clipped to C, whatever the clamp is; at
    # C = 1e8 it is not: a duplicate pair gains exactly 2^24 per step, its gradient terms cancel, the same pair is picked
    # again, and the sixth step clips it to C (6 x 2^24 > 1e8).  24 instances: 12 pairs, 72 steps.
    # (Only the opposite-label denominator can be clamped with a non-zero numerator: two instances of one class whose kernel
    # rows coincide have the same gradient, so Gi - Gj = 0 and the step is zero with any denominator.)
    im, lab = duplicates_and_blanks()
    for kernel in (LINEAR, POLY2):
        out[f"dup24_C1e8_{kname[kernel]}"] = _case(im, lab, kernel, 1e8, at_upper=24, free=0, rho_branch="bounds",
                                                   stopped_by="eps", iterations=72, rho=0.0)
    out["dup24_C1e8_onestep"] = _case(im, lab, LINEAR, 1e8, max_iter=1, iterations=1, free=2, at_lower=22, at_upper=0)
    out["dup24_C1e8_fivesteps"] = _case(im, lab, POLY2, 1e8, max_iter=5, iterations=5, free=2, at_lower=22, at_upper=0)

    # one-instance classes
    for which, tag in ((1, "one_positive"), (-1, "one_negative")):
        im, lab = one_instance_class(which)
        for kernel in (LINEAR, POLY2):
            out[f"{tag}_{kname[kernel]}"] = _case(im, lab, kernel, 0.05, stopped_by="eps")
    return out


_DESCRIPTORS = {}


def descriptors(images):
    """oracle_py.hog_many(images), once per distinct image set (several cases share one)."""
    import hashlib

    from oracle import oracle_py as O

    key = (images.shape, hashlib.sha1(images.tobytes()).hexdigest())
    if key not in _DESCRIPTORS:
        _DESCRIPTORS[key] = O.hog_many(images)
    return _DESCRIPTORS[key]


def solve(case, **override):
    """oracle_py.train_svm on a case, with parameters replaced by `override` (C_, eps, max_iter, kernel)."""
    from oracle import oracle_py as O

    kw = dict(C_=case["C"], eps=case["eps"], max_iter=case["max_iter"], kernel=case["kernel"])
    kw.update(override)
    return O.train_svm(descriptors(case["images"]), case["labels"], **kw)


@functools.lru_cache(maxsize=None)
def oracle(name):
    case = cases()[name]
    return descriptors(case["images"]), solve(case)
