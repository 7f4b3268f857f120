"""Query images and general SVM models (several support vectors, alpha != 1, LINEAR or POLY degree 2) that put CvSVM::predict's
HIP path (k_svm_transpose at load, k_svm_kvals, k_svm_decide; csrc/train.hip) on the counts where it changes behaviour (numpy
only).  tests/test_svm_model_cases.py proves on the CPU what the cases promise, tests/test_gpu_svm_predict.py runs them.

A model is the tuple (kernel, sv, alpha, rho) that oracle_py.classify_model and ref_numpy.classify_model take.  This module
computes no HOG descriptor: the caller passes in the descriptors of query_images() and sv_images().

  N_SV          support-vector counts: the decide kernel's 16-wide chain and its tail (1, 2, 15 / 16 / 17), the transpose's 32 x 32
                tiles (31 / 32 / 33), the 64-vector tile and the clamp of wave_tile (63 / 64 / 65), the 256-thread work-group of
                k_svm_kvals (255 / 256 / 257) and a third column of work-groups (513)
  N_IMAGES      image counts: k_svm_kvals' two hypotheses per work-group (1, 2, 3), k_svm_decide's 64 per work-group (63 / 64 /
                65), agh_classify_images' first capacity (1024 / 1025)
  SPLIT_COUNT   the smallest count that takes a second k_svm_kvals launch (gridDim.y = 65535 pairs): a lone odd hypothesis
  query_images  the mix below plus one blank and one full image
  sv_images     the pool whose first n_sv images are a model's support vectors
  model         alpha non-dyadic in (-1, 1), rho the median decision value: the labels split evenly, values sit on the threshold
  clamp_models  kernel values above CvSVMKernel::calc's clamp, with POLY2 by way of a square that overflows float
"""
import numpy as np

from tests import ref_numpy as R

LINEAR, POLY2 = 0, 1
N_SV = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)
N_IMAGES = (1, 2, 3, 63, 64, 65, 1024, 1025)
SPLIT_COUNT = 131071
N_QUERY = 131  # odd, and more than two work-groups of k_svm_decide
BLANK, FULL = 7, 8  # their places among the query images (both descriptors are zero: every gradient is)

# clamp_models: the factor on the LINEAR model's rows, chosen on the CPU from the transcription's values.  Over the 131 query
# images, the largest unscaled float dot of a query with the three support vectors is 49.2 .. 97.5 on the 65 dense queries and
# 0 .. 29.9 on the 66 others (64 stroke images, the blank and the full one).  With 9e33 the kernel value passes
# FLT_MAX * 1e-3 = 3.4e35 for some support vector on CLAMP_LINEAR_COUNTS[0] = 65 queries (4.4e35 at least) and for none on
# CLAMP_LINEAR_COUNTS[1] = 66 (2.7e35 at most); no dot passes 8.8e35 and no scaled entry 6.8e33: everything stays finite.
# tests/test_svm_model_cases.py holds the two counts to what the transcription gives.
CLAMP_LINEAR_SCALE = np.float32(9e33)
CLAMP_LINEAR_COUNTS = (65, 66)
CLAMP_POLY_SCALE = np.float32(1e18)


def _mixed(n, seed, pure):
    """(n, 8000) uint8 images, 0 / 255.  Every second one a few random strokes, as real grasp images are (a descriptor that is
    mostly exact zeros); the others dense: half-density noise (no group of four descriptor entries is zero) and 1100-stripes in x
    or in y
    (with `pure` the first of each kind as it is, all others with 0.5 to 5 % of the pixels flipped and a phase of their own)."""
    rng = np.random.default_rng(seed)
    images = np.zeros((n, 80, 100), np.uint8)
    for i, im in enumerate(images):
        kind = i % 6
        if kind % 2 == 1:
            for _ in range(int(rng.integers(1, 6))):
                r, c = int(rng.integers(0, 80)), int(rng.integers(0, 100))
                im[r:r + int(rng.integers(1, 30)), c:c + int(rng.integers(1, 4))] = 255
        elif kind == 0:
            im[:] = (rng.random((80, 100)) < 0.5) * 255
        else:
            phase = 0 if pure and i < 6 else int(rng.integers(0, 4))
            flip = 0.0 if pure and i < 6 else float(rng.uniform(0.005, 0.05))
            if kind == 2:
                im[:, ((np.arange(100) + phase) % 4) < 2] = 255
            else:
                im[((np.arange(80) + phase) % 4) < 2, :] = 255
            im ^= ((rng.random((80, 100)) < flip) * 255).astype(np.uint8)
    return images.reshape(n, 8000)


def query_images(n=N_QUERY, seed=20):
    """The first n of the mix; from n = 9 on, image BLANK is blank and image FULL is full."""
    images = _mixed(n, seed, True)
    if n > FULL:
        images[BLANK] = 0
        images[FULL] = 255
    return images


def sv_images(n=max(N_SV), seed=21):
    """The pool of support-vector images (a dense one first: a one-vector model then has no ties at zero)."""
    return _mixed(n, seed, False)


def model(n_sv, kernel, seed, sv_desc, query_desc):
    """The first n_sv rows of `sv_desc` as support vectors, alpha from rng.uniform(-1, 1) (non-dyadic: a reordered sum changes
    bits), rho the median of the transcription's decision values of `query_desc` at rho = 0."""
    sv = np.ascontiguousarray(sv_desc[:n_sv], np.float32)
    assert sv.shape == (n_sv, 3528)
    alpha = np.random.default_rng(seed).uniform(-1.0, 1.0, n_sv)
    _, sums = R.svm_decide(_kernel_values(query_desc, kernel, sv_desc)[:, :n_sv], alpha, 0.0)
    return kernel, sv, alpha, float(np.median(sums))


_KVALS = {}


def _kernel_values(query_desc, kernel, sv_desc):
    """Kernel values of the whole pool, computed once per (queries, pool, kernel): a value depends on its own support vector
    alone, so the first n_sv columns are what an n_sv-vector model gives."""
    key = (id(query_desc), id(sv_desc), kernel)
    hit = _KVALS.get(key)
    if hit is None or hit[0] is not query_desc or hit[1] is not sv_desc:
        hit = _KVALS[key] = (query_desc, sv_desc, R.svm_kernel_values(query_desc, kernel, sv_desc))
    return hit[2]


def model_seed(n_sv, kernel):
    return 1000 * (kernel + 1) + n_sv


def clamp_models(sv):
    """Two models on the first three rows of `sv` (descriptors: no negative entry), rows scaled by a positive factor, so no
    inf - inf can arise.  POLY2: dots around 1e19, the square overflows float to inf and clamps.  LINEAR: the dot itself is
    finite and above the clamp for the dense queries, below it for the sparse ones.  A blank query gives 0 in both.
    rho = a quarter of the clamp: a fully clamped query (alpha sums to 0.85) is dropped, a blank one kept."""
    sv = np.ascontiguousarray(sv[:3], np.float32)
    assert sv.shape == (3, 3528) and (sv >= 0).all()
    alpha = np.array([0.7, -0.3, 0.45])
    rho = 0.25 * float(R.SVM_MAX_VAL)
    return ((POLY2, sv * CLAMP_POLY_SCALE, alpha, rho), (LINEAR, sv * CLAMP_LINEAR_SCALE, alpha, rho))
