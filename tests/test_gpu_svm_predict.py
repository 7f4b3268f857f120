"""CvSVM::predict with a general model (k_svm_transpose at load, k_svm_kvals, k_svm_decide; csrc/train.hip) and the general
branch of agh_classify_images (csrc/hog_svm.hip), at the support-vector and image counts where they change behaviour, against
the oracle with exact equality on the labels and on the float64 decision values.

The cases come from tests/svm_model_cases.py; tests/test_svm_model_cases.py checks them on the CPU, the oracle against an
independent numpy transcription included.  The descriptors behind the models and the oracle's values of the 131 query images
are computed once for the module."""
import functools
import time

import numpy as np
import pytest

from tests import svm_model_cases as S

pytestmark = pytest.mark.gpu


def _ctx():
    from agile_grasp_amd import binding, synthetic

    return binding.Context(synthetic.camera_origins())


@functools.lru_cache(maxsize=None)
def _data():
    """query images, their packed words, their descriptors, the descriptors of the support-vector pool (all from the oracle)"""
    from agile_grasp_amd import binding
    from oracle import oracle_py as O

    images = S.query_images()
    return images, binding.pack_images(images), O.hog_many(images), O.hog_many(S.sv_images())


@functools.lru_cache(maxsize=None)
def _case(n_sv, kernel):
    """(model, oracle labels, oracle decision values) over the 131 query images"""
    from oracle import oracle_py as O

    images, _, desc, pool = _data()
    model = S.model(n_sv, kernel, S.model_seed(n_sv, kernel), pool, desc)
    keep, sums = O.classify_model(images, model)
    assert 0.25 * S.N_QUERY <= int(keep.sum()) <= 0.75 * S.N_QUERY
    return model, keep, sums


def _take(a, n):
    """the first n of `a` repeated: how the larger image counts are made, and what they must give"""
    return a[:n] if n <= len(a) else np.tile(a, (-(-n // len(a)),) + (1,) * (a.ndim - 1))[:n]


def _assert_equal(got, keep, sums, what=""):
    assert got[0].dtype == np.uint8 and got[1].dtype == np.float64
    assert np.array_equal(got[1], sums), (what, np.nonzero(got[1] != sums)[0][:8])
    assert np.array_equal(got[0], keep), (what, np.nonzero(got[0] != keep)[0][:8])


@pytest.mark.parametrize("kernel", [S.LINEAR, S.POLY2])
@pytest.mark.parametrize("n_sv", S.N_SV)
def test_support_vector_counts(n_sv, kernel):
    """The decide kernel's 16-wide chain and its tail, the transpose's 32 x 32 tiles, the 64-vector tile with wave_tile's
    clamp, one to three columns of k_svm_kvals work-groups; 131 images: an odd last pair, three decide work-groups.  The
    second call reuses every buffer."""
    model, keep, sums = _case(n_sv, kernel)
    packed = _data()[1]
    ctx = _ctx()
    ctx.load_svm_model(*model)
    for call in range(2):
        _assert_equal(ctx.classify_images(packed), keep, sums, call)


@pytest.mark.parametrize("n", S.N_IMAGES)
def test_image_counts(n):
    """One, two, three hypotheses (the odd last one pairs with itself), 63 / 64 / 65 (the decide work-group), 1024 / 1025
    (the first capacity of agh_classify_images' buffers); and none at all."""
    packed = _take(_data()[1], n)
    ctx = _ctx()
    for n_sv, kernel in ((65, S.POLY2), (17, S.LINEAR)):
        model, keep, sums = _case(n_sv, kernel)
        ctx.load_svm_model(*model)
        _assert_equal(ctx.classify_images(packed), _take(keep, n), _take(sums, n), (n_sv, kernel))
        none = ctx.classify_images(np.zeros((0, 250), "<u4"))
        assert none[0].shape == (0,) and none[1].shape == (0,)
        _assert_equal(ctx.classify_images(packed), _take(keep, n), _take(sums, n), (n_sv, kernel, "again"))


def test_second_kvals_launch():
    """131 071 images: 65 535 pairs in the first k_svm_kvals launch, and a second launch of one odd hypothesis at
    h_base = 131 070.  64 distinct images, tiled as packed words (131 MB); the oracle's 64 values tile the same way."""
    model, keep, sums = _case(2, S.POLY2)
    n = S.SPLIT_COUNT
    packed = _take(np.ascontiguousarray(_data()[1][:64]), n)
    assert packed.shape == (n, 250)
    keep, sums = _take(keep[:64], n), _take(sums[:64], n)
    assert 0 < keep[:64].sum() < 64
    ctx = _ctx()
    ctx.load_svm_model(*model)
    t0 = time.perf_counter()
    got = ctx.classify_images(packed)
    print(f"classify_images({n} images, n_sv = 2, POLY2): {time.perf_counter() - t0:.3f} s")
    # the last pair of the first launch, and the lone hypothesis of the second
    for h in (n - 3, n - 2, n - 1):
        assert got[1][h] == sums[h] and got[0][h] == keep[h], h
    _assert_equal(got, keep, sums)


def test_buffers_across_model_and_count_changes(svm_model):
    """One context: the descriptor and kernel-value buffers grow on demand and are kept across model changes; cap * n_sv
    shrinks while n grows, then grows; the compacted vector takes the fused path in between."""
    from oracle import oracle_py as O

    images, packed = _data()[:2]
    big = _take(packed, 1025)
    ctx = _ctx()
    for n_sv, kernel, n in ((257, S.POLY2, 3), (1, S.POLY2, 1025), (257, S.POLY2, 1025)):
        model, keep, sums = _case(n_sv, kernel)
        ctx.load_svm_model(*model)
        _assert_equal(ctx.classify_images(_take(packed, n)), _take(keep, n), _take(sums, n), (n_sv, n))
    w, rho = svm_model
    ctx.load_svm(w, rho)  # the compacted linear vector: back on the fused path
    okeep, osums = O.classify(images, w, rho)
    _assert_equal(ctx.classify_images(big), _take(np.asarray(okeep, np.uint8), 1025), _take(osums, 1025), "fused")
    model, keep, sums = _case(65, S.POLY2)
    ctx.load_svm_model(*model)
    _assert_equal(ctx.classify_images(packed[:64]), keep[:64], sums[:64], (65, 64))


def test_chain_and_stateless_paths_share_buffers(tiny_scene):
    """agh_classify (the chain's hog_svm) and agh_classify_images use the same descriptor and kernel-value buffers: a stateless
    call with more images than the search has hypotheses grows them between two chain calls."""
    from oracle import oracle_py as O

    sc = tiny_scene
    _, packed, _, pool = _data()
    ctx = _ctx()
    ctx.set_cloud(sc.xyz, sc.cam)
    hyps = ctx.find_hands(sc.samples)
    images = ctx.images()
    assert len(hyps) == len(images) > 2
    # rho from this search's own images, so that its labels split evenly as well
    model = S.model(65, S.POLY2, S.model_seed(65, S.POLY2), pool, O.hog_many(images))
    okeep, osums = O.classify_model(images, model)
    assert 0 < okeep.sum() < okeep.size
    ctx.load_svm_model(*model)
    keep = ctx.classify()
    assert np.array_equal(keep, okeep) and np.array_equal(ctx.hog()[1], osums)
    n = 8 * sc.samples.size + 67  # the chain sizes both buffers for 8 hypotheses per sample, whatever the search found
    assert n > len(hyps)
    more = _take(packed, n)
    qkeep, qsums = O.classify_model(S.query_images(), model)
    _assert_equal(ctx.classify_images(more), _take(qkeep, n), _take(qsums, n), "stateless")
    keep = ctx.classify()
    assert np.array_equal(keep, okeep) and np.array_equal(ctx.hog()[1], osums)
    _assert_equal(ctx.classify_images(ctx.packed_images()), okeep, osums, "the search's images, stateless")


def test_kernel_value_clamp():
    """CvSVMKernel::calc's clamp to (float)(FLT_MAX * 1e-3): POLY2 through a square that overflows float, LINEAR through a
    dot that is finite and above it; queries below the clamp (and a blank one) in the same call."""
    from oracle import oracle_py as O

    images, packed, _, pool = _data()
    ctx = _ctx()
    for model in S.clamp_models(pool):
        okeep, osums = O.classify_model(images, model)
        assert np.isfinite(osums).all() and 0 < okeep.sum() < okeep.size and (np.abs(osums) > 1e34).any()
        ctx.load_svm_model(*model)
        _assert_equal(ctx.classify_images(packed), okeep, osums, model[0])
