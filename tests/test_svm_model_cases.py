"""What tests/svm_model_cases.py promises, on the CPU: the oracle's CvSVM::predict against the independent numpy transcription
(tests/ref_numpy.classify_model) bit for bit at every support-vector count, the even split of the labels, and the two clamp
regimes.  The descriptors of the 131 query images and the 513 pool images are computed once for the module."""
import functools

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import ref_numpy as R
from tests import svm_model_cases as S


@functools.lru_cache(maxsize=None)
def _data():
    images, pool = S.query_images(), S.sv_images()
    return images, O.hog_many(images), O.hog_many(pool)


def test_image_mix():
    images, desc, pool = _data()
    both = np.concatenate([images, S.sv_images()])
    assert images.shape == (S.N_QUERY, 8000) and set(np.unique(both)) == {0, 255}
    assert len({im.tobytes() for im in both}) == len(both)  # no image twice, in either set or across them
    assert not images[S.BLANK].any() and images[S.FULL].all()
    assert not desc[S.BLANK].any() and not desc[S.FULL].any()
    stroke = np.arange(S.N_QUERY) % 2 == 1
    stroke[S.BLANK] = False
    dense = ~stroke
    dense[[S.BLANK, S.FULL]] = False
    assert np.mean(desc[stroke] == 0) > 0.9  # sparse, as a grasp image's descriptor is
    groups = desc.reshape(S.N_QUERY, 882, 4)
    filled = (groups.max(axis=2) > 0).mean(axis=1)
    assert (filled[0::6] == 1).all()  # noise: no group of four products is zero
    assert (filled[dense] > 0.4).all() and (filled[stroke] < 0.4).all()  # (pure stripes fill 4/9 or 5/9 of the groups)
    assert (desc >= 0).all() and (pool >= 0).all() and pool[0].any()
    assert np.array_equal(S.query_images(64), images[:64]) and np.array_equal(S.query_images(3), images[:3])


@pytest.mark.parametrize("kernel", [S.LINEAR, S.POLY2])
@pytest.mark.parametrize("n_sv", S.N_SV)
def test_oracle_matches_transcription(n_sv, kernel):
    images, desc, pool = _data()
    model = S.model(n_sv, kernel, S.model_seed(n_sv, kernel), pool, desc)
    assert model[1].shape == (n_sv, 3528) and model[2].shape == (n_sv,) and np.array_equal(model[1], pool[:n_sv])
    okeep, osums = O.classify_model(images, model)
    q = R.svm_kernel_values(desc, model[0], model[1])  # (R.classify_model is svm_decide of these)
    rkeep, rsums = R.svm_decide(q, model[2], model[3])
    assert np.array_equal(okeep, rkeep) and np.array_equal(osums, rsums)
    assert np.isfinite(rsums).all()
    # a condition on the inputs, from the reference alone: both labels, split about evenly, one value on the threshold
    assert 0.25 * S.N_QUERY <= int(rkeep.sum()) <= 0.75 * S.N_QUERY
    _, at_zero = R.svm_decide(q, model[2], 0.0)
    assert model[3] == np.median(at_zero) and (at_zero == model[3]).any()
    # the alphas are what makes a reordered sum change bits: not dyadic, both signs from two vectors on
    assert (np.abs(model[2]) < 1).all() and (np.ldexp(model[2], 20) != np.rint(np.ldexp(model[2], 20))).all()
    assert n_sv < 15 or ((model[2] > 0).any() and (model[2] < 0).any())


def test_clamp_models():
    images, desc, pool = _data()
    poly, linear = S.clamp_models(pool)
    assert poly[0] == S.POLY2 and linear[0] == S.LINEAR
    for model in (poly, linear):
        assert model[1].shape == (3, 3528) and np.isfinite(model[1]).all() and (model[1] >= 0).all()
        raw = R.svm_kernel_values(desc, model[0], model[1], clamp=False)
        clamped = (raw > R.SVM_MAX_VAL).any(axis=1)
        assert clamped.any() and not clamped.all()
        assert not clamped[S.BLANK] and not raw[S.BLANK].any()
        okeep, osums = O.classify_model(images, model)
        rkeep, rsums = R.classify_model(desc, *model)
        assert np.array_equal(okeep, rkeep) and np.array_equal(osums, rsums)
        assert np.isfinite(rsums).all() and 0 < int(rkeep.sum()) < S.N_QUERY
        assert rsums[S.BLANK] == -model[3] and (np.abs(rsums[clamped]) > 1e34).all()
        if model[0] == S.POLY2:
            assert np.isinf(raw).any()  # the square overflowed and was clamped, it did not stay inf
        else:
            assert np.isfinite(raw).all()  # the float dot is finite and above the clamp
            assert (int(clamped.sum()), int((~clamped).sum())) == S.CLAMP_LINEAR_COUNTS
            dense = np.arange(S.N_QUERY) % 2 == 0
            dense[S.FULL] = False
            assert np.array_equal(clamped, dense)
