"""The depth filter's numpy model and its cases (tests/depth_filter_cases.py): every case exercises what its name says, and the
injected main case is one on which the filter has something to do.  Conditions on the INPUTS of the GPU tests, not on the library;
needs no GPU."""
import numpy as np
import pytest

from tests import depth_captures as DC
from tests import depth_filter_cases as FC


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_case_exercises_what_it_says(name):
    case = FC.cases()[name]
    case["check"](case)
    pts, counts = FC.filter_points(case["images"], case["fp"])
    assert pts.dtype == np.float32 and pts.shape == (sum(im["data"].size for im in case["images"]), 3)
    kept = np.isfinite(pts).all(1)
    assert (np.isnan(pts).all(1) | kept).all() and kept.sum() == counts[:, 3].sum()
    assert (counts[:, 0] == counts[:, 1:].sum(1)).all()


def test_the_cases_cover_the_sizes_formats_radii_and_supports():
    cases = FC.cases()
    for w, h in FC.SIZES:
        for fmt in ("u16", "f32"):
            assert any(n.startswith(f"{fmt}_{w}x{h}_") for n in cases), (fmt, w, h)
    seen = {(c["fp"]["radius"], c["fp"]["min_support"]) for c in cases.values()}
    assert set(FC.settings(1) + FC.settings(2)) <= seen
    assert any(len(c["images"]) == 2 and c["images"][0]["data"].dtype != c["images"][1]["data"].dtype for c in cases.values())


def test_model_without_a_neighbourhood_is_the_plain_deprojection():
    # min_support cannot be 0, but a tolerance of +inf on a full image keeps every valid pixel: the model's points are deproject_ref's
    images = [FC.cases()["borders_s3"]["images"][0]]
    pts, counts = FC.filter_points(images, FC.params(max_jump_abs=3e38))
    assert np.array_equal(pts, DC.deproject_ref(images)) and counts[0, 3] == images[0]["data"].size


def test_injected_main_case_rejects_the_flying_pixels_and_keeps_the_rest():
    images, masks, _ws, _origins, fp = FC.injected_main()
    for k, (im, inj) in enumerate(zip(images, masks)):
        m = FC.filter_image(im, fp)
        n_inj = int(inj.sum())
        rejected = int((inj & ~m["keep"]).sum())
        others = m["valid"] & ~inj
        kept = float((others & m["keep"]).sum()) / float(others.sum())
        print(f"image {k}: {rejected} of {n_inj} injected pixels rejected, {100 * kept:.2f} % of the other valid pixels kept")
        assert n_inj > 1000
        assert rejected >= 0.99 * n_inj
        assert kept >= 0.99


def test_model_keeps_the_unmodified_main_case():
    images, _ws, _origins = DC.main_case()
    for k, im in enumerate(images):
        m = FC.filter_image(im, FC.params())
        frac = float(m["keep"].sum()) / float(m["valid"].sum())
        print(f"image {k}: {100 * frac:.2f} % of the valid pixels kept")
        assert frac >= 0.99
