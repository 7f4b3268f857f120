"""The captures of tests/depth_captures.py are in the regimes the GPU tests (tests/test_gpu_localize_depth.py) rely on.  No GPU."""
import numpy as np

from tests import depth_captures as D

SAMPLES = 400


def samples_for(n_voxels: int) -> np.ndarray:
    """the explicit sample list the GPU test uses on the main case"""
    return np.sort(np.random.default_rng(5).permutation(n_voxels)[:SAMPLES]).astype(np.int32)


def test_main_case_has_padded_rows_and_many_invalid_pixels():
    images, _, _ = D.main_case()
    assert len(images) == 2
    for im in images:
        d = im["data"]
        assert d.dtype == np.uint16 and d.shape == (D.MAIN_H, D.MAIN_W) and d.strides[0] > d.shape[1] * 2
        frac = float((d == 0).mean())
        print("invalid fraction", frac)
        assert 0.10 <= frac <= 0.90
    assert float((images[0]["data"] == 0).mean()) >= 0.10


def test_rank_labels_differ_from_image_index_on_kept_voxels():
    """dense = 0 ranks the finite points: with this many invalid pixels camera 1's first points would be labelled camera 0.
    The voxelised clouds of the two labellings differ, so the GPU test tells them apart."""
    images, ws, _ = D.main_case()
    pts = D.deproject_ref(images)
    by_image = D.voxel_model(pts, D.image_index(images), ws)
    lab = D.rank_labels(pts, images[0]["data"].size)
    by_rank = D.voxel_model(pts[lab >= 0], lab[lab >= 0], ws)
    a = set(map(tuple, np.column_stack([by_image[0].view(np.uint32), by_image[1]])))
    b = set(map(tuple, np.column_stack([by_rank[0].view(np.uint32), by_rank[1]])))
    assert len(a - b) >= 1 and len(b - a) >= 1
    assert np.bincount(by_image[1], minlength=2).min() > 1000


def test_float32_model_differs_from_float64():
    images, _, _ = D.main_case()
    a, b = D.deproject_ref(images), D.deproject_f64(images)
    fin = np.isfinite(a).all(1)
    assert np.array_equal(fin, np.isfinite(b).all(1)) and fin.sum() > 10_000
    assert int((a[fin].view(np.uint32) != b[fin].view(np.uint32)).sum()) >= 1
    assert np.allclose(a[fin], b[fin], rtol=0, atol=1e-5)  # ... and is the same back-projection


def test_voxel_model_is_the_oracles_preprocessing_with_dense_ids():
    from oracle import oracle_py as O

    images, ws, _ = D.main_case()
    pts = D.deproject_ref(images)
    vox, cam = D.voxel_model(pts, D.image_index(images), ws)
    ovox, ocam = O.preprocess(pts, images[0]["data"].size, ws, 0.003, dense=True)
    assert np.array_equal(vox, ovox) and np.array_equal(cam, ocam)


def test_oracle_finds_hands_and_handles_on_the_deprojected_cloud():
    from oracle import oracle_py as O

    images, ws, origins = D.main_case()
    pts = D.deproject_ref(images)
    vox, cam = D.voxel_model(pts, D.image_index(images), ws)
    hyps = O.find_hands(O.default_params(origins), vox, cam, samples_for(len(vox)))["hyps"]
    handles, _ = O.find_handles(hyps, 2, 0.005)
    print("hypotheses", len(hyps), "handles", len(handles))
    assert len(hyps) >= 20 and len(handles) >= 1


def test_edge_cases_cover_the_kernels_paths():
    cases = D.edge_cases()
    totals = {sum(im["data"].size for im in ims) for ims in cases.values()}
    assert {1, 1023, 1024, 1025} <= totals
    widths = {im["data"].shape[1] for ims in cases.values() for im in ims}
    assert {1, 63, 65, 257} <= widths and any(w % 4 == 0 for w in widths)
    odd = cases["u16_odd_stride"][0]["data"]
    assert odd.dtype == np.uint16 and (odd.strides[0] // 2) % 2 == 1 and odd.strides[0] > odd.shape[1] * 2
    sp = cases["f32_special_values"][0]["data"]
    assert (sp == 0).any() and (sp < 0).any() and np.isnan(sp).any() and np.isposinf(sp).any()
    assert ((sp > 0) & (sp < np.finfo(np.float32).tiny)).any()  # a denormal: valid
    ref = D.deproject_ref(cases["f32_special_values"])
    assert np.isnan(ref[[0, 1, 2, 3, 5, 6]]).all() and np.isfinite(ref[[4, 7, 8]]).all()
    so = cases["f32_special_unaligned"][0]["data"]
    assert so.shape[1] % 4 != 0 and (so.shape[1] * 4) % 16 != 0  # rows off the 16-byte boundary, a tail run in each
    assert np.isnan(so[1]).any() and np.isposinf(so[1]).any() and ((so[1] > 0) & (so[1] < np.finfo(np.float32).tiny)).any()
    ref = D.deproject_ref(cases["f32_special_unaligned"])
    assert np.isnan(ref[[7, 8, 9, 10, 12]]).all() and np.isfinite(ref[[11, 13]]).all()
    assert len(cases["one_image"]) == 1
    for name, ims in cases.items():
        assert D.deproject_ref(ims).shape == (sum(im["data"].size for im in ims), 3), name
