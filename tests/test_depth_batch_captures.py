"""The batches of tests/depth_batch_captures.py are in the regimes the GPU tests (tests/test_gpu_localize_depth_batch.py) rely
on, so that none of them passes on an empty case.  No GPU."""
import numpy as np

from tests import depth_batch_captures as DB
from tests import depth_captures as D


def test_edge_batch_covers_the_batch_kernels_paths():
    caps = DB.edge_batch()
    starts = DB.starts_of(caps)
    assert {len(c) for c in caps} == {1, 2}  # captures of one image and of two
    fmts = [{im["data"].dtype.type for im in c} for c in caps]
    assert any(f == {np.uint16, np.float32} for f in fmts)  # both formats within one capture ...
    assert {np.uint16} in fmts and {np.float32} in fmts     # ... and across captures
    # a 1 x 1 image next to the 320 x 240 main images: one block beside 75 per view
    shapes = [[im["data"].shape for im in c] for c in caps]
    big = [k for k, s in enumerate(shapes) if s == [(D.MAIN_H, D.MAIN_W)] * 2]
    assert big and shapes[big[0] + 1] == [(1, 1)]
    # totals of 1023 and 1025: the next capture's first point is no multiple of four, and it has whole runs of four pixels, which
    # therefore take the element stores; the main images, at point 0, take the wide ones
    totals = [DB.points_of(c) for c in caps]
    for t in (1023, 1025):
        k = totals.index(t)
        assert starts[k + 1] % 4 != 0 and caps[k + 1][0]["data"].shape[1] >= 4, t
    assert starts[big[0]] % 4 == 0
    assert any(starts[k] % 4 != 0 and shapes[k][0] == (D.MAIN_H, D.MAIN_W) for k in range(len(caps)))  # ... and a large image off it
    # padded rows, and a U16 stride that is an odd number of elements
    strides = [(im["data"].strides[0], im["data"].shape[1] * im["data"].itemsize, im["data"].dtype) for c in caps for im in c]
    assert any(s > row and dt == np.float32 for s, row, dt in strides)
    assert any(s > row and dt == np.uint16 and (s // 2) % 2 == 1 for s, row, dt in strides)
    assert DB.deproject_ref(caps).shape == (starts[-1], 3)


def test_max_views_fills_the_table():
    caps = DB.max_views()
    assert len(caps) == 64 and all(len(c) == 2 for c in caps)
    sizes = [im["data"].size for c in caps for im in c]
    assert len(sizes) == 128 and max(sizes) <= 27 and len(set(sizes)) > 4
    assert {im["data"].dtype.type for c in caps for im in c} == {np.uint16, np.float32}
    starts = DB.starts_of(caps)
    assert len({int(s) % 4 for s in starts[:-1]}) == 4  # every alignment of a capture's first point


def test_main_batch_layout():
    caps, ws, origins = DB.main_batch()
    assert [len(c) for c in caps] == [2, 2, 2, 2, 1, 2]
    assert all(im["data"].dtype == np.uint16 for c in caps[:5] for im in c)
    assert all(im["data"].dtype == np.float32 for im in caps[5])
    assert all(im["data"].shape == (D.MAIN_H, D.MAIN_W) and im["data"].strides[0] > D.MAIN_W * im["data"].itemsize
               for c in caps for im in c)
    # different captures: no two of the U16 ones hold the same readings
    firsts = [c[0]["data"] for c in caps[:5]]
    assert all(not np.array_equal(firsts[a], firsts[b]) for a in range(5) for b in range(a))
    # the float32 capture is capture 2 in metres: the same points, bit for bit
    assert np.array_equal(D.deproject_ref(caps[5]).view(np.uint32), D.deproject_ref(caps[2]).view(np.uint32))
    assert origins.shape == (2, 3) and len(ws) == 6


def test_oracle_finds_hands_in_every_capture_and_a_handle_in_the_batch():
    from oracle import oracle_py as O

    caps, ws, origins = DB.main_batch()
    n_handles = 0
    for k, images in enumerate(caps):
        vox, cam = DB.voxels_of(images, ws)
        hyps = O.find_hands(O.default_params(origins), vox, cam, DB.samples_for(k, len(vox)))["hyps"]
        handles, _ = O.find_handles(hyps, 2, 0.005)
        print("capture", k, "voxels", len(vox), "hypotheses", len(hyps), "handles", len(handles))
        assert len(hyps) >= 20, k
        if len(images) == 2:
            assert np.bincount(cam, minlength=2).min() > 1000
        n_handles += len(handles)
    assert n_handles >= 1
