"""The adapter's labelled batch calls RUN: on the GPU Localization::localizeHandlesDepthBatchLabeled and localizeHandlesBatchLabeled
return, per capture and object, the kept hands, the handles and the eligible-voxel counts of the C call
(agh_localize_depth_batch_labeled), and a labelled Begin while a chain is pending returns false and leaves that chain collectable
(tests/cpp/batch_label_adapter_test.cpp).  The new methods compile in both type branches."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
SRC = os.path.join(ROOT, "tests", "cpp", "batch_label_adapter_test.cpp")
PICK = (0, 1, 4)  # of the main batch: two captures of two images, one of one (uint16 all: the file holds uint16 pixels)
TILES = ((2, 3), (1, 1), (1, 2))  # image 0's tiling per picked capture: 6, 1 and 2 objects


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = CXX + ["-fsyntax-only"]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [SRC])
    for hdr, names in (("hand_search.h", ("localizeBatchLabeledBegin", "localizeDepthBatchLabeledBegin", "batchLabelCounts")),
                       ("localization.h", ("localizeHandlesBatchLabeled", "localizeHandlesBatchLabeledBegin",
                                           "localizeHandlesDepthBatchLabeled", "localizeHandlesDepthBatchLabeledBegin",
                                           "getBatchLabelCounts"))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr


@pytest.mark.gpu
def test_adapter_labelled_batch_calls_return_the_handles_of_the_c_call(tmp_path):
    from agile_grasp_amd import build
    from tests import depth_captures as D
    from tests import label_cases as L
    from tests import mask_batch_cases as MB
    from tests import mask_cases as M

    build.build()
    exe = str(tmp_path / "batch_label_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(CXX + ["-O1", SRC, "-o", exe, "-L" + libdir, "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                                 "-Wl,-rpath,/opt/rocm/lib"])
    b = MB.depth_batches()["main"]
    ws = b["workspaces"][0]
    rng = np.random.default_rng(3)
    path = str(tmp_path / "batch.bin")
    want_m = []
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(PICK)))
        f.write(np.asarray(ws, np.float64).tobytes())
        f.write(struct.pack("<qq", 100, 7))
        for k, (rows, cols) in zip(PICK, TILES):
            images = b["captures"][k]
            labels = [M.padded_mask(rng, L.tiled_labels(images[0]["data"].shape, rows, cols), 5), None][:len(images)]
            packed = M.packed_masks(images, labels)
            pts, cams = D.deproject_ref(images), D.image_index(images)
            want_m += [len(M.eligible_model(pts, cams, packed == j + 1, ws)) for j in range(rows * cols)]
            f.write(struct.pack("<qq", rows * cols, len(images)))
            for im, m in zip(images, labels):
                d = im["data"]
                wide = np.full((d.shape[0], d.strides[0] // 2), 7, np.uint16)  # (the rows with their padding)
                wide[:, :d.shape[1]] = d
                f.write(struct.pack("<qqq", d.shape[1], d.shape[0], d.strides[0]))
                f.write(np.array([im["fx"], im["fy"], im["cx"], im["cy"]], np.float64).tobytes())
                f.write(np.asarray(im["pose"], np.float64).tobytes())
                f.write(wide.tobytes())
                if m is None:
                    f.write(struct.pack("<q", 0))
                else:
                    f.write(struct.pack("<q", m.strides[0]))
                    f.write(np.ascontiguousarray(m.base).tobytes())
    out = subprocess.run([exe, path, SVM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-1200:])
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.split()]
    c_rows = [[int(x) for x in r[1:]] for r in rows if r[0] == "C"]
    assert [(r[0], r[1]) for r in c_rows] == [(c, j) for c, (rr, cc) in enumerate(TILES) for j in range(rr * cc)]
    assert sum(r[2] for r in c_rows) >= 20 and sum(r[3] for r in c_rows) >= 2, c_rows  # kept hands and handles to compare
    for c in range(len(PICK)):
        assert max(r[2] for r in c_rows if r[0] == c) >= 1, c_rows  # ... in every capture
    assert [r[4] for r in c_rows] == want_m
    lines = {r[0]: r[1:] for r in rows if r[0] in ("DEPTH", "POINTS", "PENDING", "FLAT", "OTHER")}
    assert lines["DEPTH"] == ["1", "1", "1", "1"]  # counts, handle records, sample list, M_{k,j}
    assert lines["POINTS"] == ["1", "1"]
    assert lines["PENDING"] == ["1", "1", "0", "1"]  # both Begins refused, no counts while pending, the chain collected
    assert lines["FLAT"] == ["1"]
    assert lines["OTHER"] == ["1", "1", "1"]  # the labelled End refused on an unlabelled pending batch, which is then collected
