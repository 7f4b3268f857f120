"""The adapter's labelled calls RUN: on the GPU Localization::localizeHandlesDepthLabeled and localizeHandlesLabeled return, per
object, the handles and kept hands of the C call (agh_localize_depth_labeled: the same sample list, eligible-voxel counts and
handle records); a labelled call while a chain is pending returns empty lists and leaves that chain collectable
(tests/cpp/label_adapter_test.cpp).  The new methods compile in both type branches."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
SRC = os.path.join(ROOT, "tests", "cpp", "label_adapter_test.cpp")


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = CXX + ["-fsyntax-only"]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [SRC])
    for hdr, names in (("hand_search.h", ("localizeLabeled", "localizeDepthLabeled", "labelCounts")),
                       ("localization.h", ("localizeHandlesLabeled", "localizeHandlesDepthLabeled", "getLabelCounts")),
                       ("types.h", ("struct LabelImage",))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr


@pytest.mark.gpu
def test_adapter_labelled_calls_return_the_handles_of_the_c_call(tmp_path):
    from agile_grasp_amd import build
    from tests import depth_captures as D
    from tests import label_cases as L
    from tests import mask_cases as M

    build.build()
    exe = str(tmp_path / "label_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(CXX + ["-O1", SRC, "-o", exe, "-L" + libdir, "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                                 "-Wl,-rpath,/opt/rocm/lib"])
    images, ws, _ = D.main_case()
    K, S = 12, 100
    rng = np.random.default_rng(3)
    labels = [M.padded_mask(rng, L.tiled_labels(images[0]["data"].shape), 5), None]
    pts = D.deproject_ref(images)
    packed = M.packed_masks(images, labels)
    E = [M.eligible_model(pts, D.image_index(images), packed == j + 1, ws) for j in range(K)]
    path = str(tmp_path / "capture.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(images)))
        for im in images:
            d = im["data"]
            wide = np.full((d.shape[0], d.strides[0] // 2), 7, np.uint16)  # (the rows with their padding)
            wide[:, :d.shape[1]] = d
            f.write(struct.pack("<qqq", d.shape[1], d.shape[0], d.strides[0]))
            f.write(np.array([im["fx"], im["fy"], im["cx"], im["cy"]], np.float64).tobytes())
            f.write(np.asarray(im["pose"], np.float64).tobytes())
            f.write(wide.tobytes())
        f.write(np.asarray(ws, np.float64).tobytes())
        f.write(struct.pack("<qqq", S, 7, K))
        for m in labels:
            if m is None:
                f.write(struct.pack("<q", 0))
            else:
                f.write(struct.pack("<q", m.strides[0]))
                f.write(np.ascontiguousarray(m.base).tobytes())
    out = subprocess.run([exe, "gpu", path, SVM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-800:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in
             ("C", "DEPTH", "POINTS", "PENDING")}
    n_kept, n_handles, eligible, with_handles = (int(x) for x in lines["C"])
    assert n_kept >= 10 and n_handles >= 2 and with_handles >= 2 and eligible == sum(len(e) for e in E) > 300
    assert lines["DEPTH"] == ["1", "1", "1"]
    assert lines["POINTS"] == ["1", "-1"]  # (a labelled chain leaves no mask count)
    # the refused call: K empty lists, the masked chain in flight collected afterwards with its count; 65 objects: no list
    n_refused, refused_handles, count_m, kept_m, too_many = (int(x) for x in lines["PENDING"])
    assert (n_refused, refused_handles, too_many) == (K, 0, 0) and kept_m >= 1
    assert count_m == len(M.eligible_model(pts, D.image_index(images), packed != 0, ws))
