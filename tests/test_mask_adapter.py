"""The adapter's masked calls RUN: on the GPU Localization::localizeHandlesDepthMasked and localizeHandlesMasked return the
handles of the C calls (agh_localize_depth_masked: the same sample list, counts and handle records) and of localizeHandles with
the list the masked call searched; a masked Begin while a chain is pending returns false and leaves that chain collectable
(tests/cpp/mask_adapter_test.cpp).  The new methods compile in both type branches."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
SRC = os.path.join(ROOT, "tests", "cpp", "mask_adapter_test.cpp")


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = CXX + ["-fsyntax-only"]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [SRC])
    for hdr, names in (("hand_search.h", ("localizeMaskedBegin", "localizeDepthMaskedBegin", "sampleMaskCount")),
                       ("localization.h", ("localizeHandlesMasked", "localizeHandlesDepthMasked", "getSampleMaskCount")),
                       ("types.h", ("struct SampleMask",))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr


@pytest.mark.gpu
def test_adapter_masked_calls_return_the_handles_of_the_c_calls(tmp_path):
    from agile_grasp_amd import build
    from tests import depth_captures as D
    from tests import mask_cases as M
    from tests.test_gpu_localize_masked import RECT

    build.build()
    exe = str(tmp_path / "mask_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(CXX + ["-O1", SRC, "-o", exe, "-L" + libdir, "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                                 "-Wl,-rpath,/opt/rocm/lib"])
    images, ws, _ = D.main_case()
    m0 = np.zeros(images[0]["data"].shape, np.uint8)
    m0[RECT] = 1
    rng = np.random.default_rng(3)
    masks = [M.padded_mask(rng, m0, 5), None]
    pts = D.deproject_ref(images)
    E = M.eligible_model(pts, D.image_index(images), M.packed_masks(images, masks), ws)
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
        f.write(struct.pack("<qq", 300, 7))
        for m in masks:
            if m is None:
                f.write(struct.pack("<q", 0))
            else:
                f.write(struct.pack("<q", m.strides[0]))
                f.write(np.ascontiguousarray(m.base).tobytes())
    out = subprocess.run([exe, "gpu", path, SVM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-800:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in
             ("C", "DEPTH", "EXPLICIT", "POINTS", "PENDING")}
    n_kept, n_handles, m_c = (int(x) for x in lines["C"])
    assert n_kept >= 1 and n_handles >= 1 and m_c == len(E) > 300
    assert lines["DEPTH"] == [str(n_kept), str(n_handles), str(len(E)), "1", "1"]
    assert lines["EXPLICIT"] == [str(n_kept), str(n_handles), "1", "-1"]  # (an unmasked chain leaves no count)
    assert lines["POINTS"] == ["1", str(len(E))]
    assert lines["PENDING"] == ["1", "1", "-1", "1"]
