"""The adapter's depth-image calls RUN (tests/cpp/depth_tu.cpp only compiles them): Localization::toHandles for a chain without a
host cloud on the host, and on the GPU localizeHandlesDepth, the Begin / stageNextDepth / End stream and images with poses of
their own, each equal to localizeHandles on the back-projected cloud (tests/cpp/depth_adapter_test.cpp)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")


def _build(tmp_path):
    from agile_grasp_amd import build

    build.build()
    exe = str(tmp_path / "depth_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "depth_adapter_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_to_handles_takes_a_chain_without_a_host_cloud(tmp_path):
    """what localizeHandlesEnd passes on for a chain begun from depth images: an empty cloud pointer"""
    out = subprocess.run([_build(tmp_path), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert "HOST 0 0" in out.stdout


@pytest.mark.gpu
def test_adapter_depth_calls_equal_localize_handles_on_the_deprojected_cloud(tmp_path):
    from tests import depth_captures as D
    from tests.test_depth_captures import samples_for

    images, ws, _ = D.main_case()
    pts = D.deproject_ref(images)
    vox, _ = D.voxel_model(pts, D.image_index(images), ws)
    idx = samples_for(len(vox))
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
        f.write(struct.pack("<q", len(idx)))
        f.write(idx.astype(np.int32).tobytes())
    out = subprocess.run([_build(tmp_path), "gpu", path, SVM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    lines = {ln.split()[0] + (" " + ln.split()[1] if ln.startswith("STREAM") else ""): ln.split() for ln in out.stdout.splitlines()
             if ln.split() and ln.split()[0] in ("POINTS", "DEPTH", "STREAM", "POSED")}
    n_kept, n_handles = int(lines["POINTS"][1]), int(lines["POINTS"][2])
    print(out.stdout[-600:])
    assert n_kept >= 1 and n_handles >= 1
    assert lines["DEPTH"][1:] == [str(n_kept), str(n_handles), "1"]
    assert lines["STREAM 0"][2:] == ["1", "1", "1"]  # the second Begin refused, the stage accepted, the results the same
    assert lines["STREAM 1"][2:] == ["1"]
    assert lines["POSED"][1:] == ["1"]
