"""The adapter's depth-batch calls RUN (tests/cpp/depth_batch_tu.cpp only compiles them): on the GPU localizeHandlesDepthBatch,
the Begin / localizeHandlesBatchEnd halves and the overload with per-capture camera transforms, each equal to
localizeHandlesBatch on the back-projected clouds (tests/cpp/depth_batch_adapter_test.cpp)."""
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
    exe = str(tmp_path / "depth_batch_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "depth_batch_adapter_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_the_program_builds_and_refuses_a_missing_file(tmp_path):
    out = subprocess.run([_build(tmp_path), str(tmp_path / "none.bin"), SVM], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2


@pytest.mark.gpu
def test_adapter_depth_batch_equals_localize_handles_batch_on_the_deprojected_clouds(tmp_path):
    from tests import depth_batch_captures as DB

    caps, ws, _ = DB.main_batch()
    pick = [0, 1, 4]  # two captures of two images, one of one (uint16 all: the file holds uint16 pixels)
    path = str(tmp_path / "batch.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(pick)))
        f.write(np.asarray(ws, np.float64).tobytes())
        for k in pick:
            images = caps[k]
            f.write(struct.pack("<q", len(images)))
            for im in images:
                d = im["data"]
                wide = np.full((d.shape[0], d.strides[0] // 2), 7, np.uint16)  # (the rows with their padding)
                wide[:, :d.shape[1]] = d
                f.write(struct.pack("<qqq", d.shape[1], d.shape[0], d.strides[0]))
                f.write(np.array([im["fx"], im["fy"], im["cx"], im["cy"]], np.float64).tobytes())
                f.write(np.asarray(im["pose"], np.float64).tobytes())
                f.write(wide.tobytes())
            idx = DB.samples_for(k, len(DB.voxels_of(images, ws)[0]))
            f.write(struct.pack("<q", len(idx)))
            f.write(idx.astype(np.int32).tobytes())
    out = subprocess.run([_build(tmp_path), path, SVM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()
             if ln.split() and ln.split()[0] in ("POINTS", "DEPTH", "HALVES", "RIGS", "FAR")}
    print(out.stdout[-600:])
    n_caps, least_kept, _n_kept, n_handles = (int(x) for x in lines["POINTS"])
    assert n_caps == len(pick) and least_kept >= 1 and n_handles >= 1
    assert lines["DEPTH"] == ["1"]
    assert lines["HALVES"] == ["1", "1"]  # a second Begin of either kind refused, the results the same
    assert lines["RIGS"] == ["1"]
    assert lines["FAR"] == ["0"]  # (without the table the object's far origins turn the normals: other hands)
