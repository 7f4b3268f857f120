"""The adapter's voxel-filter methods RUN (tests/test_voxel_filter_abi.py only compiles them): Localization::setVoxelFilter and
its family through localizeHandles on the speckle capture of tests/voxel_filter_cases.py -- the counts are the numpy model's, the
setting is sticky across a re-created search, refused while a chain is pending, and cleared it gives the unfiltered chain back
(tests/cpp/voxel_filter_adapter_test.cpp)."""
import os
import subprocess

import pytest

from tests.test_cpp_adapter import GOLD, ROOT, _dump_raw

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")


def _build(tmp_path):
    from agile_grasp_amd import build

    build.build()
    exe = str(tmp_path / "voxel_filter_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "voxel_filter_adapter_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_adapter_voxel_filter_counts_stickiness_and_refusals(tmp_path):
    from agile_grasp_amd.binding import draw_samples
    from tests import voxel_filter_cases as VF

    c = VF.speckle_capture()
    m = VF.case_model(c)
    idx = draw_samples(int(m["keep"].sum()), 300, 3)  # (valid in the filtered cloud, so in the unfiltered one too)
    path = str(tmp_path / "raw.bin")
    _dump_raw(path, c["points"], c["size_left"], idx, c["workspace"], c["origins"])
    out = subprocess.run([_build(tmp_path), SVM, path, str(c["radius"]), str(c["min_neighbors"])], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-600:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()
             if ln.split() and ln.split()[0] in ("COUNTS", "PLAIN", "FILTERED", "LOCALIZATION", "SEARCH")}
    assert [int(v) for v in lines["COUNTS"]] == m["counts"].tolist()
    assert lines["LOCALIZATION"] == ["1"] * 13
    assert lines["SEARCH"] == ["1", "1", "0", "1"]  # (the last voxelisation, after the clear, ran unfiltered: no counts)
    assert int(lines["PLAIN"][0]) >= 1 and int(lines["FILTERED"][0]) >= 1
