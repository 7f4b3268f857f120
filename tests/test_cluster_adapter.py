"""The adapter's clustered calls RUN: on the GPU Localization::localizeHandlesClustered returns, per object, the handles and kept
hands of the C call (agh_localize_clustered: the same sample list, object sizes and handle records); a clustered call while a
chain is pending returns empty lists and leaves that chain collectable (tests/cpp/cluster_adapter_test.cpp).  The new methods
compile in both type branches."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
SRC = os.path.join(ROOT, "tests", "cpp", "cluster_adapter_test.cpp")


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = CXX + ["-fsyntax-only"]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [SRC])
    for hdr, names in (("hand_search.h", ("localizeClustered", "localizeDepthClustered", "clusterInfo", "clusterLabels")),
                       ("localization.h", ("localizeHandlesClustered", "localizeHandlesDepthClustered", "setClusterParams",
                                           "getClusterSizes"))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr


@pytest.mark.gpu
def test_adapter_clustered_calls_return_the_handles_of_the_c_call(tmp_path):
    from agile_grasp_amd import build
    from tests import cluster_cases as CC

    build.build()
    exe = str(tmp_path / "cluster_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(CXX + ["-O1", SRC, "-o", exe, "-L" + libdir, "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                                 "-Wl,-rpath,/opt/rocm/lib"])
    xyz, size_left, ws, origins, cp = CC.table_scene()
    K, S = cp["max_objects"], 60
    path = str(tmp_path / "capture.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<qq", len(xyz), size_left))
        f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
        f.write(np.asarray(ws, np.float64).tobytes())
        f.write(np.array(list(cp["plane"]) + [cp["min_height"], cp["max_height"], cp["tolerance"]], np.float64).tobytes())
        f.write(struct.pack("<qqqq", cp["min_voxels"], K, S, 7))
        f.write(np.asarray(origins, np.float64).tobytes())
    out = subprocess.run([exe, "gpu", path, SVM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-800:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in
             ("C", "POINTS", "PENDING")}
    n_kept, n_handles, n_objects, n_foreground = (int(x) for x in lines["C"])
    assert n_kept >= 10 and n_handles >= 2 and n_objects == 3 and n_foreground > 1000
    assert lines["POINTS"] == ["1", "1", "1"]
    # the refused call: K empty lists, the plain chain in flight collected afterwards; 65 lists: no list, and no sizes after it
    n_refused, refused_handles, kept_p, too_many, sizes_after = (int(x) for x in lines["PENDING"])
    assert (n_refused, refused_handles, too_many, sizes_after) == (K, 0, 0, 0) and kept_p >= 1


@pytest.mark.gpu
def test_example_prints_handles_per_object_on_a_table(tmp_path):
    """examples/localize_pcd.cpp --table: the table scene's cubes inside the example's fixed workspace, handles per object."""
    from tests import cluster_cases as CC
    from tests.test_cpp_adapter import _build_example, _write_pcd

    exe = _build_example(tmp_path)
    xyz, size_left, _ws, _origins, cp = CC.table_scene()
    left, right = str(tmp_path / "l.pcd"), str(tmp_path / "r.pcd")
    _write_pcd(left, xyz[:size_left], True)
    _write_pcd(right, xyz[size_left:], True)
    plane = ",".join(repr(float(v)) for v in cp["plane"])
    out = subprocess.run([exe, "--table", plane, "--cluster-tolerance", "0.007", SVM, left, right, "60", "2"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout[-1500:])
    objects = [ln for ln in out.stdout.splitlines() if ln.startswith("object ")]
    sizes = [int(ln.split()[2]) for ln in objects]
    assert len(objects) >= 2 and sizes == sorted(sizes, reverse=True) and min(sizes) >= 50
    n_handles = sum(int(ln.split()[4]) for ln in objects)
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("  grasp ")]) == n_handles
