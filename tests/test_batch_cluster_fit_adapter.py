"""The adapter's fitted clustered batch calls RUN: on the GPU Localization::localizeHandlesBatchClusteredFit returns, per capture
and object, the handles and kept hands of the C call (agh_localize_batch_clustered_fit: the same planes, object sizes and handle
records), its Begin / End halves give the same, and a fitted batch while a chain is pending returns empty lists and leaves that
chain collectable (tests/cpp/batch_cluster_fit_adapter_test.cpp).  The new members compile in both type branches."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
SRC = os.path.join(ROOT, "tests", "cpp", "batch_cluster_fit_adapter_test.cpp")


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_members_compile_in_both_type_branches(real_types):
    cmd = CXX + ["-fsyntax-only"]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [SRC])
    for hdr, names in (("hand_search.h", ("agh_localize_batch_clustered_fit_begin(", "agh_localize_depth_batch_clustered_fit_begin(",
                                          "batchPlaneFit")),
                       ("localization.h", ("localizeHandlesBatchClusteredFit", "localizeHandlesBatchClusteredFitBegin",
                                           "localizeHandlesDepthBatchClusteredFit", "localizeHandlesDepthBatchClusteredFitBegin",
                                           "fittedPlanes", "std::vector<agh_plane_fit_params> fp(clouds.size(), plane_fit_)"))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr


def test_adapter_members_behave_on_the_host_stubs(tmp_path):
    """Without a device: the record checks of the Begin halves refuse before any library call, and the getters answer empty."""
    src = tmp_path / "host.cpp"
    src.write_text(r'''
#include <cstdio>
#include "chain_common.h"
int main()
{
  Localization loc(1, false, 0);
  std::vector<bool> found(3, true);
  const bool none = loc.fittedPlanes(&found).empty() && found.empty();  // (no search object yet: no library call)
  std::vector<PointCloud::Ptr> clouds(2);  // (null clouds: "Input cloud is empty!")
  const std::vector<int> sizes(2, 1);
  const bool empty_refused = !loc.localizeHandlesBatchClusteredFitBegin(clouds, sizes, "no-such-svm", 2, 0.005);
  std::vector<std::vector<std::vector<GraspHypothesis> > > kept(1);
  loc.setClusterParams(0.005, 0.5, 0.011, 4, 3);
  const std::vector<std::vector<std::vector<Handle> > > out = loc.localizeHandlesBatchClusteredFit(clouds, sizes, "no-such-svm", 2, 0.005, &kept);
  bool shaped = out.size() == 2 && kept.size() == 2;  // (per capture and object where the records say how many)
  for (size_t k = 0; shaped && k < 2; k++)
    shaped = out[k].size() == 3 && kept[k].size() == 3 && out[k][0].empty();
  const std::vector<agh_cluster_params> three(3);
  const bool mismatch = loc.localizeHandlesBatchClusteredFit(clouds, sizes, "no-such-svm", 2, 0.005, nullptr, nullptr, &three).empty();
  std::vector<std::vector<DepthImage> > captures(2);  // (no image in either capture)
  const bool depth_refused = !loc.localizeHandlesDepthBatchClusteredFitBegin(captures, "no-such-svm", 2, 0.005) &&
                             loc.localizeHandlesDepthBatchClusteredFit(captures, "no-such-svm", 2, 0.005).size() == 2;
  std::printf("HOST %d %d %d %d %d\n", none ? 1 : 0, empty_refused ? 1 : 0, shaped ? 1 : 0, mismatch ? 1 : 0, depth_refused ? 1 : 0);
  return 0;
}
''')
    exe = str(tmp_path / "host")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(CXX + ["-O1", "-I" + os.path.join(ROOT, "tests", "cpp"), str(src), "-o", exe, "-L" + libdir, "-lagile_grasp_hip",
                                 "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("HOST ")]
    assert line and line[0].split()[1:] == ["1", "1", "1", "1", "1"], out.stdout[-2000:]


@pytest.mark.gpu
def test_adapter_fitted_batch_returns_the_handles_of_the_c_call(tmp_path):
    from agile_grasp_amd import build
    from tests import plane_fit_cases as PF

    build.build()
    exe = str(tmp_path / "batch_cluster_fit_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(CXX + ["-O1", SRC, "-o", exe, "-L" + libdir, "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                                 "-Wl,-rpath,/opt/rocm/lib"])
    xyz, size_left, ws, origins, cp, _centre = PF.rotated_scene()
    K, S = cp["max_objects"], 40
    path = str(tmp_path / "capture.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<qq", len(xyz), size_left))
        f.write(np.ascontiguousarray(xyz, np.float32).tobytes())
        f.write(np.asarray(ws, np.float64).tobytes())
        f.write(np.array([1.0, 0.0, 0.0, 0.0, cp["min_height"], cp["max_height"], cp["tolerance"]], np.float64).tobytes())
        f.write(struct.pack("<qqqq", cp["min_voxels"], K, S, 7))
        f.write(np.asarray(origins, np.float64).tobytes())
        f.write(struct.pack("<qqd", 128, 2, 0.004))
    out = subprocess.run([exe, "gpu", path, SVM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-800:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln.split() and ln.split()[0] in
             ("C", "POINTS", "PENDING")}
    n_kept, n_handles, n_objects, n_foreground, found, refined = (int(x) for x in lines["C"])
    assert n_kept >= 10 and n_handles >= 2 and n_objects == 6 and n_foreground > 2000 and (found, refined) == (2, 2)
    assert lines["POINTS"] == ["1", "1", "1", "1"]
    # the refused call: two captures of K empty lists and no fitted planes, the plain chain in flight collected afterwards; cluster
    # records for three captures with two clouds: no list
    captures, lists, refused_handles, kept_p, planes_pending, mismatch = (int(x) for x in lines["PENDING"])
    assert (captures, lists, refused_handles, planes_pending, mismatch) == (2, 2 * K, 0, 0, 0) and kept_p >= 1
