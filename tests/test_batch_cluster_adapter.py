"""The adapter's clustered batch calls (include/agile_grasp_amd/localization.h, hand_search.h) compile in both type branches
with the documented types: a plane per capture, an optional vector of per-capture cluster records, collected by
localizeHandlesBatchLabeledEnd (tests/cpp/batch_cluster_adapter_test.cpp).  Needs no GPU."""
import os
import subprocess

import pytest

from tests.test_cpp_adapter import ROOT

CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
SRC = os.path.join(ROOT, "tests", "cpp", "batch_cluster_adapter_test.cpp")


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = CXX + ["-fsyntax-only"]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [SRC])
    for hdr, names in (("hand_search.h", ("localizeBatchClusteredBegin", "localizeDepthBatchClusteredBegin", "batchClusterInfo",
                                          "agh_localize_batch_clustered_begin", "agh_localize_depth_batch_clustered_begin",
                                          "agh_get_batch_cluster_info")),
                       ("localization.h", ("localizeHandlesBatchClustered", "localizeHandlesBatchClusteredBegin",
                                           "localizeHandlesDepthBatchClustered", "localizeHandlesDepthBatchClusteredBegin",
                                           "getBatchClusterSizes"))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr


def test_without_records_set_cluster_params_applies_to_every_capture():
    """the Begin builds the records from setClusterParams' one where no vector is given, and takes the plane from planes[k]"""
    text = open(os.path.join(ROOT, "include", "agile_grasp_amd", "localization.h")).read()
    body = text[text.index("std::vector<agh_cluster_params> batchClusterParams("):]
    body = body[:body.index("bool batchPlanesGiven(")]
    assert "cluster_params ? (*cluster_params)[k] : cluster_" in body and "plane[q] = planes[k](q)" in body
    end = text[text.index("localizeHandlesBatchClustered("):text.index("bool localizeHandlesBatchClusteredBegin(")]
    assert "localizeHandlesBatchLabeledEnd(antipodal_hands_per_object)" in end
