"""agh_localize_batch_begin / _begin_device / _stage / _end (include/agh.h): declared with the documented signatures, exported by
the library, refused without a context before any device call, and the adapter's new methods
(HandSearch::localizeBatchBegin / localizeBatchStage / localizeBatchEnd, Localization::localizeHandlesBatchBegin / stageNextBatch /
localizeHandlesBatchEnd) compile in both type branches.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_batch_begin", "agh_localize_batch_begin_device", "agh_localize_batch_stage", "agh_localize_batch_end")

SRC = r"""
#include <type_traits>
#include "agh.h"
typedef int (*begin_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const agh_localize_params*, int32_t);
typedef int (*stage_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, int32_t);
typedef int (*end_fn)(agh_ctx*, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
static_assert(std::is_same<decltype(&agh_localize_batch_begin), begin_fn>::value, "agh_localize_batch_begin");
static_assert(std::is_same<decltype(&agh_localize_batch_begin_device), begin_fn>::value, "agh_localize_batch_begin_device");
static_assert(std::is_same<decltype(&agh_localize_batch_stage), stage_fn>::value, "agh_localize_batch_stage");
static_assert(std::is_same<decltype(&agh_localize_batch_end), end_fn>::value, "agh_localize_batch_end");
int main() { return 0; }
"""


def test_header_declares_and_library_exports_the_calls(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "agh.h")).read()
    from agile_grasp_amd import binding

    lib = binding.load_library()
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    src = tmp_path / "sig.cpp"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_a_null_context_is_refused_without_a_device():
    """(the bad-argument paths need a context, hence a device: tests/test_gpu_localize_batch_stream.py)"""
    from agile_grasp_amd import binding

    lib = binding.load_library()
    ptrs, strides, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(12), (C.c_int64 * 1)(0)
    lps = (binding.AghLocalizeParams * 1)()
    res = (binding.AghLocalizeBatchResult * 1)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    assert lib.agh_localize_batch_begin(None, ptrs, strides, ns, lps, C.c_int32(1)) == bad
    assert lib.agh_localize_batch_begin_device(None, ptrs, strides, ns, lps, C.c_int32(1)) == bad
    assert lib.agh_localize_batch_stage(None, ptrs, strides, ns, C.c_int32(1)) == bad
    assert lib.agh_localize_batch_end(None, None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res) == bad


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "batch_stream_tu.cpp")])
    for hdr, names in (("hand_search.h", ("localizeBatchBegin", "localizeBatchStage", "localizeBatchEnd")),
                       ("localization.h", ("localizeHandlesBatchBegin", "stageNextBatch", "localizeHandlesBatchEnd"))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr
