"""agh_localize_batch / agh_localize_batch_device (include/agh.h): declared in the header, exported by the library, and the
ctypes mirror of agh_localize_batch_result in binding.py has the header's size and offsets.  Needs no GPU."""
import ctypes
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

SRC = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "agh.h"
int main()
{
  std::printf("%zu %zu %zu %zu %zu %zu\n", sizeof(agh_localize_batch_result), offsetof(agh_localize_batch_result, r),
    offsetof(agh_localize_batch_result, first_handle), offsetof(agh_localize_batch_result, first_inlier_idx),
    offsetof(agh_localize_batch_result, first_hand), offsetof(agh_localize_batch_result, first_sample));
  return 0;
}
typedef int (*batch_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const agh_localize_params*, int32_t,
  agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
static_assert(std::is_same<decltype(&agh_localize_batch), batch_fn>::value, "agh_localize_batch");
static_assert(std::is_same<decltype(&agh_localize_batch_device), batch_fn>::value, "agh_localize_batch_device");
"""


def test_header_declares_and_library_exports_the_batch_calls():
    hdr = open(os.path.join(ROOT, "include", "agh.h")).read()
    for fn in ("agh_localize_batch", "agh_localize_batch_device"):
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    from agile_grasp_amd import binding

    lib = binding.load_library()
    assert hasattr(lib, "agh_localize_batch") and hasattr(lib, "agh_localize_batch_device")
    assert "agh_localize_batch" in binding.EXPORTS and "agh_localize_batch_device" in binding.EXPORTS


def test_batch_result_mirror_matches_the_header(tmp_path):
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                          stdout=subprocess.DEVNULL)
    size, off_r, off_h, off_i, off_k, off_s = (int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split())
    from agile_grasp_amd.binding import AghLocalizeBatchResult, AghLocalizeResult

    assert ctypes.sizeof(AghLocalizeBatchResult) == size == ctypes.sizeof(AghLocalizeResult) + 32
    assert AghLocalizeBatchResult.r.offset == off_r == 0
    assert (AghLocalizeBatchResult.first_handle.offset, AghLocalizeBatchResult.first_inlier_idx.offset,
            AghLocalizeBatchResult.first_hand.offset, AghLocalizeBatchResult.first_sample.offset) == (off_h, off_i, off_k, off_s)


def test_adapter_compiles_with_localize_handles_batch(tmp_path):
    """include/agile_grasp_amd/localization.h declares Localization::localizeHandlesBatch: the adapter test builds against it
    with a plain g++ (as tests/test_cpp_adapter.py builds the other adapter tests)."""
    src = os.path.join(ROOT, "tests", "cpp", "localize_batch_test.cpp")
    assert "localizeHandlesBatch" in open(os.path.join(ROOT, "include", "agile_grasp_amd", "localization.h")).read()
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                           src, "-o", str(tmp_path / "localize_batch_test.o")])
