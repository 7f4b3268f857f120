"""agh_localize_params::filters_boundaries (include/agh.h) took the place of the unused `reserved` word: same offset, same
struct size, and the ctypes mirror in binding.py agrees.  Needs no GPU."""
import ctypes
import os
import subprocess

from tests.test_cpp_adapter import ROOT

SRC = r"""
#include <cstddef>
#include <cstdio>
#include "agh.h"
int main()
{
  std::printf("%zu %zu %zu %zu\n", offsetof(agh_localize_params, filters_boundaries), sizeof(agh_localize_params),
    offsetof(agh_localize_params, min_inliers), offsetof(agh_localize_params, min_length));
  return 0;
}
"""


def test_filters_boundaries_sits_where_reserved_was(tmp_path):
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    off, size, off_inl, off_len = (int(v) for v in subprocess.check_output([exe], text=True).split())
    assert (off, size) == (100, 112)
    assert (off_inl, off_len) == (96, 104)  # its neighbours stay put

    from agile_grasp_amd.binding import AghLocalizeParams

    assert AghLocalizeParams.filters_boundaries.offset == off
    assert ctypes.sizeof(AghLocalizeParams) == size
    assert AghLocalizeParams.min_length.offset == off_len
    lp = AghLocalizeParams()
    assert lp.filters_boundaries == 0  # ctypes zero-initialises: today's behaviour unless asked for
