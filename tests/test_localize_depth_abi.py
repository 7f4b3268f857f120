"""agh_deproject / agh_localize_depth / _device / _begin / _stage (include/agh.h): declared with the documented signatures, exported
by the library, refused without a context before any device call, agh_depth_image laid out as the binding's record, and the
adapter's new methods (HandSearch::localizeDepth / localizeDepthBegin / localizeDepthStage, Localization::localizeHandlesDepth /
localizeHandlesDepthBegin / stageNextDepth) compile in both type branches.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_deproject", "agh_localize_depth", "agh_localize_depth_device", "agh_localize_depth_begin", "agh_localize_depth_stage")

SRC = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "agh.h"
typedef int (*deproject_fn)(agh_ctx*, const agh_depth_image*, int32_t, float*, int64_t);
typedef int (*call_fn)(agh_ctx*, const agh_depth_image*, int32_t, const agh_localize_params*, agh_handle*, int64_t, int32_t*, int64_t,
  agh_hypothesis*, int64_t, int32_t*, agh_localize_result*);
typedef int (*begin_fn)(agh_ctx*, const agh_depth_image*, int32_t, const agh_localize_params*);
typedef int (*stage_fn)(agh_ctx*, const agh_depth_image*, int32_t);
static_assert(std::is_same<decltype(&agh_deproject), deproject_fn>::value, "agh_deproject");
static_assert(std::is_same<decltype(&agh_localize_depth), call_fn>::value, "agh_localize_depth");
static_assert(std::is_same<decltype(&agh_localize_depth_device), call_fn>::value, "agh_localize_depth_device");
static_assert(std::is_same<decltype(&agh_localize_depth_begin), begin_fn>::value, "agh_localize_depth_begin");
static_assert(std::is_same<decltype(&agh_localize_depth_stage), stage_fn>::value, "agh_localize_depth_stage");
static_assert(AGH_DEPTH_U16 == 0 && AGH_DEPTH_F32 == 1, "formats");
int main()
{
  std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(agh_depth_image), offsetof(agh_depth_image, data),
    offsetof(agh_depth_image, width), offsetof(agh_depth_image, height), offsetof(agh_depth_image, row_stride_bytes),
    offsetof(agh_depth_image, format), offsetof(agh_depth_image, depth_scale), offsetof(agh_depth_image, fx),
    offsetof(agh_depth_image, pose));
  return 0;
}
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
    exe = tmp_path / "sig"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    rec = binding.AghDepthImage
    want = [C.sizeof(rec)] + [getattr(rec, f).offset for f in ("data", "width", "height", "row_stride_bytes", "format", "depth_scale",
                                                               "fx", "pose")]
    assert got == want and C.sizeof(rec) == 160
    assert (binding.DEPTH_U16, binding.DEPTH_F32) == (0, 1)


def test_header_says_what_the_issue_asks_it_to_say():
    hdr = open(os.path.join(ROOT, "include", "agh.h")).read()
    block = hdr[hdr.index("The same chain straight from DEPTH IMAGES"):hdr.index("int agh_localize_depth_stage(")]
    for phrase in ("dense = 1", "camera id is its image's index", "does NOT set the camera origins", "quiet NaNs"):
        assert phrase in block, phrase
    allowed = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    assert "agh_localize_depth_stage" in allowed.split("may be called on the context")[0]
    assert "agh_deproject" in allowed.split("may be called on the context")[1]


def test_a_null_context_is_refused_without_a_device():
    """(the bad-argument paths need a context, hence a device: tests/test_gpu_localize_depth.py)"""
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    lp = binding.AghLocalizeParams()
    res = binding.AghLocalizeResult()
    out = (C.c_float * 3)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    assert lib.agh_deproject(None, recs, C.c_int32(1), out, C.c_int64(1)) == bad
    for fn in (lib.agh_localize_depth, lib.agh_localize_depth_device):
        assert fn(None, recs, C.c_int32(1), C.byref(lp), None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None,
                  C.byref(res)) == bad
    assert lib.agh_localize_depth_begin(None, recs, C.c_int32(1), C.byref(lp)) == bad
    assert lib.agh_localize_depth_stage(None, recs, C.c_int32(1)) == bad


def test_records_of_the_binding_carry_strides_formats_and_poses():
    import numpy as np

    from agile_grasp_amd import binding
    from tests import depth_captures as D

    images = D.edge_cases()["u16_odd_stride"] + D.edge_cases()["f32_padded"][:1]
    recs, keep, on_device = binding.depth_image_records(images[:2])
    assert not on_device and len(keep) == 2
    for r, im in zip(recs, images):
        d = im["data"]
        assert (r.width, r.height, r.row_stride_bytes, r.data) == (d.shape[1], d.shape[0], d.strides[0], d.ctypes.data)
        assert r.format == binding.DEPTH_U16 and r.depth_scale == np.float32(D.SCALE)
        assert np.array_equal(np.array(r.pose[:]), np.asarray(im["pose"]).reshape(12)) and r.fx == im["fx"] and r.cy == im["cy"]
    assert binding.depth_image_records(images[2:])[0][0].format == binding.DEPTH_F32


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "depth_tu.cpp")])
    for hdr, names in (("hand_search.h", ("localizeDepth", "localizeDepthBegin", "localizeDepthStage")),
                       ("localization.h", ("localizeHandlesDepth", "localizeHandlesDepthBegin", "stageNextDepth")),
                       ("types.h", ("struct DepthImage",))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr
