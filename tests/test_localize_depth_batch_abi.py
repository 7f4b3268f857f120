"""agh_localize_depth_batch / _device / _begin / _begin_device and agh_deproject_batch (include/agh.h): declared with the
documented signatures, exported by the library (with the kernel k_deproject_batch), refused without a context before any device
call, carried by the binding as one flat record array with n_images, and the adapter's new methods compile in both type
branches.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_depth_batch", "agh_localize_depth_batch_device", "agh_localize_depth_batch_begin",
         "agh_localize_depth_batch_begin_device", "agh_deproject_batch")

SRC = r"""
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const agh_depth_image*, const int32_t*, const agh_localize_params*, int32_t, agh_handle*, int64_t,
  int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*begin_fn)(agh_ctx*, const agh_depth_image*, const int32_t*, const agh_localize_params*, int32_t);
typedef int (*deproject_fn)(agh_ctx*, const agh_depth_image*, const int32_t*, int32_t, float*, int64_t);
static_assert(std::is_same<decltype(&agh_localize_depth_batch), call_fn>::value, "agh_localize_depth_batch");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_device), call_fn>::value, "agh_localize_depth_batch_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_begin), begin_fn>::value, "agh_localize_depth_batch_begin");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_begin_device), begin_fn>::value, "agh_localize_depth_batch_begin_device");
static_assert(std::is_same<decltype(&agh_deproject_batch), deproject_fn>::value, "agh_deproject_batch");
int main() { return 0; }
"""


def test_header_declares_and_library_exports_the_calls(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "agh.h")).read()
    from agile_grasp_amd import binding

    lib = binding.load_library()
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    assert hasattr(lib, "k_deproject_batch") and hasattr(lib, "k_deproject")  # (the kernels' host-side handles)
    src = tmp_path / "sig.cpp"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "agh.h")).read()
    block = hdr[hdr.index("The batch chain straight from DEPTH IMAGES"):hdr.index("int agh_localize_depth_batch(")]
    for phrase in ("n_images[k] is 1 or 2", "bit for bit", "agh_localize_depth returns for capture k's images alone",
                   "size_left = W0 x H0", "dense = 1", "the poses do NOT set them", "capture 3, image 1: fx must",
                   "n_captures outside 1..64", "2^30 points or more", "AGH_ERR_CAPACITY with every results[k] filled",
                   "Not built: a _stage call for depth batches", "mixed in one batch", "agh_localize_batch_end"):
        assert phrase in " ".join(block.split()).replace(" * ", " "), phrase
    refused = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    refused = refused.split("may be called on the context")[1]
    assert "agh_deproject_batch" in refused and "agh_localize_depth_batch" in refused
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set"):hdr.index("int agh_localize_batch_begin(")]
    assert "agh_localize_depth_batch" in batch and "agh_deproject_batch" in batch


def test_a_null_context_is_refused_without_a_device():
    """(the bad-argument paths need a context, hence a device: tests/test_gpu_localize_depth_batch.py)"""
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    n_images = (C.c_int32 * 1)(1)
    lp = (binding.AghLocalizeParams * 1)()
    res = (binding.AghLocalizeBatchResult * 1)()
    out = (C.c_float * 3)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    assert lib.agh_deproject_batch(None, recs, n_images, C.c_int32(1), out, C.c_int64(1)) == bad
    for fn in (lib.agh_localize_depth_batch, lib.agh_localize_depth_batch_device):
        assert fn(None, recs, n_images, lp, C.c_int32(1), None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res) == bad
    for fn in (lib.agh_localize_depth_batch_begin, lib.agh_localize_depth_batch_begin_device):
        assert fn(None, recs, n_images, lp, C.c_int32(1)) == bad


def test_the_binding_carries_the_captures_in_order():
    from agile_grasp_amd import binding
    from tests import depth_batch_captures as DB

    caps = DB.edge_batch()
    recs, n_images, keep, on_device = binding.Context.depth_batch_records(caps)
    flat = [im for c in caps for im in c]
    assert not on_device and len(recs) == len(flat) == len(keep) and list(n_images) == [len(c) for c in caps]
    assert set(n_images) == {1, 2}
    for r, im in zip(recs, flat):
        d = im["data"]
        assert (r.width, r.height, r.row_stride_bytes, r.data) == (d.shape[1], d.shape[0], d.strides[0], d.ctypes.data)
        assert r.format == (binding.DEPTH_U16 if d.dtype == np.uint16 else binding.DEPTH_F32)
        assert r.depth_scale == np.float32(im["depth_scale"]) and r.fx == im["fx"] and r.cy == im["cy"]
        assert np.array_equal(np.array(r.pose[:]), np.asarray(im["pose"]).reshape(12))
    for name in ("localize_depth_batch", "localize_depth_batch_begin", "deproject_batch"):
        assert callable(getattr(binding.Context, name))


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "depth_batch_tu.cpp")])
    for hdr, names in (("hand_search.h", ("localizeDepthBatch", "localizeDepthBatchBegin")),
                       ("localization.h", ("localizeHandlesDepthBatch", "localizeHandlesDepthBatchBegin"))):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in names), hdr
