"""agh_localize_batch_masked / _device / _begin / _begin_device, agh_localize_depth_batch_masked / _device / _begin /
_begin_device and agh_get_batch_mask_counts (include/agh.h): declared with the documented signatures, exported by the library and
listed by the binding, refused without a context before any device call; the header's mid-chain lists and "Not built" sentences
and DESIGN.md's subsection name what they should.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_batch_masked", "agh_localize_batch_masked_device", "agh_localize_batch_masked_begin",
         "agh_localize_batch_masked_begin_device", "agh_localize_depth_batch_masked", "agh_localize_depth_batch_masked_device",
         "agh_localize_depth_batch_masked_begin", "agh_localize_depth_batch_masked_begin_device", "agh_get_batch_mask_counts")

SRC = r"""
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const uint8_t* const*, const agh_localize_params*,
  int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*begin_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const uint8_t* const*, const agh_localize_params*,
  int32_t);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, const agh_sample_mask*, const int32_t*, const agh_localize_params*,
  int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*depth_begin_fn)(agh_ctx*, const agh_depth_image*, const agh_sample_mask*, const int32_t*, const agh_localize_params*,
  int32_t);
typedef int (*counts_fn)(agh_ctx*, int64_t*, int32_t);
static_assert(std::is_same<decltype(&agh_localize_batch_masked), call_fn>::value, "agh_localize_batch_masked");
static_assert(std::is_same<decltype(&agh_localize_batch_masked_device), call_fn>::value, "agh_localize_batch_masked_device");
static_assert(std::is_same<decltype(&agh_localize_batch_masked_begin), begin_fn>::value, "agh_localize_batch_masked_begin");
static_assert(std::is_same<decltype(&agh_localize_batch_masked_begin_device), begin_fn>::value, "agh_localize_batch_masked_begin_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_masked), depth_call_fn>::value, "agh_localize_depth_batch_masked");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_masked_device), depth_call_fn>::value, "agh_localize_depth_batch_masked_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_masked_begin), depth_begin_fn>::value, "agh_localize_depth_batch_masked_begin");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_masked_begin_device), depth_begin_fn>::value,
  "agh_localize_depth_batch_masked_begin_device");
static_assert(std::is_same<decltype(&agh_get_batch_mask_counts), counts_fn>::value, "agh_get_batch_mask_counts");
int main() { return 0; }
"""


def _header():
    return open(os.path.join(ROOT, "include", "agh.h")).read()


def test_header_declares_and_library_exports_the_calls(tmp_path):
    hdr = _header()
    from agile_grasp_amd import binding

    lib = binding.load_library()
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    src = tmp_path / "sig.cpp"
    src.write_text(SRC)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    for method in ("localize_batch_masked", "localize_batch_masked_begin", "localize_depth_batch_masked",
                   "localize_depth_batch_masked_begin", "batch_mask_counts"):
        assert callable(getattr(binding.Context, method)), method


def test_a_null_context_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    mrecs = (binding.AghSampleMask * 1)()
    n_images = (C.c_int32 * 1)(1)
    lp = binding.AghLocalizeParams()
    res = (binding.AghLocalizeBatchResult * 1)()
    m = (C.c_int64 * 64)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res)
    one = C.c_int32(1)
    for fn in (lib.agh_localize_batch_masked, lib.agh_localize_batch_masked_device):
        assert fn(None, None, None, None, None, C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_batch_masked_begin, lib.agh_localize_batch_masked_begin_device):
        assert fn(None, None, None, None, None, C.byref(lp), one) == bad
    for fn in (lib.agh_localize_depth_batch_masked, lib.agh_localize_depth_batch_masked_device):
        assert fn(None, recs, mrecs, n_images, C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_depth_batch_masked_begin, lib.agh_localize_depth_batch_masked_begin_device):
        assert fn(None, recs, mrecs, n_images, C.byref(lp), one) == bad
    assert lib.agh_get_batch_mask_counts(None, m, C.c_int32(64)) == bad


def test_header_names_what_is_refused_mid_chain_and_what_is_not_built():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_localize_batch_masked*", "agh_localize_batch_masked_begin*", "agh_localize_depth_batch_masked*",
                 "agh_localize_depth_batch_masked_begin*", "agh_get_batch_mask_counts"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    block = hdr[hdr.index("The batch chains with every capture's samples drawn UNDER ITS OWN MASK"):hdr.index("int agh_localize_batch_masked(")]
    not_built = block[block.index("Not built:"):]
    for phrase in ("_stage call for masks", "label images in the batch", "mixed in one batch", "sharded variants"):
        assert phrase in not_built, phrase
    for phrase in ("CAPTURE-LOCAL", "INT32_MIN", "agh_localize_batch_end", "never adopts a staged set", "any byte alignment",
                   "n_samples = 0", "AGH_ERR_CAPACITY if cap_captures", "naming the capture"):
        assert phrase in block, phrase
    # the single form's block no longer says that the batch masks are missing, and says where they are
    masks = hdr[hdr.index("The same chains with their samples drawn UNDER A MASK"):hdr.index("int agh_get_sample_mask_count(")]
    old = masks[masks.index("Not built:"):]
    assert "masks for agh_localize_batch*" not in old and "agh_localize_batch_masked*" in old


def test_design_and_integration_name_the_stage():
    from agile_grasp_amd import build

    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("Sample masks in the batch chains"):]
    for phrase in ("k_mask_mark_batch", "k_mask_scan_batch", "k_mask_emit_batch", "k_batch_samples_masked", "raw_off", "repacked",
                   "agh_get_batch_mask_counts"):
        assert phrase in section, phrase
    assert "one byte and one 32-bit word per raw point" in design
    src = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_mask.hip")).read()
    for kernel in ("k_mask_mark_batch", "k_mask_scan_batch", "k_mask_emit_batch", "k_batch_samples_masked"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", src), kernel
    assert "sample_mask.hip" in build.SRC
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("agh_localize_batch_masked", "agh_localize_depth_batch_masked", "localizeHandlesBatchMasked"):
        assert name in integration, name
