"""agh_localize_masked / _device / _begin, agh_localize_depth_masked / _device / _begin and agh_get_sample_mask_count
(include/agh.h): declared with the documented signatures, exported by the library, refused without a context before any device
call, agh_sample_mask laid out as the binding's record, and the header's "Not built" sentence and mid-chain lists name what they
should.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_masked", "agh_localize_masked_device", "agh_localize_masked_begin", "agh_localize_depth_masked",
         "agh_localize_depth_masked_device", "agh_localize_depth_masked_begin", "agh_get_sample_mask_count")

SRC = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float*, int64_t, int64_t, const uint8_t*, const agh_localize_params*, agh_handle*, int64_t,
  int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_result*);
typedef int (*begin_fn)(agh_ctx*, const float*, int64_t, int64_t, const uint8_t*, const agh_localize_params*);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, const agh_sample_mask*, int32_t, const agh_localize_params*, agh_handle*,
  int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_result*);
typedef int (*depth_begin_fn)(agh_ctx*, const agh_depth_image*, const agh_sample_mask*, int32_t, const agh_localize_params*);
typedef int (*count_fn)(agh_ctx*, int64_t*);
static_assert(std::is_same<decltype(&agh_localize_masked), call_fn>::value, "agh_localize_masked");
static_assert(std::is_same<decltype(&agh_localize_masked_device), call_fn>::value, "agh_localize_masked_device");
static_assert(std::is_same<decltype(&agh_localize_masked_begin), begin_fn>::value, "agh_localize_masked_begin");
static_assert(std::is_same<decltype(&agh_localize_depth_masked), depth_call_fn>::value, "agh_localize_depth_masked");
static_assert(std::is_same<decltype(&agh_localize_depth_masked_device), depth_call_fn>::value, "agh_localize_depth_masked_device");
static_assert(std::is_same<decltype(&agh_localize_depth_masked_begin), depth_begin_fn>::value, "agh_localize_depth_masked_begin");
static_assert(std::is_same<decltype(&agh_get_sample_mask_count), count_fn>::value, "agh_get_sample_mask_count");
static_assert(std::is_same<decltype(agh_sample_mask::data), const uint8_t*>::value, "data");
static_assert(std::is_same<decltype(agh_sample_mask::row_stride_bytes), int64_t>::value, "row_stride_bytes");
int main()
{
  std::printf("%zu %zu %zu\n", sizeof(agh_sample_mask), offsetof(agh_sample_mask, data), offsetof(agh_sample_mask, row_stride_bytes));
  return 0;
}
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
    assert "typedef struct agh_sample_mask" in hdr
    src = tmp_path / "sig.cpp"
    src.write_text(SRC)
    exe = tmp_path / "sig"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    rec = binding.AghSampleMask
    assert got == [C.sizeof(rec), rec.data.offset, rec.row_stride_bytes.offset] == [16, 0, 8]


def test_header_names_what_is_not_built_and_what_is_refused_mid_chain():
    hdr = _header()
    block = hdr[hdr.index("The same chains with their samples drawn UNDER A MASK"):hdr.index("int agh_get_sample_mask_count(")]
    not_built = block[block.index("Not built:"):]
    for phrase in ("_stage call for masks", "agh_localize_batch*", "agh_localize_depth_batch*", "label images", "sharded variants"):
        assert phrase in not_built, phrase
    for phrase in ("never adopts a staged set", "INT32_MIN", "all NULL is AGH_ERR_INVALID_ARGUMENT", "n_samples = 0", "any byte alignment"):
        assert phrase in block, phrase
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    refused = single.split("may be called on the context")[1]
    for name in ("agh_localize_masked_begin", "agh_localize_depth_masked_begin", "agh_get_sample_mask_count"):
        assert name in refused and name not in single.split("may be called on the context")[0], name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("Sample masks"):]
    for phrase in ("k_mask_mark", "k_mask_emit", "k_draw_samples_masked", "Not built"):
        assert phrase in section, phrase


def test_the_new_source_file_is_built_with_the_others():
    from agile_grasp_amd import build

    assert "sample_mask.hip" in build.SRC and os.path.exists(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_mask.hip"))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = re.search(r"agile_grasp_amd/csrc/\{([a-z_,]+)\}\.hip", integration).group(1).split(",")
    assert listed == [f[:-len(".hip")] for f in build.SRC]  # the direct hipcc command names the files build.py compiles
    assert "sample_mask.hip" in integration


def test_a_null_context_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    mrecs = (binding.AghSampleMask * 1)()
    lp = binding.AghLocalizeParams()
    res = binding.AghLocalizeResult()
    m = C.c_int64(0)
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, C.byref(res))
    for fn in (lib.agh_localize_masked, lib.agh_localize_masked_device):
        assert fn(None, None, C.c_int64(12), C.c_int64(0), None, C.byref(lp), *outs) == bad
    assert lib.agh_localize_masked_begin(None, None, C.c_int64(12), C.c_int64(0), None, C.byref(lp)) == bad
    for fn in (lib.agh_localize_depth_masked, lib.agh_localize_depth_masked_device):
        assert fn(None, recs, mrecs, C.c_int32(1), C.byref(lp), *outs) == bad
    assert lib.agh_localize_depth_masked_begin(None, recs, mrecs, C.c_int32(1), C.byref(lp)) == bad
    assert lib.agh_get_sample_mask_count(None, C.byref(m)) == bad


def test_records_of_the_binding_carry_strides_and_nulls():
    import numpy as np

    from agile_grasp_amd import binding
    from tests import mask_cases as M

    images, masks, _ = M.depth_cases()["u16_odd_stride_first_null"]
    recs, keep = binding.sample_mask_records(masks, False)
    assert recs[0].data is None and recs[1].data == masks[1].ctypes.data and recs[1].row_stride_bytes == masks[1].strides[0]
    assert masks[1].strides[0] > masks[1].shape[1] and len(keep) == 2
    packed = M.packed_masks(images, masks)
    assert packed.dtype == np.uint8 and not packed[:images[0]["data"].size].any() and packed.any()
