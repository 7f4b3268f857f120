"""agh_localize_labeled / _device, agh_localize_depth_labeled / _device and agh_get_label_counts (include/agh.h): declared with
the documented signatures, exported by the library, refused without a context before any device call, agh_label_image laid out
as the binding's record, and the header's "Not built" sentences and mid-chain lists name what they should.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_labeled", "agh_localize_labeled_device", "agh_localize_depth_labeled", "agh_localize_depth_labeled_device",
         "agh_get_label_counts")

SRC = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float*, int64_t, int64_t, const uint8_t*, int32_t, const agh_localize_params*, agh_handle*,
  int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, const agh_label_image*, int32_t, int32_t, const agh_localize_params*,
  agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*counts_fn)(agh_ctx*, int64_t*, int32_t);
static_assert(std::is_same<decltype(&agh_localize_labeled), call_fn>::value, "agh_localize_labeled");
static_assert(std::is_same<decltype(&agh_localize_labeled_device), call_fn>::value, "agh_localize_labeled_device");
static_assert(std::is_same<decltype(&agh_localize_depth_labeled), depth_call_fn>::value, "agh_localize_depth_labeled");
static_assert(std::is_same<decltype(&agh_localize_depth_labeled_device), depth_call_fn>::value, "agh_localize_depth_labeled_device");
static_assert(std::is_same<decltype(&agh_get_label_counts), counts_fn>::value, "agh_get_label_counts");
static_assert(std::is_same<decltype(agh_label_image::data), const uint8_t*>::value, "data");
static_assert(std::is_same<decltype(agh_label_image::row_stride_bytes), int64_t>::value, "row_stride_bytes");
int main()
{
  std::printf("%zu %zu %zu\n", sizeof(agh_label_image), offsetof(agh_label_image, data), offsetof(agh_label_image, row_stride_bytes));
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
    assert "typedef struct agh_label_image" in hdr
    src = tmp_path / "sig.cpp"
    src.write_text(SRC)
    exe = tmp_path / "sig"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    rec = binding.AghLabelImage
    assert got == [C.sizeof(rec), rec.data.offset, rec.row_stride_bytes.offset] == [16, 0, 8]
    # the header is a C header: the labelled block names the batch result record ahead of its definition
    csrc = tmp_path / "c.c"
    csrc.write_text('#include "agh.h"\nint main(void) { return sizeof(agh_label_image) == 16 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(csrc), "-o",
                           str(tmp_path / "c")])


def test_header_names_what_is_not_built_and_what_is_refused_mid_chain():
    hdr = _header()
    block = hdr[hdr.index("one sample list PER OBJECT of a LABEL IMAGE"):hdr.index("int agh_get_label_counts(")]
    not_built = block[block.index("Not built:"):block.index("typedef struct agh_label_image")]
    for phrase in ("_begin / _end and _stage forms", "labels in the batch chains", "more than 64 objects", "wider than a byte",
                   "sharded variants"):
        assert phrase in not_built, phrase
    for phrase in ("1 <= n_objects <= 64", "2^24", "INT32_MIN", "AGH_NORMALS_RAND50", "only object 0", "all NULL is AGH_ERR_INVALID_ARGUMENT",
                   "any byte alignment", "single bound cloud", "AGH_ERR_CAPACITY with every results[j] filled"):
        assert phrase in block, phrase
    masked = hdr[hdr.index("The same chains with their samples drawn UNDER A MASK"):hdr.index("int agh_get_sample_mask_count(")]
    assert "label images in the batch" in masked[masked.index("Not built:"):]
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    refused = single.split("may be called on the context")[1]
    for name in ("agh_localize_labeled*", "agh_localize_depth_labeled*", "agh_get_label_counts"):
        assert name in refused and name not in single.split("may be called on the context")[0], name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("Label images"):]
    for phrase in ("k_vox_word_rank", "k_label_mark", "k_label_count", "k_label_scan", "k_label_emit", "k_draw_samples_labeled",
                   "RAND50", "Not built"):
        assert phrase in section, phrase


def test_the_new_source_file_is_built_with_the_others():
    from agile_grasp_amd import build

    assert "sample_labels.hip" in build.SRC and os.path.exists(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_labels.hip"))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = re.search(r"agile_grasp_amd/csrc/\{([a-z_,]+)\}\.hip", integration).group(1).split(",")
    assert listed == [f[:-len(".hip")] for f in build.SRC]  # the direct hipcc command names the files build.py compiles
    assert "agh_localize_labeled" in integration


def test_a_null_context_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    lrecs = (binding.AghLabelImage * 1)()
    lp = binding.AghLocalizeParams()
    res = (binding.AghLocalizeBatchResult * 2)()
    m = (C.c_int64 * 2)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res)
    for fn in (lib.agh_localize_labeled, lib.agh_localize_labeled_device):
        assert fn(None, None, C.c_int64(12), C.c_int64(0), None, C.c_int32(2), C.byref(lp), *outs) == bad
    for fn in (lib.agh_localize_depth_labeled, lib.agh_localize_depth_labeled_device):
        assert fn(None, recs, lrecs, C.c_int32(1), C.c_int32(2), C.byref(lp), *outs) == bad
    assert lib.agh_get_label_counts(None, m, C.c_int32(2)) == bad


def test_records_and_sample_lists_of_the_binding():
    import numpy as np

    from agile_grasp_amd import binding
    from tests import label_cases as L

    wide = np.ones((4, 9), np.uint8)
    recs, keep = binding.label_image_records([None, wide[:, :6]], False)
    assert recs[0].data is None and recs[1].data == wide.ctypes.data and recs[1].row_stride_bytes == 9 and len(keep) == 2
    c = L.point_cases()["dropped"]
    E = L.eligible_lists(c)
    got = binding.labeled_samples(E, 3, 5)
    assert got.dtype == np.int32 and len(got) == 9
    for j in range(3):
        assert np.array_equal(got[3 * j:3 * j + 3], binding.masked_samples(E[j], 3, 5))
    assert (got[3:6] == -(1 << 31)).all() and len(binding.labeled_samples(E, 0, 5)) == 0
