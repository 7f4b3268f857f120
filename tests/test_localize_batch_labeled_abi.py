"""agh_localize_batch_labeled / _device / _begin / _begin_device, agh_localize_depth_batch_labeled / _device / _begin /
_begin_device and agh_get_batch_label_counts (include/agh.h): declared with the documented signatures, exported by the library
and listed by the binding, refused without a context before any device call; the header's numbered block, its mid-chain lists
and DESIGN.md's subsection name what they should.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_batch_labeled", "agh_localize_batch_labeled_device", "agh_localize_batch_labeled_begin",
         "agh_localize_batch_labeled_begin_device", "agh_localize_depth_batch_labeled", "agh_localize_depth_batch_labeled_device",
         "agh_localize_depth_batch_labeled_begin", "agh_localize_depth_batch_labeled_begin_device", "agh_get_batch_label_counts")
KERNELS = ("k_vox_word_rank_batch", "k_label_mark_batch", "k_label_count_batch", "k_label_emit_batch", "k_batch_samples_labeled")

SRC = r"""
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const uint8_t* const*, const int32_t*,
  const agh_localize_params*, int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*,
  agh_localize_batch_result*);
typedef int (*begin_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const uint8_t* const*, const int32_t*,
  const agh_localize_params*, int32_t);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, const agh_label_image*, const int32_t*, const int32_t*,
  const agh_localize_params*, int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*,
  agh_localize_batch_result*);
typedef int (*depth_begin_fn)(agh_ctx*, const agh_depth_image*, const agh_label_image*, const int32_t*, const int32_t*,
  const agh_localize_params*, int32_t);
typedef int (*counts_fn)(agh_ctx*, int64_t*, int32_t);
static_assert(std::is_same<decltype(&agh_localize_batch_labeled), call_fn>::value, "agh_localize_batch_labeled");
static_assert(std::is_same<decltype(&agh_localize_batch_labeled_device), call_fn>::value, "agh_localize_batch_labeled_device");
static_assert(std::is_same<decltype(&agh_localize_batch_labeled_begin), begin_fn>::value, "agh_localize_batch_labeled_begin");
static_assert(std::is_same<decltype(&agh_localize_batch_labeled_begin_device), begin_fn>::value, "agh_localize_batch_labeled_begin_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_labeled), depth_call_fn>::value, "agh_localize_depth_batch_labeled");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_labeled_device), depth_call_fn>::value, "agh_localize_depth_batch_labeled_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_labeled_begin), depth_begin_fn>::value, "agh_localize_depth_batch_labeled_begin");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_labeled_begin_device), depth_begin_fn>::value,
  "agh_localize_depth_batch_labeled_begin_device");
static_assert(std::is_same<decltype(&agh_get_batch_label_counts), counts_fn>::value, "agh_get_batch_label_counts");
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
    csrc = tmp_path / "c.c"  # (the header stays a C header)
    csrc.write_text('#include "agh.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])
    for method in ("localize_batch_labeled", "localize_batch_labeled_begin", "localize_depth_batch_labeled",
                   "localize_depth_batch_labeled_begin", "batch_label_counts"):
        assert callable(getattr(binding.Context, method)), method
    assert callable(binding.batch_labeled_samples)


def test_the_numpy_helper_concatenates_the_captures_lists():
    import numpy as np

    from agile_grasp_amd import binding

    E = [[np.arange(5, 50, 3), np.zeros(0, np.int32)], [np.array([4, 9])]]
    got = binding.batch_labeled_samples(E, [4, 3], [7, 8])
    want = np.concatenate([binding.masked_samples(E[0][0], 4, 7), binding.masked_samples(E[0][1], 4, 7), binding.masked_samples(E[1][0], 3, 8)])
    assert np.array_equal(got, want) and got.tolist()[4:8] == [-(1 << 31)] * 4 and got.tolist()[8:] == [4, 9, -(1 << 31)]
    assert len(binding.batch_labeled_samples(E, 0, 1)) == 0


def test_a_null_context_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    lrecs = (binding.AghLabelImage * 1)()
    n_images = (C.c_int32 * 1)(1)
    n_objects = (C.c_int32 * 1)(1)
    lp = binding.AghLocalizeParams()
    res = (binding.AghLocalizeBatchResult * 1)()
    m = (C.c_int64 * 64)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res)
    one = C.c_int32(1)
    for fn in (lib.agh_localize_batch_labeled, lib.agh_localize_batch_labeled_device):
        assert fn(None, None, None, None, None, n_objects, C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_batch_labeled_begin, lib.agh_localize_batch_labeled_begin_device):
        assert fn(None, None, None, None, None, n_objects, C.byref(lp), one) == bad
    for fn in (lib.agh_localize_depth_batch_labeled, lib.agh_localize_depth_batch_labeled_device):
        assert fn(None, recs, lrecs, n_images, n_objects, C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_depth_batch_labeled_begin, lib.agh_localize_depth_batch_labeled_begin_device):
        assert fn(None, recs, lrecs, n_images, n_objects, C.byref(lp), one) == bad
    assert lib.agh_get_batch_label_counts(None, m, C.c_int32(64)) == bad


def test_header_block_and_mid_chain_lists():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_localize_batch_labeled*", "agh_localize_batch_labeled_begin*", "agh_localize_depth_batch_labeled*",
                 "agh_localize_depth_batch_labeled_begin*", "agh_get_batch_label_counts"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    block = hdr[hdr.index("one sample list PER OBJECT of every capture's LABEL IMAGE"):hdr.index("int agh_localize_batch_labeled(")]
    for k in range(1, 11):
        assert re.search(r"\n \* +%d\. " % k, block), k  # the numbered contract, 1 to 10
    for phrase in ("first_list", "exclusive prefix sum", "L <= 64", "2^24", "names the capture", "CAPTURE-LOCAL", "INT32_MIN",
                   "capture k, object j", "AGH_ERR_CAPACITY with every results[l] filled", "AGH_NORMALS_RAND50", "only list 0",
                   "agh_localize_labeled", "agh_localize_depth_labeled", "per CAPTURE, not per list", "agh_localize_batch_end",
                   "never adopts a staged set", "any byte alignment", "AGH_ERR_CAPACITY if cap_lists < L", "ceil(n_max / 256)"):
        assert phrase in block, phrase
    not_built = block[block.index("Not built:"):]
    for phrase in ("more than 64 lists per call", "wider than a byte", "_stage call for labels", "mixed in one batch", "sharded variants"):
        assert phrase in not_built, phrase
    # the older blocks say where the batch forms are
    labelled = hdr[hdr.index("one sample list PER OBJECT of a LABEL IMAGE"):hdr.index("int agh_get_label_counts(")]
    assert "agh_localize_batch_labeled*" in labelled[labelled.index("Not built:"):]
    masked = hdr[hdr.index("The batch chains with every capture's samples drawn UNDER ITS OWN MASK"):hdr.index("int agh_localize_batch_masked(")]
    assert "agh_localize_batch_labeled*" in masked[masked.index("Not built:"):]


def test_design_and_integration_name_the_stage():
    from agile_grasp_amd import build

    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("Label images in the batch chains"):]
    for phrase in KERNELS + ("k_label_scan", "first_list", "raw_off", "agh_get_batch_label_counts", "Not built"):
        assert phrase in section, phrase
    src = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_labels.hip")).read()
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", src), kernel
    assert "sample_labels.hip" in build.SRC
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("agh_localize_batch_labeled", "agh_localize_depth_batch_labeled", "localizeHandlesBatchLabeled"):
        assert name in integration, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "agh_localize_batch_labeled" in readme
