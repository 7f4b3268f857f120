"""agh_localize_batch_clustered / _device / _begin / _begin_device, agh_localize_depth_batch_clustered / _device / _begin /
_begin_device, agh_get_batch_cluster_info and agh_get_batch_cluster_labels (include/agh.h): declared with the documented
signatures, exported by the library and listed by the binding, refused without a context before any device call; the header's
numbered block, its mid-chain lists and DESIGN.md's subsection name what they should.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

CALLS = ("agh_localize_batch_clustered", "agh_localize_batch_clustered_device", "agh_localize_batch_clustered_begin",
         "agh_localize_batch_clustered_begin_device", "agh_localize_depth_batch_clustered", "agh_localize_depth_batch_clustered_device",
         "agh_localize_depth_batch_clustered_begin", "agh_localize_depth_batch_clustered_begin_device")
NAMES = CALLS + ("agh_get_batch_cluster_info", "agh_get_batch_cluster_labels")
KERNELS = ("k_cluster_init_batch", "k_cluster_link_batch", "k_cluster_flatten_batch", "k_cluster_select_batch", "k_cluster_mark_batch")
SINGLE = ("k_cluster_init", "k_cluster_link", "k_cluster_flatten", "k_cluster_select", "k_cluster_mark")

SRC = r"""
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const agh_cluster_params*,
  const agh_localize_params*, int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*,
  agh_localize_batch_result*);
typedef int (*begin_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const agh_cluster_params*,
  const agh_localize_params*, int32_t);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, const int32_t*, const agh_cluster_params*, const agh_localize_params*,
  int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*depth_begin_fn)(agh_ctx*, const agh_depth_image*, const int32_t*, const agh_cluster_params*, const agh_localize_params*,
  int32_t);
typedef int (*info_fn)(agh_ctx*, agh_cluster_info*, int64_t*, int32_t*, int32_t, int32_t);
typedef int (*labels_fn)(agh_ctx*, uint8_t*, int64_t);
static_assert(std::is_same<decltype(&agh_localize_batch_clustered), call_fn>::value, "agh_localize_batch_clustered");
static_assert(std::is_same<decltype(&agh_localize_batch_clustered_device), call_fn>::value, "agh_localize_batch_clustered_device");
static_assert(std::is_same<decltype(&agh_localize_batch_clustered_begin), begin_fn>::value, "agh_localize_batch_clustered_begin");
static_assert(std::is_same<decltype(&agh_localize_batch_clustered_begin_device), begin_fn>::value, "agh_localize_batch_clustered_begin_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered), depth_call_fn>::value, "agh_localize_depth_batch_clustered");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered_device), depth_call_fn>::value, "agh_localize_depth_batch_clustered_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered_begin), depth_begin_fn>::value, "agh_localize_depth_batch_clustered_begin");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered_begin_device), depth_begin_fn>::value,
  "agh_localize_depth_batch_clustered_begin_device");
static_assert(std::is_same<decltype(&agh_get_batch_cluster_info), info_fn>::value, "agh_get_batch_cluster_info");
static_assert(std::is_same<decltype(&agh_get_batch_cluster_labels), labels_fn>::value, "agh_get_batch_cluster_labels");
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
    for method in ("localize_batch_clustered", "localize_batch_clustered_begin", "localize_depth_batch_clustered",
                   "localize_depth_batch_clustered_begin", "batch_cluster_info", "batch_cluster_labels"):
        assert callable(getattr(binding.Context, method)), method


def test_a_null_context_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    n_images = (C.c_int32 * 1)(1)
    cp = binding.cluster_params()
    lp = binding.AghLocalizeParams()
    res = (binding.AghLocalizeBatchResult * 1)()
    info = (binding.AghClusterInfo * 64)()
    m, ids, labels = (C.c_int64 * 64)(), (C.c_int32 * 64)(), (C.c_uint8 * 16)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res)
    one = C.c_int32(1)
    for fn in (lib.agh_localize_batch_clustered, lib.agh_localize_batch_clustered_device):
        assert fn(None, None, None, None, C.byref(cp), C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_batch_clustered_begin, lib.agh_localize_batch_clustered_begin_device):
        assert fn(None, None, None, None, C.byref(cp), C.byref(lp), one) == bad
    for fn in (lib.agh_localize_depth_batch_clustered, lib.agh_localize_depth_batch_clustered_device):
        assert fn(None, recs, n_images, C.byref(cp), C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_depth_batch_clustered_begin, lib.agh_localize_depth_batch_clustered_begin_device):
        assert fn(None, recs, n_images, C.byref(cp), C.byref(lp), one) == bad
    assert lib.agh_get_batch_cluster_info(None, info, m, ids, C.c_int32(64), C.c_int32(64)) == bad
    assert lib.agh_get_batch_cluster_labels(None, labels, C.c_int64(16)) == bad


def test_header_block_and_mid_chain_lists():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_localize_batch_clustered*", "agh_localize_batch_clustered_begin*", "agh_localize_depth_batch_clustered*",
                 "agh_localize_depth_batch_clustered_begin*", "agh_get_batch_cluster_info", "agh_get_batch_cluster_labels"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    block = hdr[hdr.index("one sample list per CONNECTED COMPONENT of every capture's own cloud"):hdr.index("int agh_localize_batch_clustered(")]
    for k in range(1, 9):
        assert re.search(r"\n \* +%d\. " % k, block), k  # the numbered contract, 1 to 8
    block = re.sub(r"\n \*\s+", " ", block)  # (the comment's line breaks fall where they fall)
    for phrase in ("first_list", "exclusive prefix sum", "L <= 64", "2^24", "cp[k].max_objects", "CAPTURE-LOCAL",
                   "No pair is ever formed across captures", "its own grid descriptor and cp[k].tolerance", "agh_localize_clustered",
                   "agh_localize_depth_clustered", "agh_localize_batch_labeled", "AGH_NORMALS_RAND50", "only list 0",
                   "order of an atomic", "cp == NULL", "naming the capture and the field", "lp[k].sample_idx != NULL",
                   "per CAPTURE, not per list", "capture k, object j", "AGH_ERR_CAPACITY with every results[l] filled",
                   "S_k = 0", "agh_localize_batch_end", "never adopts a staged set", "with the cp records the chain holds",
                   "agh_get_cloud's order", "two 32-bit words and a byte per raw point", "four 64-bit counters per capture",
                   "4 words per capture plus 2 per list", "with n_captures x 64"):
        assert phrase in block, phrase
    for getter in ("agh_get_sample_mask_count", "agh_get_label_counts", "agh_get_cluster_info", "agh_get_cluster_labels",
                   "agh_get_batch_mask_counts", "agh_get_batch_label_counts"):  # the six that answer AGH_ERR_STATE afterwards
        assert getter in block[block.index("After a clustered batch"):], getter
    not_built = block[block.index("Not built:"):]
    for phrase in ("_stage call", "more than 64 lists", "fitted plane", "mixed with labelled, masked or unmasked", "sharded forms"):
        assert phrase in not_built, phrase
    # the single-capture block says where the batch forms are
    older = hdr[hdr.index("WITHOUT A SEGMENTER"):hdr.index("typedef struct agh_cluster_params")]
    assert "agh_localize_batch_clustered*" in older[older.index("Not built:"):]


def test_design_and_sources_name_the_stage():
    from agile_grasp_amd import build

    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("Clusters in the batch chains"):]
    for phrase in NAMES[:1] + ("agh_localize_depth_batch_clustered", "agh_get_batch_cluster_info", "agh_get_batch_cluster_labels") + KERNELS + (
            "sample_cluster_stage_batch", "label_compact_stage_batch", "cloud_off", "raw_off", "Not built"):
        assert phrase in section, phrase
    older = design[design.index("Clusters as the label source"):design.index("Clusters in the batch chains")]
    assert "agh_localize_batch_clustered" in older[older.index("Not built"):]
    src = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_cluster.hip")).read()
    for kernel in KERNELS + SINGLE:  # both forms are kernels of their own, around the shared bodies
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", src), kernel
    for body in ("cluster_init_voxel", "cluster_link_groups", "cluster_flatten_voxel", "cluster_select_roots", "cluster_mark_voxel"):
        assert len(re.findall(r"__device__ __forceinline__ void " + body + r"\(", src)) == 1, body  # moved, not copied
        assert len(re.findall(r"\b" + body + r"\(", src)) == 3, body  # defined once, called by the two forms
    labels = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_labels.hip")).read()
    assert re.search(r"\bint label_compact_stage_batch\(", labels) and "return label_compact_stage_batch(c, m, any, st);" in labels
    assert len(re.findall(r"hipLaunchKernelGGL\(k_label_emit_batch", labels)) == 1
    batch = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "localize_batch.hip")).read()
    assert "sample_cluster_stage_batch(c, m, b->d_ccap, st)" in batch
    # the batch keeps a copy of the records for a repeat of the pass: in the stored source, which the single chain keeps too
    internal = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "agh_internal.h")).read()
    assert "std::vector<agh_cluster_params> cluster;" in internal[internal.index("struct StoredSource"):internal.index("struct LocalizeState")]
    assert "StoredSource source;" in batch[batch.index("struct BatchCall"):batch.index("struct LocalizeBatchState")]
    assert "sample_cluster.hip" in build.SRC
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("agh_localize_batch_clustered", "agh_localize_depth_batch_clustered", "localizeHandlesBatchClustered"):
        assert name in integration, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "agh_localize_batch_clustered" in readme
    notes = open(os.path.join(ROOT, "profiles", "NOTES.md")).read()
    assert "k_cluster_link_batch" in notes and "k_cluster_select_batch" in notes
