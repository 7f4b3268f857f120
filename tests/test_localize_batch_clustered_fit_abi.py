"""agh_localize_batch_clustered_fit / _device / _begin / _begin_device, agh_localize_depth_batch_clustered_fit / _device / _begin /
_begin_device, agh_get_batch_plane_fit and agh_get_batch_plane_fit_candidates (include/agh.h): declared with the documented
signatures, exported by the library and listed by the binding, refused without a context before any device call; the header's
numbered block carries its phrases, the older blocks and the documents point to the new calls, and the kernels were moved, not
copied.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

CALLS = ("agh_localize_batch_clustered_fit", "agh_localize_batch_clustered_fit_device", "agh_localize_batch_clustered_fit_begin",
         "agh_localize_batch_clustered_fit_begin_device", "agh_localize_depth_batch_clustered_fit",
         "agh_localize_depth_batch_clustered_fit_device", "agh_localize_depth_batch_clustered_fit_begin",
         "agh_localize_depth_batch_clustered_fit_begin_device")
NAMES = CALLS + ("agh_get_batch_plane_fit", "agh_get_batch_plane_fit_candidates")
KERNELS = ("k_fit_candidates_batch", "k_fit_score_batch", "k_fit_moments_batch", "k_fit_finish_batch")
SINGLE = ("k_fit_candidates", "k_fit_score", "k_fit_moments", "k_fit_finish")
BODIES = ("fit_candidates", "fit_score", "fit_moments", "fit_finish")

SRC = r"""
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const agh_plane_fit_params*,
  const agh_cluster_params*, const agh_localize_params*, int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t,
  int32_t*, agh_localize_batch_result*);
typedef int (*begin_fn)(agh_ctx*, const float* const*, const int64_t*, const int64_t*, const agh_plane_fit_params*,
  const agh_cluster_params*, const agh_localize_params*, int32_t);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, const int32_t*, const agh_plane_fit_params*, const agh_cluster_params*,
  const agh_localize_params*, int32_t, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*,
  agh_localize_batch_result*);
typedef int (*depth_begin_fn)(agh_ctx*, const agh_depth_image*, const int32_t*, const agh_plane_fit_params*, const agh_cluster_params*,
  const agh_localize_params*, int32_t);
typedef int (*fit_fn)(agh_ctx*, agh_plane_fit_result*, int32_t);
typedef int (*cand_fn)(agh_ctx*, int32_t, int32_t*, double*, int64_t*, int32_t);
static_assert(std::is_same<decltype(&agh_localize_batch_clustered_fit), call_fn>::value, "agh_localize_batch_clustered_fit");
static_assert(std::is_same<decltype(&agh_localize_batch_clustered_fit_device), call_fn>::value, "agh_localize_batch_clustered_fit_device");
static_assert(std::is_same<decltype(&agh_localize_batch_clustered_fit_begin), begin_fn>::value, "agh_localize_batch_clustered_fit_begin");
static_assert(std::is_same<decltype(&agh_localize_batch_clustered_fit_begin_device), begin_fn>::value,
  "agh_localize_batch_clustered_fit_begin_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered_fit), depth_call_fn>::value, "agh_localize_depth_batch_clustered_fit");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered_fit_device), depth_call_fn>::value,
  "agh_localize_depth_batch_clustered_fit_device");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered_fit_begin), depth_begin_fn>::value,
  "agh_localize_depth_batch_clustered_fit_begin");
static_assert(std::is_same<decltype(&agh_localize_depth_batch_clustered_fit_begin_device), depth_begin_fn>::value,
  "agh_localize_depth_batch_clustered_fit_begin_device");
static_assert(std::is_same<decltype(&agh_get_batch_plane_fit), fit_fn>::value, "agh_get_batch_plane_fit");
static_assert(std::is_same<decltype(&agh_get_batch_plane_fit_candidates), cand_fn>::value, "agh_get_batch_plane_fit_candidates");
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
    for method in ("localize_batch_clustered_fit", "localize_batch_clustered_fit_begin", "localize_depth_batch_clustered_fit",
                   "localize_depth_batch_clustered_fit_begin", "batch_plane_fit", "batch_plane_fit_candidates"):
        assert callable(getattr(binding.Context, method)), method


def test_a_null_context_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    n_images = (C.c_int32 * 1)(1)
    cp, fp = binding.cluster_params(), binding.plane_fit_params()
    lp = binding.AghLocalizeParams()
    res = (binding.AghLocalizeBatchResult * 1)()
    fits = (binding.AghPlaneFitResult * 64)()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res)
    one = C.c_int32(1)
    for fn in (lib.agh_localize_batch_clustered_fit, lib.agh_localize_batch_clustered_fit_device):
        assert fn(None, None, None, None, C.byref(fp), C.byref(cp), C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_batch_clustered_fit_begin, lib.agh_localize_batch_clustered_fit_begin_device):
        assert fn(None, None, None, None, C.byref(fp), C.byref(cp), C.byref(lp), one) == bad
    for fn in (lib.agh_localize_depth_batch_clustered_fit, lib.agh_localize_depth_batch_clustered_fit_device):
        assert fn(None, recs, n_images, C.byref(fp), C.byref(cp), C.byref(lp), one, *outs) == bad
    for fn in (lib.agh_localize_depth_batch_clustered_fit_begin, lib.agh_localize_depth_batch_clustered_fit_begin_device):
        assert fn(None, recs, n_images, C.byref(fp), C.byref(cp), C.byref(lp), one) == bad
    assert lib.agh_get_batch_plane_fit(None, fits, C.c_int32(64)) == bad
    assert lib.agh_get_batch_plane_fit_candidates(None, C.c_int32(0), None, None, None, C.c_int32(0)) == bad


def test_header_block_and_mid_chain_lists():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_localize_batch_clustered_fit*", "agh_localize_batch_clustered_fit_begin*", "agh_localize_depth_batch_clustered_fit*",
                 "agh_localize_depth_batch_clustered_fit_begin*", "agh_get_batch_plane_fit", "agh_get_batch_plane_fit_candidates"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    # the block stands behind agh_get_batch_cluster_labels, so that the single fit's rules 1 .. 12 stay as they are
    assert hdr.index("int agh_get_batch_cluster_labels(") < hdr.index("WITH EVERY CAPTURE'S SUPPORT PLANE FITTED ON THE DEVICE")
    block = hdr[hdr.index("WITH EVERY CAPTURE'S SUPPORT PLANE FITTED ON THE DEVICE"):hdr.index("int agh_localize_batch_clustered_fit(")]
    assert [int(x) for x in re.findall(r"^ \* {1,2}(\d+)\. ", block, re.M)] == list(range(1, 10))  # the numbered contract, 1 to 9
    block = re.sub(r"\n \*\s+", " ", block)  # (the comment's line breaks fall where they fall)
    for phrase in ("an array of n_captures records", "Rules 1 to 6 of agh_localize_clustered_fit hold per capture", "capture-local",
                   "row k of an n_captures-row agh_set_cloud_cam_origins table", "agh_params::cam_origin[0]",
                   "No voxel of another capture is ever drawn, scored or summed for capture k", "bit for bit",
                   "agh_localize_depth_clustered_fit", "agh_localize_batch_clustered with cp[k].plane set to the reported plane",
                   "K_k empty lists", "a reported plane of zeros", "the other captures are unaffected", "AGH_OK",
                   "on one context and on a fresh one", "fp == NULL", "naming the capture and the field", '"capture k: ..."',
                   "cp[k].plane is ignored and not validated", "an outgrown-slot repeat re-enters with both",
                   "agh_get_batch_cluster_info and agh_get_batch_cluster_labels work as after a clustered batch",
                   "agh_get_plane_fit and agh_get_plane_fit_candidates", "AGH_ERR_STATE", "AGH_ERR_CAPACITY", "pinned",
                   "any array may be NULL", "C_k", "about 0.8 MB", "Nothing is allocated per point"):
        assert phrase in block, phrase
    not_built = block[block.index("Not built:"):]
    for phrase in ("_stage call", "mixed with captures whose plane is given", "more than 256 candidates", "sharded forms"):
        assert phrase in not_built, phrase
    # the older blocks point to the new calls and keep their pinned phrases
    clustered = hdr[hdr.index("one sample list per CONNECTED COMPONENT of every capture's own cloud"):hdr.index("int agh_localize_batch_clustered(")]
    tail = re.sub(r"\n \*\s+", " ", clustered[clustered.index("Not built:"):])
    assert "fitted plane" in tail and "agh_localize_batch_clustered_fit*" in tail
    fit = hdr[hdr.index("WITH THE SUPPORT PLANE FITTED ON THE DEVICE"):hdr.index("typedef struct agh_plane_fit_params")]
    tail = re.sub(r"\n \*\s+", " ", fit[fit.index("Not built:"):])
    assert "batch forms" in tail and "agh_localize_batch_clustered_fit*" in tail
    assert "a fitted plane" in hdr[hdr.index("int agh_get_plane_fit_candidates("):]


def test_documents_and_sources_name_the_stage():
    from agile_grasp_amd import build

    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### A fitted plane in the batch chains"):]
    section = section[:section.index("\n### ", 4)]
    for phrase in NAMES[:1] + ("agh_localize_depth_batch_clustered_fit", "agh_get_batch_plane_fit", "agh_get_batch_plane_fit_candidates") + \
            KERNELS + BODIES + ("| kernel | shape | per capture k |", "plane_fit_stage_batch", "PlaneFitDev", "label_voxels", "d_ccap[k].plane",
                                "Moved, not copied", "scalar loads", "no float atomic", "9 KiB", "Not built"):
        assert phrase in section, phrase
    older = design[design.index("### A fitted plane for the clustered chain"):design.index("### Clusters in the batch chains")]
    assert "agh_localize_batch_clustered_fit" in older[older.index("Not built"):]
    older = design[design.index("### Clusters in the batch chains"):design.index("### A fitted plane in the batch chains")]
    assert "agh_localize_batch_clustered_fit" in older[older.index("Not built"):]
    # moved, not copied: every body is defined once and called by the two forms; the single kernels keep names and arguments
    src = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "plane_fit.hip")).read()
    for kernel in KERNELS + SINGLE:
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", src), kernel
    for body in BODIES:
        assert len(re.findall(r"__device__ __forceinline__ (?:void|bool) " + body + r"\(", src)) == 1, body
        assert len(re.findall(r"(?<![A-Za-z_])" + body + r"\(", src)) == 3, body
    args = r"\(const float\* __restrict__ xyz, int64_t stride, const VoxDesc\* __restrict__ d,\s+int64_t n, PlaneFitDev fp, "
    for kernel in SINGLE[:3]:
        assert re.search(kernel + args + r"PlaneFitBuffers\* __restrict__ fb\)", src), kernel
    assert re.search(SINGLE[3] + args + r"ClusterDev cp, PlaneFitBuffers\* __restrict__ fb, agh_plane_fit_result\* __restrict__ h_result\)", src)
    for kernel in KERNELS:  # one launch per step
        assert len(re.findall(r"hipLaunchKernelGGL\(" + kernel + r",", src)) == 1, kernel
    targets = set(re.findall(r"atomicAdd\(&([A-Za-z_>-]+)\[", src))  # no float atomic anywhere: every target is an integer array
    assert targets == {"cnt", "acc", "fb->counts", "fb->sums"} and len(re.findall(r"atomic[A-Z][A-Za-z]*\(", src)) == 4
    batch = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "localize_batch.hip")).read()
    # the batch keeps copies of both records for a repeat of the pass: in the stored source, which the single chain keeps too
    internal = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "agh_internal.h")).read()
    stored = internal[internal.index("struct StoredSource"):internal.index("struct LocalizeState")]
    assert "std::vector<agh_plane_fit_params> fit;" in stored and "std::vector<agh_cluster_params> cluster;" in stored
    assert "StoredSource source;" in batch[batch.index("struct BatchCall"):batch.index("struct LocalizeBatchState")]
    stage, cluster = batch.index("plane_fit_stage_batch(c, f, st)"), batch.index("sample_cluster_stage_batch(c, m, b->d_ccap, st)")
    upload = batch.index("table_to_device(c, b->d_ccap, b->h_ccap")
    assert upload < stage < cluster  # behind the records' upload, in front of the cluster stage
    # INTEGRATION's source list stays equal to build.SRC (18 units then; since, the hand drop stage and its two tests)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = re.search(r"agile_grasp_amd/csrc/\{([a-z_,]+)\}\.hip", integration).group(1).split(",")
    assert listed == [f[:-len(".hip")] for f in build.SRC] and len(build.SRC) == 21
    for name in ("agh_localize_batch_clustered_fit", "agh_localize_depth_batch_clustered_fit", "localizeHandlesBatchClusteredFit",
                 "localizeHandlesDepthBatchClusteredFit", "fittedPlanes", "batch_plane_fit_candidates"):
        assert name in integration, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "agh_localize_batch_clustered_fit" in readme and "profiles/localize_batch_plane_fit_bench.json" in readme
    notes = open(os.path.join(ROOT, "profiles", "NOTES.md")).read()
    assert "A fitted plane in the batch chains" in notes and "k_fit_score_batch" in notes and "k_fit_finish_batch" in notes
    assert os.path.exists(os.path.join(ROOT, "scripts", "localize_batch_plane_fit_bench.py"))
