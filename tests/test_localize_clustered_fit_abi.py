"""agh_localize_clustered_fit / _device, agh_localize_depth_clustered_fit / _device, agh_get_plane_fit,
agh_get_plane_fit_candidates and agh_default_plane_fit_params (include/agh.h): declared with the documented signatures, exported by
the library, refused without a context before any device call, the two records laid out as the binding's, the defaults as
documented, and the header, DESIGN.md and INTEGRATION.md name what they should.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_clustered_fit", "agh_localize_clustered_fit_device", "agh_localize_depth_clustered_fit",
         "agh_localize_depth_clustered_fit_device", "agh_get_plane_fit", "agh_get_plane_fit_candidates")

SRC = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float*, int64_t, int64_t, const agh_plane_fit_params*, const agh_cluster_params*,
  const agh_localize_params*, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, int32_t, const agh_plane_fit_params*, const agh_cluster_params*,
  const agh_localize_params*, agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*fit_fn)(agh_ctx*, agh_plane_fit_result*);
typedef int (*cand_fn)(agh_ctx*, int32_t*, double*, int64_t*, int32_t);
typedef void (*defaults_fn)(agh_plane_fit_params*);
static_assert(std::is_same<decltype(&agh_localize_clustered_fit), call_fn>::value, "agh_localize_clustered_fit");
static_assert(std::is_same<decltype(&agh_localize_clustered_fit_device), call_fn>::value, "agh_localize_clustered_fit_device");
static_assert(std::is_same<decltype(&agh_localize_depth_clustered_fit), depth_call_fn>::value, "agh_localize_depth_clustered_fit");
static_assert(std::is_same<decltype(&agh_localize_depth_clustered_fit_device), depth_call_fn>::value, "agh_localize_depth_clustered_fit_device");
static_assert(std::is_same<decltype(&agh_get_plane_fit), fit_fn>::value, "agh_get_plane_fit");
static_assert(std::is_same<decltype(&agh_get_plane_fit_candidates), cand_fn>::value, "agh_get_plane_fit_candidates");
static_assert(std::is_same<decltype(&agh_default_plane_fit_params), defaults_fn>::value, "agh_default_plane_fit_params");
static_assert(std::is_same<decltype(agh_plane_fit_params::n_candidates), int32_t>::value, "n_candidates");
static_assert(std::is_same<decltype(agh_plane_fit_params::distance_threshold), double>::value, "distance_threshold");
static_assert(std::is_same<decltype(agh_plane_fit_params::seed), uint64_t>::value, "seed");
static_assert(std::is_same<decltype(agh_plane_fit_result::plane), double[4]>::value, "plane");
static_assert(std::is_same<decltype(agh_plane_fit_result::n_refit), int64_t>::value, "n_refit");
static_assert(std::is_same<decltype(agh_plane_fit_result::best_candidate), int32_t>::value, "best_candidate");
int main()
{
  std::printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(agh_plane_fit_params), offsetof(agh_plane_fit_params, refine),
    offsetof(agh_plane_fit_params, min_inliers), offsetof(agh_plane_fit_params, reserved), offsetof(agh_plane_fit_params, distance_threshold),
    offsetof(agh_plane_fit_params, seed), sizeof(agh_plane_fit_result));
  std::printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(agh_plane_fit_result, n_voxels), offsetof(agh_plane_fit_result, n_inliers),
    offsetof(agh_plane_fit_result, n_refit), offsetof(agh_plane_fit_result, best_candidate), offsetof(agh_plane_fit_result, found),
    offsetof(agh_plane_fit_result, refined), offsetof(agh_plane_fit_result, reserved));
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
    assert re.search(r"\bvoid agh_default_plane_fit_params\(", hdr) and "agh_default_plane_fit_params" in binding.EXPORTS
    assert "typedef struct agh_plane_fit_params" in hdr and "typedef struct agh_plane_fit_result" in hdr
    src = tmp_path / "sig.cpp"
    src.write_text(SRC)
    exe = tmp_path / "sig"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    p, r = binding.AghPlaneFitParams, binding.AghPlaneFitResult
    assert got[:7] == [C.sizeof(p), p.refine.offset, p.min_inliers.offset, p.reserved.offset, p.distance_threshold.offset,
                       p.seed.offset, C.sizeof(r)] == [32, 4, 8, 12, 16, 24, 72]
    assert got[7:] == [r.n_voxels.offset, r.n_inliers.offset, r.n_refit.offset, r.best_candidate.offset, r.found.offset,
                       r.refined.offset, r.reserved.offset] == [32, 40, 48, 56, 60, 64, 68]
    # the header is a C header
    csrc = tmp_path / "c.c"
    csrc.write_text('#include "agh.h"\nint main(void) { agh_plane_fit_params p; agh_plane_fit_result r; (void) p; (void) r; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])


def test_the_defaults():
    from agile_grasp_amd import binding

    fp = binding.plane_fit_params()
    assert (fp.n_candidates, fp.refine, fp.min_inliers, fp.reserved, fp.distance_threshold, fp.seed) == (128, 1, 3, 0, 0.01, 1)
    binding.load_library().agh_default_plane_fit_params(None)  # (a NULL record is ignored)
    fp = binding.plane_fit_params(n_candidates=256, seed=2 ** 64 - 1)
    assert (fp.n_candidates, fp.seed, fp.min_inliers) == (256, 2 ** 64 - 1, 3)


def test_the_documents_name_the_calls_where_they_list_calls():
    hdr = _header()
    block = hdr[hdr.index("WITH THE SUPPORT PLANE FITTED ON THE DEVICE"):hdr.index("int agh_get_plane_fit_candidates(")]
    for phrase in ("splitmix64", "0x9E3779B97F4A7C15", "never contracted", "three divisions", "ties to the smaller c", "65536.0",
                   "2^24", ">= 8", "smallest_eigvec3", "cam_origin[0]", "one-row", "NaN plane", "not validated", "1 .. 256", "0.05",
                   "AGH_ERR_NO_SVM", "pinned", "Not built", "batch forms", "_begin / _end", "_stage", "sharded", "termination rule"):
        assert phrase in block, phrase
    # the rules are numbered as the clustered block's are
    assert [int(x) for x in re.findall(r"^ \* {1,2}(\d+)\. ", block, re.M)] == list(range(1, 13))
    # the single clustered block points to the new call; the batch blocks keep "fitted plane"
    clustered = hdr[hdr.index("WITHOUT A SEGMENTER"):hdr.index("int agh_get_cluster_labels(")]
    tail = clustered[clustered.index("Not built"):]
    assert "agh_localize_clustered_fit" in tail and "a fitted plane (the caller supplies it)" not in tail
    assert "a fitted plane" in hdr[hdr.index("int agh_get_plane_fit_candidates("):]
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("A begin of either kind while a chain of either kind is in"):hdr.index("int agh_localize_batch_begin(")]
    refused = single.split("may be called on the context")[1]
    for name in ("agh_localize_clustered_fit*", "agh_localize_depth_clustered_fit*", "agh_get_plane_fit,", "agh_get_plane_fit_candidates"):
        assert name in refused and name not in single.split("may be called on the context")[0], name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("A fitted plane for the clustered chain"):]
    for phrase in ("k_fit_candidates", "k_fit_score", "k_fit_moments", "k_fit_finish", "k_cluster_init_dev", "k_cluster_link_dev",
                   "ballot", "int64", "Not built"):
        assert phrase in section, phrase
    assert "agh_localize_clustered_fit" in design[design.index("Clusters as the label source"):design.index("A fitted plane for the clustered chain")]
    for doc in ("README.md", "INTEGRATION.md"):
        assert "agh_localize_clustered_fit" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_new_source_file_is_built_with_the_others():
    from agile_grasp_amd import build

    assert "plane_fit.hip" in build.SRC and os.path.exists(os.path.join(ROOT, "agile_grasp_amd", "csrc", "plane_fit.hip"))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = re.search(r"agile_grasp_amd/csrc/\{([a-z_,]+)\}\.hip", integration).group(1).split(",")
    assert listed == [f[:-len(".hip")] for f in build.SRC]


def test_a_null_context_or_record_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    lp = binding.AghLocalizeParams()
    cp = binding.cluster_params()
    fp = binding.plane_fit_params()
    res = (binding.AghLocalizeBatchResult * 16)()
    fit = binding.AghPlaneFitResult()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res)
    for fn in (lib.agh_localize_clustered_fit, lib.agh_localize_clustered_fit_device):
        assert fn(None, None, C.c_int64(12), C.c_int64(0), C.byref(fp), C.byref(cp), C.byref(lp), *outs) == bad
    for fn in (lib.agh_localize_depth_clustered_fit, lib.agh_localize_depth_clustered_fit_device):
        assert fn(None, recs, C.c_int32(1), C.byref(fp), C.byref(cp), C.byref(lp), *outs) == bad
    assert lib.agh_get_plane_fit(None, C.byref(fit)) == bad
    assert lib.agh_get_plane_fit_candidates(None, None, None, None, C.c_int32(0)) == bad
