"""agh_localize_clustered / _device, agh_localize_depth_clustered / _device, agh_get_cluster_info, agh_get_cluster_labels and
agh_default_cluster_params (include/agh.h): declared with the documented signatures, exported by the library, refused without a
context before any device call, the two records laid out as the binding's, the defaults as documented, and the header's "Not built"
sentence and mid-chain lists name what they should.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_localize_clustered", "agh_localize_clustered_device", "agh_localize_depth_clustered",
         "agh_localize_depth_clustered_device", "agh_get_cluster_info", "agh_get_cluster_labels")

SRC = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "agh.h"
typedef int (*call_fn)(agh_ctx*, const float*, int64_t, int64_t, const agh_cluster_params*, const agh_localize_params*, agh_handle*,
  int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*depth_call_fn)(agh_ctx*, const agh_depth_image*, int32_t, const agh_cluster_params*, const agh_localize_params*,
  agh_handle*, int64_t, int32_t*, int64_t, agh_hypothesis*, int64_t, int32_t*, agh_localize_batch_result*);
typedef int (*info_fn)(agh_ctx*, agh_cluster_info*, int64_t*, int32_t*, int32_t);
typedef int (*labels_fn)(agh_ctx*, uint8_t*, int64_t);
typedef void (*defaults_fn)(agh_cluster_params*);
static_assert(std::is_same<decltype(&agh_localize_clustered), call_fn>::value, "agh_localize_clustered");
static_assert(std::is_same<decltype(&agh_localize_clustered_device), call_fn>::value, "agh_localize_clustered_device");
static_assert(std::is_same<decltype(&agh_localize_depth_clustered), depth_call_fn>::value, "agh_localize_depth_clustered");
static_assert(std::is_same<decltype(&agh_localize_depth_clustered_device), depth_call_fn>::value, "agh_localize_depth_clustered_device");
static_assert(std::is_same<decltype(&agh_get_cluster_info), info_fn>::value, "agh_get_cluster_info");
static_assert(std::is_same<decltype(&agh_get_cluster_labels), labels_fn>::value, "agh_get_cluster_labels");
static_assert(std::is_same<decltype(&agh_default_cluster_params), defaults_fn>::value, "agh_default_cluster_params");
static_assert(std::is_same<decltype(agh_cluster_params::plane), double[4]>::value, "plane");
static_assert(std::is_same<decltype(agh_cluster_params::min_voxels), int32_t>::value, "min_voxels");
static_assert(std::is_same<decltype(agh_cluster_info::n_components), int64_t>::value, "n_components");
int main()
{
  std::printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(agh_cluster_params), offsetof(agh_cluster_params, min_height),
    offsetof(agh_cluster_params, max_height), offsetof(agh_cluster_params, tolerance), offsetof(agh_cluster_params, min_voxels),
    offsetof(agh_cluster_params, max_objects), sizeof(agh_cluster_info));
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
    assert re.search(r"\bvoid agh_default_cluster_params\(", hdr) and "agh_default_cluster_params" in binding.EXPORTS
    assert "typedef struct agh_cluster_params" in hdr and "typedef struct agh_cluster_info" in hdr
    src = tmp_path / "sig.cpp"
    src.write_text(SRC)
    exe = tmp_path / "sig"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    rec = binding.AghClusterParams
    assert got == [C.sizeof(rec), rec.min_height.offset, rec.max_height.offset, rec.tolerance.offset, rec.min_voxels.offset,
                   rec.max_objects.offset, C.sizeof(binding.AghClusterInfo)] == [64, 32, 40, 48, 56, 60, 24]
    # the header is a C header
    csrc = tmp_path / "c.c"
    csrc.write_text('#include "agh.h"\nint main(void) { agh_cluster_params p; agh_cluster_info i; (void) p; (void) i; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])


def test_the_defaults():
    from agile_grasp_amd import binding

    cp = binding.cluster_params()
    assert list(cp.plane) == [0.0, 0.0, 1.0, 0.0]
    assert (cp.min_height, cp.max_height, cp.tolerance, cp.min_voxels, cp.max_objects) == (0.01, 0.5, 0.01, 50, 16)
    binding.load_library().agh_default_cluster_params(None)  # (a NULL record is ignored)
    cp = binding.cluster_params(plane=(0.0, 1.0, 0.0, -0.5), max_objects=3)
    assert list(cp.plane) == [0.0, 1.0, 0.0, -0.5] and cp.max_objects == 3 and cp.min_voxels == 50


def test_the_header_names_the_calls_where_it_lists_calls():
    hdr = _header()
    block = hdr[hdr.index("WITHOUT A SEGMENTER"):hdr.index("int agh_get_cluster_labels(")]
    for phrase in ("min_height < h < max_height", "never contracted", "smallest voxel", "size descending", "INT32_MIN", "1e-6", "0.05",
                   "2^24", "AGH_ERR_NO_SVM", "Not built", "_begin / _end", "batch and sharded", "8192-hand"):
        assert phrase in block, phrase
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("A begin of either kind while a chain of either kind is in"):hdr.index("int agh_localize_batch_begin(")]
    refused = single.split("may be called on the context")[1]
    for name in ("agh_localize_clustered*", "agh_localize_depth_clustered*", "agh_get_cluster_info", "agh_get_cluster_labels"):
        assert name in refused and name not in single.split("may be called on the context")[0], name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("Clusters as the label source"):]
    for phrase in ("k_cluster_init", "k_cluster_link", "k_cluster_flatten", "k_cluster_select", "k_cluster_mark", "strictly decreases",
                   "Not built"):
        assert phrase in section, phrase


def test_the_new_source_file_is_built_with_the_others():
    from agile_grasp_amd import build

    assert "sample_cluster.hip" in build.SRC and os.path.exists(os.path.join(ROOT, "agile_grasp_amd", "csrc", "sample_cluster.hip"))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = re.search(r"agile_grasp_amd/csrc/\{([a-z_,]+)\}\.hip", integration).group(1).split(",")
    assert listed == [f[:-len(".hip")] for f in build.SRC]
    assert "agh_localize_clustered" in integration


def test_a_null_context_or_record_is_refused_without_a_device():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    recs = (binding.AghDepthImage * 1)()
    lp = binding.AghLocalizeParams()
    cp = binding.cluster_params()
    res = (binding.AghLocalizeBatchResult * 16)()
    info = binding.AghClusterInfo()
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    outs = (None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0), None, res)
    for fn in (lib.agh_localize_clustered, lib.agh_localize_clustered_device):
        assert fn(None, None, C.c_int64(12), C.c_int64(0), C.byref(cp), C.byref(lp), *outs) == bad
    for fn in (lib.agh_localize_depth_clustered, lib.agh_localize_depth_clustered_device):
        assert fn(None, recs, C.c_int32(1), C.byref(cp), C.byref(lp), *outs) == bad
    assert lib.agh_get_cluster_info(None, C.byref(info), None, None, C.c_int32(0)) == bad
    assert lib.agh_get_cluster_labels(None, None, C.c_int64(0)) == bad
