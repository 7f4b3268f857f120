"""agh_default_depth_filter_params, agh_set_depth_filter, agh_get_depth_filter and agh_get_depth_filter_counts (include/agh.h):
declared with the documented signatures, the records laid out as the binding has them, exported by the library (with the kernels
k_deproject_filtered and k_deproject_filtered_batch), refused without a context before any device call; the header carries the
contract's phrases and lists the calls in its two mid-chain paragraphs; the adapter's methods compile in both type branches.
Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_set_depth_filter", "agh_get_depth_filter", "agh_get_depth_filter_counts")

SRC = r"""
#include <cstddef>
#include <type_traits>
#include "agh.h"
typedef void (*default_fn)(agh_depth_filter_params*);
typedef int (*set_fn)(agh_ctx*, const agh_depth_filter_params*);
typedef int (*get_fn)(agh_ctx*, agh_depth_filter_params*);
typedef int (*counts_fn)(agh_ctx*, agh_depth_filter_counts*, int32_t);
static_assert(std::is_same<decltype(&agh_default_depth_filter_params), default_fn>::value, "agh_default_depth_filter_params");
static_assert(std::is_same<decltype(&agh_set_depth_filter), set_fn>::value, "agh_set_depth_filter");
static_assert(std::is_same<decltype(&agh_get_depth_filter), get_fn>::value, "agh_get_depth_filter");
static_assert(std::is_same<decltype(&agh_get_depth_filter_counts), counts_fn>::value, "agh_get_depth_filter_counts");
static_assert(std::is_same<decltype(agh_depth_filter_params::radius), int32_t>::value, "radius");
static_assert(std::is_same<decltype(agh_depth_filter_params::min_support), int32_t>::value, "min_support");
static_assert(std::is_same<decltype(agh_depth_filter_params::z_max), double>::value, "z_max");
static_assert(std::is_same<decltype(agh_depth_filter_counts::n_kept), int64_t>::value, "n_kept");
static_assert(sizeof(agh_depth_filter_params) == %d && sizeof(agh_depth_filter_counts) == %d, "sizes");
static_assert(offsetof(agh_depth_filter_params, radius) == %d && offsetof(agh_depth_filter_params, min_support) == %d &&
  offsetof(agh_depth_filter_params, max_jump_abs) == %d && offsetof(agh_depth_filter_params, max_jump_rel) == %d &&
  offsetof(agh_depth_filter_params, z_min) == %d && offsetof(agh_depth_filter_params, z_max) == %d, "parameter offsets");
static_assert(offsetof(agh_depth_filter_counts, n_valid) == %d && offsetof(agh_depth_filter_counts, n_out_of_range) == %d &&
  offsetof(agh_depth_filter_counts, n_unsupported) == %d && offsetof(agh_depth_filter_counts, n_kept) == %d, "counter offsets");
int main() { return 0; }
"""


def _header():
    return open(os.path.join(ROOT, "include", "agh.h")).read()


def test_header_declares_the_calls_and_the_records_match_the_binding(tmp_path):
    hdr = _header()
    from agile_grasp_amd import binding

    lib = binding.load_library()
    assert re.search(r"\bvoid agh_default_depth_filter_params\(", hdr)
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    for fn in NAMES + ("agh_default_depth_filter_params",):
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    assert hasattr(lib, "k_deproject_filtered") and hasattr(lib, "k_deproject_filtered_batch")  # (the kernels' host-side handles)
    P, K = binding.AghDepthFilterParams, binding.AghDepthFilterCounts
    assert [n for n, _ in P._fields_] == ["radius", "min_support", "max_jump_abs", "max_jump_rel", "z_min", "z_max"]
    assert [n for n, _ in K._fields_] == ["n_valid", "n_out_of_range", "n_unsupported", "n_kept"]
    src = tmp_path / "sig.cpp"
    src.write_text(SRC % ((C.sizeof(P), C.sizeof(K)) + tuple(getattr(P, n).offset for n, _ in P._fields_)
                          + tuple(getattr(K, n).offset for n, _ in K._fields_)))
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    csrc = tmp_path / "c.c"  # (the header stays a C header)
    csrc.write_text('#include "agh.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])
    for method in ("set_depth_filter", "clear_depth_filter", "depth_filter", "depth_filter_counts"):
        assert callable(getattr(binding.Context, method)), method


def test_defaults_and_a_null_context():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    fp = binding.depth_filter_params()
    assert (fp.radius, fp.min_support, fp.max_jump_abs, fp.max_jump_rel, fp.z_min, fp.z_max) == (1, 3, 0.01, 0.01, 0.0, float("inf"))
    lib.agh_default_depth_filter_params(None)  # (ignored)
    with pytest.raises(TypeError):
        binding.depth_filter_params(window=3)
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    counts = (binding.AghDepthFilterCounts * 2)()
    assert lib.agh_set_depth_filter(None, C.byref(fp)) == bad and lib.agh_set_depth_filter(None, None) == bad
    assert lib.agh_get_depth_filter(None, C.byref(fp)) == bad
    assert lib.agh_get_depth_filter_counts(None, counts, C.c_int32(2)) == bad


def test_header_block_and_mid_chain_lists():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_set_depth_filter", "agh_get_depth_filter_counts"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    assert re.search(r"agh_get_depth_filter\b(?!_)", allowed)  # (host-side, like agh_get_cloud_cam_origins)
    # the block stands behind the depth-batch block
    assert hdr.index("int agh_deproject_batch(") < hdr.index("A DEPTH FILTER for every call that back-projects depth images")
    block = hdr[hdr.index("A DEPTH FILTER for every call that back-projects depth images"):hdr.index("void agh_default_depth_filter_params(")]
    assert [int(x) for x in re.findall(r"^ \* {1,2}(\d+)\. ", block, re.M)] == [1, 2, 3, 4]  # the four steps
    block = re.sub(r"\n \*\s+", " ", block)
    for phrase in ("counted on the in-range set", "three quiet NaNs", "sticky", "not symmetric", "tol = ja + (jr * z_p)",
                   "fabsf(z_q - z_p) <= tol", "z >= zlo && z <= zhi", "Pixels outside the image never support",
                   "rounds the four doubles once to float32", "NULL clears the filter", "the text names the field",
                   "the filter held before stays in force", "agh_localize_depth_stage stays a pure copy", "in launch order",
                   "AGH_ERR_CAPACITY", "AGH_ERR_STATE", "neither filter again nor count again", "One small copy and one synchronisation"):
        assert phrase in block, phrase
    not_built = block[block.index("Not built:"):]
    for phrase in ("temporal filtering", "hole filling", "lens distortion", "per-image parameters", "points forms"):
        assert phrase in not_built, phrase
    for doc, phrases in (("DESIGN.md", ("## Depth filter", "k_deproject_filtered", "128 words", "ScratchSize")),
                         ("README.md", ("agh_set_depth_filter", "set_depth_filter"))):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(p in text for p in phrases), doc


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "depth_filter_adapter_test.cpp")])
    for hdr in ("hand_search.h", "localization.h"):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in ("setDepthFilter", "clearDepthFilter", "depthFilter(", "depthFilterCounts")), hdr
