"""agh_default_hand_filter_params, agh_set_hand_filter, agh_get_hand_filter and agh_get_hand_filter_counts (include/agh.h):
declared with the documented signatures, the records laid out as the binding has them, exported by the library, refused without a
context before any device call; the header lists the calls in its two mid-chain paragraphs and states the contract's fixed
points; the adapter's methods and the example's flags compile in both type branches."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_set_hand_filter", "agh_get_hand_filter", "agh_get_hand_filter_counts")

SRC = r"""
#include <cstddef>
#include <type_traits>
#include "agh.h"
typedef void (*default_fn)(agh_hand_filter_params*);
typedef int (*set_fn)(agh_ctx*, const agh_hand_filter_params*);
typedef int (*get_fn)(agh_ctx*, agh_hand_filter_params*);
typedef int (*counts_fn)(agh_ctx*, agh_hand_filter_counts*, int32_t);
static_assert(std::is_same<decltype(&agh_default_hand_filter_params), default_fn>::value, "agh_default_hand_filter_params");
static_assert(std::is_same<decltype(&agh_set_hand_filter), set_fn>::value, "agh_set_hand_filter");
static_assert(std::is_same<decltype(&agh_get_hand_filter), get_fn>::value, "agh_get_hand_filter");
static_assert(std::is_same<decltype(&agh_get_hand_filter_counts), counts_fn>::value, "agh_get_hand_filter_counts");
static_assert(std::is_same<decltype(agh_hand_filter_params::approach_dir), double[3]>::value, "approach_dir");
static_assert(std::is_same<decltype(agh_hand_filter_params::probes_per_finger), int32_t>::value, "probes_per_finger");
static_assert(std::is_same<decltype(agh_hand_filter_counts::n_kept), int64_t>::value, "n_kept");
static_assert(sizeof(agh_hand_filter_params) == %d && sizeof(agh_hand_filter_counts) == %d, "sizes");
int main() { return 0; }
"""


def _header():
    return open(os.path.join(ROOT, "include", "agh.h")).read()


def test_header_declares_the_calls_and_the_records_match_the_binding(tmp_path):
    hdr = _header()
    from agile_grasp_amd import binding

    lib = binding.load_library()
    assert re.search(r"\bvoid agh_default_hand_filter_params\(", hdr)
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    for fn in NAMES + ("agh_default_hand_filter_params",):
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    P, K = binding.AghHandFilterParams, binding.AghHandFilterCounts
    assert [n for n, _ in P._fields_] == ["approach_on", "width_on", "view_on", "probes_per_finger", "approach_dir", "min_approach_cos",
                                          "min_width", "max_width", "depth_margin", "max_unobserved", "reserved"]
    assert [n for n, _ in K._fields_] == ["n_hypotheses", "n_dropped_approach", "n_dropped_width", "n_dropped_unobserved", "n_kept"]
    assert (C.sizeof(P), C.sizeof(K)) == (80, 40)
    offsets = "".join(f'static_assert(offsetof(agh_hand_filter_params, {n}) == {getattr(P, n).offset}, "{n}");\n' for n, _ in P._fields_)
    offsets += "".join(f'static_assert(offsetof(agh_hand_filter_counts, {n}) == {getattr(K, n).offset}, "{n}");\n' for n, _ in K._fields_)
    src = tmp_path / "sig.cpp"
    src.write_text((SRC % (C.sizeof(P), C.sizeof(K))).replace("int main()", offsets + "int main()"))
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    csrc = tmp_path / "c.c"  # (the header stays a C header)
    csrc.write_text('#include "agh.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])
    for method in ("set_hand_filter", "clear_hand_filter", "get_hand_filter", "hand_filter_counts"):
        assert callable(getattr(binding.Context, method)), method


def test_defaults_and_a_null_context():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    fp = binding.hand_filter_params()
    assert (fp.approach_on, fp.width_on, fp.view_on) == (0, 0, 0)  # each criterion is off in the defaults
    assert (fp.probes_per_finger, fp.depth_margin, fp.max_unobserved) == (4, 0.01, 0)
    assert list(fp.approach_dir) == [0.0, 0.0, 1.0] and fp.min_approach_cos == -1.0 and (fp.min_width, fp.max_width) == (0.0, 0.1)
    got = binding.hand_filter_params(approach_dir=(0.0, 1.0, 0.0), view_on=1)
    assert list(got.approach_dir) == [0.0, 1.0, 0.0] and got.view_on == 1
    lib.agh_default_hand_filter_params(None)  # (ignored)
    with pytest.raises(TypeError):
        binding.hand_filter_params(min_cos=0.5)
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    counts = (binding.AghHandFilterCounts * 2)()
    assert lib.agh_set_hand_filter(None, C.byref(fp)) == bad and lib.agh_set_hand_filter(None, None) == bad
    assert lib.agh_get_hand_filter(None, C.byref(fp)) == bad
    assert lib.agh_get_hand_filter_counts(None, counts, C.c_int32(2)) == bad


def test_header_block_mid_chain_lists_and_documents():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_set_hand_filter", "agh_get_hand_filter_counts"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    assert re.search(r"agh_get_hand_filter\b(?!_)", allowed)  # (host-side, like the other two filters' getters)
    start = hdr.index("A HAND FILTER on the way out")
    assert hdr.index("int agh_get_voxel_filter_counts(") < start  # the block stands behind the voxel filter's
    block = re.sub(r"\n \*\s+", " ", hdr[start:hdr.index("typedef struct agh_hand_filter_params")])
    for phrase in ("between the search and the classifier", "FIRST criterion that drops it", "|a^2 + b^2 + c^2 - 1| <= 1e-6",
                   "((a0 * d0 + a1 * d1) + a2 * d2) < min_approach_cos", "never contracted", "width < min_width || width > max_width",
                   "(bottom - s) . binormal", "hand_outer_diameter / 2 - finger_width / 2", "(j + 0.5) x (hand_depth / n)",
                   "-hand_height, 0, +hand_height", "q.z > 0", "depth_margin", "AS UPLOADED", "orthonormal", "the text naming the image",
                   "EVERY agh_localize* form that takes points is refused", "must not silently not apply", "A NaN in a tested field",
                   "sticky per context", "does no device work", "AGH_ERR_STATE", "allowed mid-chain", "if either filter says so",
                   "n_hypotheses stays the search's unfiltered count", "not touched", "nothing new is launched", "pinned memory"):
        assert phrase in block, phrase
    for doc, phrases in (("DESIGN.md", ("## Hand filter", "k_hand_filter", "compact_kept_records", "drop byte")),
                         ("README.md", ("agh_set_hand_filter", "set_hand_filter")), ("INTEGRATION.md", ("setHandFilter",))):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(p in text for p in phrases), doc


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "hand_filter_adapter_test.cpp")])
    for hdr in ("hand_search.h", "localization.h"):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in ("setHandFilter", "clearHandFilter", "handFilter(", "handFilterCounts")), hdr
    example = open(os.path.join(ROOT, "examples", "localize_pcd.cpp")).read()
    assert "--approach" in example and "--aperture" in example and "setHandFilter" in example
