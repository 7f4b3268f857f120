"""agh_default_handle_ranking_params, agh_set_handle_ranking, agh_get_handle_ranking, agh_get_handle_scores,
agh_get_handle_ranking_counts, agh_get_hand_margins and agh_rank_handles (include/agh.h): declared with the documented
signatures, the records laid out as the binding has them, exported by the library, refused without a context before any device
call; the header lists the calls in its mid-chain paragraphs and states the contract's numbered rules; the hand filter's and the
clearance's frozen records are what they were."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_set_handle_ranking", "agh_get_handle_ranking", "agh_get_handle_scores", "agh_get_handle_ranking_counts",
         "agh_get_hand_margins", "agh_rank_handles")

SRC = r"""
#include <cstddef>
#include <type_traits>
#include "agh.h"
typedef void (*default_fn)(agh_handle_ranking_params*);
typedef int (*set_fn)(agh_ctx*, const agh_handle_ranking_params*);
typedef int (*get_fn)(agh_ctx*, agh_handle_ranking_params*);
typedef int (*scores_fn)(agh_ctx*, agh_handle_score*, int64_t);
typedef int (*counts_fn)(agh_ctx*, agh_handle_ranking_counts*, int32_t);
typedef int (*margins_fn)(agh_ctx*, double*, int64_t);
typedef int (*rank_fn)(agh_ctx*, const agh_handle_ranking_params*, const agh_hypothesis*, int64_t, const double*, const agh_handle*,
  int64_t, const int32_t*, int64_t, agh_handle*, agh_handle_score*, int64_t, agh_handle_ranking_counts*);
static_assert(std::is_same<decltype(&agh_default_handle_ranking_params), default_fn>::value, "agh_default_handle_ranking_params");
static_assert(std::is_same<decltype(&agh_set_handle_ranking), set_fn>::value, "agh_set_handle_ranking");
static_assert(std::is_same<decltype(&agh_get_handle_ranking), get_fn>::value, "agh_get_handle_ranking");
static_assert(std::is_same<decltype(&agh_get_handle_scores), scores_fn>::value, "agh_get_handle_scores");
static_assert(std::is_same<decltype(&agh_get_handle_ranking_counts), counts_fn>::value, "agh_get_handle_ranking_counts");
static_assert(std::is_same<decltype(&agh_get_hand_margins), margins_fn>::value, "agh_get_hand_margins");
static_assert(std::is_same<decltype(&agh_rank_handles), rank_fn>::value, "agh_rank_handles");
static_assert(std::is_same<decltype(agh_handle_ranking_params::w_margin), double>::value, "w_margin");
static_assert(std::is_same<decltype(agh_handle_ranking_params::approach_dir), double[3]>::value, "approach_dir");
static_assert(std::is_same<decltype(agh_handle_ranking_params::support_cap), int32_t>::value, "support_cap");
static_assert(std::is_same<decltype(agh_handle_score::terms), double[7]>::value, "terms");
static_assert(std::is_same<decltype(agh_handle_score::best_inlier), int32_t>::value, "best_inlier");
static_assert(std::is_same<decltype(agh_handle_ranking_counts::n_below), int64_t>::value, "n_below");
static_assert(sizeof(agh_handle_score) == 72, "agh_handle_score is frozen");
static_assert(sizeof(agh_handle_ranking_params) == %d && sizeof(agh_handle_ranking_counts) == %d, "sizes");
static_assert(sizeof(agh_hand_filter_params) == 80 && sizeof(agh_hand_filter_counts) == 40, "the hand filter's records are frozen");
static_assert(sizeof(agh_hand_clearance_params) == 40 && sizeof(agh_hand_clearance_counts) == 24, "the clearance's records are frozen");
static_assert(sizeof(agh_handle) == 136 && sizeof(agh_hypothesis) == 160, "the handle and hypothesis records are what they were");
int main() { return 0; }
"""


def _header():
    return open(os.path.join(ROOT, "include", "agh.h")).read()


def test_header_declares_the_calls_and_the_records_match_the_binding(tmp_path):
    hdr = _header()
    from agile_grasp_amd import binding
    from tests import handle_ranking_cases as R

    lib = binding.load_library()
    assert re.search(r"\bvoid agh_default_handle_ranking_params\(", hdr)
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    for fn in NAMES + ("agh_default_handle_ranking_params",):
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    P, S, K = binding.AghHandleRankingParams, binding.AghHandleScore, binding.AghHandleRankingCounts
    assert [n for n, _ in P._fields_] == ["w_support", "w_margin", "w_approach", "w_position", "w_distance", "w_width", "w_length",
                                          "approach_dir", "position_dir", "ref_point", "preferred_width", "min_score", "support_cap",
                                          "max_handles"]
    assert [n for n, _ in S._fields_] == ["score", "terms", "index", "best_inlier"]
    assert [n for n, _ in K._fields_] == ["n_found", "n_below", "n_returned"]
    assert (C.sizeof(P), C.sizeof(S), C.sizeof(K)) == (152, 72, 24)
    assert binding.SCORE_DTYPE == R.SCORE_DTYPE and binding.HANDLE_DTYPE == R.HANDLE_DTYPE  # (the model restates the binding's)
    assert [binding.SCORE_DTYPE.fields[n][1] for n, _ in S._fields_] == [getattr(S, n).offset for n, _ in S._fields_]
    offsets = ""
    for rec, T in (("agh_handle_ranking_params", P), ("agh_handle_score", S), ("agh_handle_ranking_counts", K)):
        offsets += "".join(f'static_assert(offsetof({rec}, {n}) == {getattr(T, n).offset}, "{n}");\n' for n, _ in T._fields_)
    src = tmp_path / "sig.cpp"
    src.write_text((SRC % (C.sizeof(P), C.sizeof(K))).replace("int main()", offsets + "int main()"))
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    csrc = tmp_path / "c.c"  # (the header stays a C header)
    csrc.write_text('#include "agh.h"\nint main(void) { agh_handle_ranking_params p; agh_default_handle_ranking_params(&p); '
                    'return p.max_handles; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])
    for method in ("set_handle_ranking", "clear_handle_ranking", "get_handle_ranking", "handle_scores", "handle_ranking_counts",
                   "hand_margins", "rank_handles"):
        assert callable(getattr(binding.Context, method)), method


def test_every_export_is_in_the_library_and_the_library_has_the_kernel():
    from agile_grasp_amd import binding, build

    lib = binding.load_library()
    for fn in binding.EXPORTS:
        assert hasattr(lib, fn), fn
    blob = open(lib._name, "rb").read()
    assert b"k_handle_rank" in blob and b"k_handle_build" in blob  # (the native kernels, not a fall-back)
    # handle_rank.hip is part of handles.hip's translation unit, and a change to it rebuilds the library
    handles = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "handles.hip")).read()
    assert '#include "handle_rank.hip"' in handles and "handles.hip" in build.SRC and "handle_rank.hip" not in build.SRC
    assert "handle_rank.hip" in open(build.__file__).read().split("def needs_build")[1].split("def build")[0]


def test_defaults_and_a_null_context():
    from agile_grasp_amd import binding
    from tests import handle_ranking_cases as R

    lib = binding.load_library()
    rp = binding.handle_ranking_params()
    for k, v in R.DEFAULTS.items():  # (the model's defaults are the library's)
        got = getattr(rp, k)
        assert (tuple(got) if k in ("approach_dir", "position_dir", "ref_point") else got) == v, k
    assert rp.min_score == -np.inf and (rp.w_support, rp.w_margin, rp.support_cap, rp.max_handles) == (1.0, 1.0, 10, 0)
    got = binding.handle_ranking_params(w_length=2.0, max_handles=3, position_dir=(1, 2, 3))
    assert (got.w_length, got.max_handles, tuple(got.position_dir), got.w_margin) == (2.0, 3, (1.0, 2.0, 3.0), 1.0)
    lib.agh_default_handle_ranking_params(None)  # (ignored)
    with pytest.raises(TypeError):
        binding.handle_ranking_params(w_height=0.5)
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    counts = (binding.AghHandleRankingCounts * 2)()
    scores = (binding.AghHandleScore * 2)()
    margins = (C.c_double * 2)()
    assert lib.agh_set_handle_ranking(None, C.byref(rp)) == bad and lib.agh_set_handle_ranking(None, None) == bad
    assert lib.agh_get_handle_ranking(None, C.byref(rp)) == bad
    assert lib.agh_get_handle_scores(None, scores, C.c_int64(2)) == bad
    assert lib.agh_get_handle_ranking_counts(None, counts, C.c_int32(2)) == bad
    assert lib.agh_get_hand_margins(None, margins, C.c_int64(2)) == bad
    assert lib.agh_rank_handles(None, C.byref(rp), None, C.c_int64(0), None, None, C.c_int64(0), None, C.c_int64(0), None, None,
                                C.c_int64(0), counts) == bad


def test_header_block_mid_chain_lists_and_documents():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_set_handle_ranking", "agh_rank_handles", "agh_get_handle_scores", "agh_get_handle_ranking_counts",
                 "agh_get_hand_margins"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    assert re.search(r"agh_get_handle_ranking\b(?!_)", allowed)  # (host-side, like the filters' getters)
    assert re.search(r"agh_get_handle_ranking\b(?!_)", batch)
    start = hdr.index("HANDLE RANKING:")
    assert hdr.index("int agh_get_hand_clearance_counts(") < start  # the block stands behind the clearance's
    block = re.sub(r"\n \*\s+", " ", hdr[start:hdr.index("typedef struct agh_handle_ranking_params")])
    for phrase in ("float64, evaluated left to right, never contracted", "1. INPUTS", "minus the decision sum",
                   "sum = -rho + res", "kept hands have g >= 0", "With classify == 0, g = 0.0",
                   "2. THE WAVE SUM W(v, n)", "p[l] = ((v[l] + v[l+64]) + v[l+128]) + ...", "starting from +0.0",
                   "p[l] = p[l] + p[l ^ o] for o = 32, 16, 8, 4, 2, 1", "the result is p[0]",
                   "3. THE SEVEN TERMS", "t_support = (double) min(n, support_cap) / (double) support_cap",
                   "t_margin = W(g, n) / (double) n", "t_approach = (a0 d0 + a1 d1) + a2 d2", "t_position = (c0 p0 + c1 p1) + c2 p2",
                   "t_distance = sqrt((e0 e0 + e1 e1) + e2 e2)", "t_width = fabs(handle.width - preferred_width)",
                   "t_length = max_k(x_k) - min_k(x_k)", "fmax / fmin",
                   "4. THE SCORE", "(((((w_support t1 + w_margin t2) + w_approach t3) + w_position t4) + w_distance t5) + w_width t6) + w_length t7",
                   "a NaN term makes the score NaN even under weight 0", "5. best_inlier", "a NaN g never wins", "0 if none wins",
                   "6. ORDER", "!(score >= min_score)", "n_below", "NaN scores after every number", "+0 and -0 tie",
                   "ascending index", "The order is total", "no sort algorithm", "no atomic",
                   "7. OUTPUTS", "is the number returned", "AGH_ERR_CAPACITY for handle_cap is judged on it",
                   "only the handle records move", "8. SCOPE", "does no device work", "the text names it", "launches nothing",
                   "Set-then-clear is the same as never set", "9. MID-CHAIN", "AGH_ERR_STATE", "allowed mid-chain", "pinned memory",
                   "10. STAGE-WISE", "above 8192", "Not built: ranking in the sharded calls", "a per-capture ranking record in a batch",
                   "terms that need the cloud", "reordering of inlier_idx_out", "tests/handle_ranking_cases.py"):
        assert phrase in block, phrase
    for doc, phrases in (("DESIGN.md", ("### Handle ranking", "k_handle_rank", "VGPRs", "LDS", "Not built: ranking in the sharded calls")),
                         ("README.md", ("agh_set_handle_ranking", "set_handle_ranking", "--rank")),
                         ("INTEGRATION.md", ("setHandleRanking", "handleScores"))):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(p in text for p in phrases), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Not built: ranking or scoring of handles" not in design  # (struck: it is built)
