"""agh_default_voxel_filter_params, agh_set_voxel_filter, agh_get_voxel_filter and agh_get_voxel_filter_counts (include/agh.h):
declared with the documented signatures, the records laid out as the binding has them, exported by the library, refused without a
context before any device call; the header carries the contract's ten rules and lists the calls in its two mid-chain paragraphs;
the adapter's methods compile in both type branches.  On the GPU: defaults and the get / set / clear round trip, every refused
field with the field named and the old filter kept, and the counts call's return values."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_set_voxel_filter", "agh_get_voxel_filter", "agh_get_voxel_filter_counts")

SRC = r"""
#include <cstddef>
#include <type_traits>
#include "agh.h"
typedef void (*default_fn)(agh_voxel_filter_params*);
typedef int (*set_fn)(agh_ctx*, const agh_voxel_filter_params*);
typedef int (*get_fn)(agh_ctx*, agh_voxel_filter_params*);
typedef int (*counts_fn)(agh_ctx*, agh_voxel_filter_counts*, int32_t);
static_assert(std::is_same<decltype(&agh_default_voxel_filter_params), default_fn>::value, "agh_default_voxel_filter_params");
static_assert(std::is_same<decltype(&agh_set_voxel_filter), set_fn>::value, "agh_set_voxel_filter");
static_assert(std::is_same<decltype(&agh_get_voxel_filter), get_fn>::value, "agh_get_voxel_filter");
static_assert(std::is_same<decltype(&agh_get_voxel_filter_counts), counts_fn>::value, "agh_get_voxel_filter_counts");
static_assert(std::is_same<decltype(agh_voxel_filter_params::radius), int32_t>::value, "radius");
static_assert(std::is_same<decltype(agh_voxel_filter_params::min_neighbors), int32_t>::value, "min_neighbors");
static_assert(std::is_same<decltype(agh_voxel_filter_counts::n_kept), int64_t[2]>::value, "n_kept");
static_assert(sizeof(agh_voxel_filter_params) == %d && sizeof(agh_voxel_filter_counts) == %d, "sizes");
static_assert(offsetof(agh_voxel_filter_params, radius) == %d && offsetof(agh_voxel_filter_params, min_neighbors) == %d, "parameter offsets");
static_assert(offsetof(agh_voxel_filter_counts, n_occupied) == %d && offsetof(agh_voxel_filter_counts, n_pruned) == %d &&
  offsetof(agh_voxel_filter_counts, n_kept) == %d, "counter offsets");
int main() { return 0; }
"""


def _header():
    return open(os.path.join(ROOT, "include", "agh.h")).read()


def test_header_declares_the_calls_and_the_records_match_the_binding(tmp_path):
    hdr = _header()
    from agile_grasp_amd import binding

    lib = binding.load_library()
    assert re.search(r"\bvoid agh_default_voxel_filter_params\(", hdr)
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    for fn in NAMES + ("agh_default_voxel_filter_params",):
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    P, K = binding.AghVoxelFilterParams, binding.AghVoxelFilterCounts
    assert [n for n, _ in P._fields_] == ["radius", "min_neighbors"]
    assert [n for n, _ in K._fields_] == ["n_occupied", "n_pruned", "n_kept"]
    assert (C.sizeof(P), C.sizeof(K)) == (8, 48)
    src = tmp_path / "sig.cpp"
    src.write_text(SRC % ((C.sizeof(P), C.sizeof(K)) + tuple(getattr(P, n).offset for n, _ in P._fields_)
                          + tuple(getattr(K, n).offset for n, _ in K._fields_)))
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    csrc = tmp_path / "c.c"  # (the header stays a C header)
    csrc.write_text('#include "agh.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])
    for method in ("set_voxel_filter", "clear_voxel_filter", "voxel_filter", "voxel_filter_counts"):
        assert callable(getattr(binding.Context, method)), method


def test_defaults_and_a_null_context():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    fp = binding.voxel_filter_params()
    assert (fp.radius, fp.min_neighbors) == (2, 4)
    assert binding.voxel_filter_params(radius=3).radius == 3
    lib.agh_default_voxel_filter_params(None)  # (ignored)
    with pytest.raises(TypeError):
        binding.voxel_filter_params(min_support=3)
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    counts = (binding.AghVoxelFilterCounts * 2)()
    assert lib.agh_set_voxel_filter(None, C.byref(fp)) == bad and lib.agh_set_voxel_filter(None, None) == bad
    assert lib.agh_get_voxel_filter(None, C.byref(fp)) == bad
    assert lib.agh_get_voxel_filter_counts(None, counts, C.c_int32(2)) == bad


def test_header_block_and_mid_chain_lists():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in ("agh_set_voxel_filter", "agh_get_voxel_filter_counts"):
        assert name in refused and name not in allowed, name
        assert name in batch.split("AGH_ERR_STATE, the chain untouched")[0], name
    assert re.search(r"agh_get_voxel_filter\b(?!_)", allowed)  # (host-side, like agh_get_depth_filter)
    start = hdr.index("A VOXEL FILTER for every call that voxelises")
    assert hdr.index("int agh_get_depth_filter_counts(") < start  # the block stands behind the depth filter's
    block = hdr[start:hdr.index("void agh_default_voxel_filter_params(")]
    assert [int(x) for x in re.findall(r"^ \* {1,2}(\d+)\. ", block, re.M)] == list(range(1, 11))  # the ten rules
    block = re.sub(r"\n \*\s+", " ", block)
    for phrase in ("the filter never moves the minimum", "UNFILTERED voxel list with rows taken out", "NOT the voxelisation of the raw points that survive",
                   "dx^2 + dy^2 + dz^2 <= radius^2", "7, 33, 123, 257", "Positions outside the lattice", "never support one another",
                   "never on the filter's own output", "not iterated", "SURVIVING voxel", "sticky", "after the depth filter",
                   "_begin / _stage / _end", "the lattice outgrew the bitmap", "the two ints travel as kernel arguments",
                   "every launch is exactly what it was", "the text names the field", "the filter held before stays in force",
                   "AGH_ERR_STATE", "AGH_ERR_CAPACITY", "n_occupied = n_pruned + n_kept", "zero voxels, empty lists, no error",
                   "2^28 words", "SECOND bitmap", "memory doubles"):
        assert phrase in block, phrase
    not_built = block[block.index("Not built:"):]
    for phrase in ("iterated or statistical", "across cameras or captures", "per-capture parameters", "agh_set_cloud*"):
        assert phrase in not_built, phrase
    depth = hdr[hdr.index("A DEPTH FILTER for every call"):hdr.index("void agh_default_depth_filter_params(")]
    assert "a filter for the points" not in re.sub(r"\n \*\s+", " ", depth)  # (built now: this block)
    for doc, phrases in (("DESIGN.md", ("## Voxel filter", "k_vox_prune", "k_mask_mark", "k_label_mark", "second bitmap")),
                         ("README.md", ("agh_set_voxel_filter", "set_voxel_filter"))):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(p in text for p in phrases), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "a filter for the points forms" not in re.sub(r"\s+", " ", design)


@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_methods_compile_in_both_type_branches(real_types):
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "voxel_filter_adapter_test.cpp")])
    for hdr in ("hand_search.h", "localization.h"):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in ("setVoxelFilter", "clearVoxelFilter", "voxelFilter(", "voxelFilterCounts")), hdr
    example = open(os.path.join(ROOT, "examples", "localize_pcd.cpp")).read()
    assert "--voxel-filter" in example and "setVoxelFilter" in example


@pytest.mark.gpu
def test_round_trip_and_every_refusal_names_its_field_and_keeps_the_old_filter():
    from agile_grasp_amd import binding
    from tests import voxel_filter_cases as VF

    ctx = binding.Context(np.zeros((2, 3)))
    assert ctx.voxel_filter() is None and ctx.voxel_filter_counts().shape == (0, 6)
    ctx.set_voxel_filter()
    assert (ctx.voxel_filter().radius, ctx.voxel_filter().min_neighbors) == (2, 4)
    ctx.set_voxel_filter(binding.voxel_filter_params(radius=3), min_neighbors=7)
    assert (ctx.voxel_filter().radius, ctx.voxel_filter().min_neighbors) == (3, 7)
    ctx.clear_voxel_filter()
    assert ctx.voxel_filter() is None
    c = VF.cases()["seams"]
    ctx.set_voxel_filter(radius=c["radius"], min_neighbors=c["min_neighbors"])
    for field, values in (("radius", (0, 5, -1)), ("min_neighbors", (0, 33, -2))):
        for v in values:
            with pytest.raises(binding.AghError) as e:
                ctx.set_voxel_filter(**{"radius": c["radius"], "min_neighbors": c["min_neighbors"], field: v})
            assert e.value.code == binding.AGH_ERR_INVALID_ARGUMENT and "agh_set_voxel_filter: " + field in str(e.value), (field, v)
    for r, top in ((1, 6), (2, 32), (3, 122), (4, 256)):  # B(radius) - 1 follows the radius
        with pytest.raises(binding.AghError) as e:
            ctx.set_voxel_filter(radius=r, min_neighbors=top + 1)
        assert "min_neighbors" in str(e.value)
    held = ctx.voxel_filter()
    assert (held.radius, held.min_neighbors) == (c["radius"], c["min_neighbors"])
    for r, top in ((1, 6), (4, 256)):
        ctx.set_voxel_filter(radius=r, min_neighbors=top)
    # the counts call: 0 before any voxelisation, the captures after a filtered one, AGH_ERR_CAPACITY, 0 after an unfiltered one
    recs = (binding.AghVoxelFilterCounts * 1)()
    assert ctx.lib.agh_get_voxel_filter_counts(ctx._h, recs, C.c_int32(1)) == 0
    ctx.set_voxel_filter(radius=c["radius"], min_neighbors=c["min_neighbors"])
    ctx.preprocess(c["points"], c["size_left"], c["workspace"], c["cell"], dense=True)
    assert ctx.lib.agh_get_voxel_filter_counts(ctx._h, recs, C.c_int32(1)) == 1
    m = VF.case_model(c)
    assert list(recs[0].n_occupied) + list(recs[0].n_pruned) + list(recs[0].n_kept) == m["counts"].tolist()
    assert ctx.lib.agh_get_voxel_filter_counts(ctx._h, recs, C.c_int32(0)) == binding.AGH_ERR_CAPACITY
    assert ctx.lib.agh_get_voxel_filter_counts(ctx._h, None, C.c_int32(1)) == binding.AGH_ERR_CAPACITY
    ctx.clear_voxel_filter()
    ctx.preprocess(c["points"], c["size_left"], c["workspace"], c["cell"], dense=True)
    assert ctx.lib.agh_get_voxel_filter_counts(ctx._h, recs, C.c_int32(1)) == 0
    ctx.close()
