"""agh_default_depth_fusion_params, agh_fuse_depth, agh_fuse_depth_device, agh_get_depth_fusion_counts and agh_get_fused_depth
(include/agh.h): declared with the documented signatures, the records laid out as the binding has them, exported by the library,
refused without a context before any device call; the header states the contract's numbered rules and lists the calls in both
mid-chain paragraphs; the library holds the kernel and the documents describe the call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_cpp_adapter import ROOT

NAMES = ("agh_fuse_depth", "agh_fuse_depth_device", "agh_get_depth_fusion_counts", "agh_get_fused_depth")

SRC = r"""
#include <cstddef>
#include <type_traits>
#include "agh.h"
typedef void (*default_fn)(agh_depth_fusion_params*);
typedef int (*fuse_fn)(agh_ctx*, const agh_depth_image*, int32_t, const agh_depth_fusion_params*, int32_t, agh_depth_image*);
typedef int (*counts_fn)(agh_ctx*, int32_t, agh_depth_fusion_counts*);
typedef int (*get_fn)(agh_ctx*, int32_t, void*, int64_t, agh_depth_image*);
static_assert(std::is_same<decltype(&agh_default_depth_fusion_params), default_fn>::value, "agh_default_depth_fusion_params");
static_assert(std::is_same<decltype(&agh_fuse_depth), fuse_fn>::value, "agh_fuse_depth");
static_assert(std::is_same<decltype(&agh_fuse_depth_device), fuse_fn>::value, "agh_fuse_depth_device");
static_assert(std::is_same<decltype(&agh_get_depth_fusion_counts), counts_fn>::value, "agh_get_depth_fusion_counts");
static_assert(std::is_same<decltype(&agh_get_fused_depth), get_fn>::value, "agh_get_fused_depth");
static_assert(std::is_same<decltype(agh_depth_fusion_params::min_valid), int32_t>::value, "min_valid");
static_assert(std::is_same<decltype(agh_depth_fusion_params::max_spread_rel), double>::value, "max_spread_rel");
static_assert(std::is_same<decltype(agh_depth_fusion_counts::n_filled), int64_t>::value, "n_filled");
static_assert(sizeof(agh_depth_fusion_params) == %d && sizeof(agh_depth_fusion_counts) == %d, "sizes");
static_assert(sizeof(agh_depth_filter_params) == 40 && sizeof(agh_depth_filter_counts) == 32, "the depth filter's records are frozen");
int main() { return 0; }
"""


def _header():
    return open(os.path.join(ROOT, "include", "agh.h")).read()


def test_header_declares_the_calls_and_the_records_match_the_binding(tmp_path):
    hdr = _header()
    from agile_grasp_amd import binding

    lib = binding.load_library()
    assert re.search(r"\bvoid agh_default_depth_fusion_params\(", hdr)
    for fn in NAMES:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    for fn in NAMES + ("agh_default_depth_fusion_params",):
        assert hasattr(lib, fn) and fn in binding.EXPORTS, fn
    P, K = binding.AghDepthFusionParams, binding.AghDepthFusionCounts
    assert [n for n, _ in P._fields_] == ["min_valid", "reserved", "max_spread_abs", "max_spread_rel"]
    assert [n for n, _ in K._fields_] == ["n_pixels", "n_empty", "n_unsupported", "n_inconsistent", "n_fused", "n_filled"]
    assert (C.sizeof(P), C.sizeof(K)) == (24, 48)
    offsets = "".join(f'static_assert(offsetof(agh_depth_fusion_params, {n}) == {getattr(P, n).offset}, "{n}");\n' for n, _ in P._fields_)
    offsets += "".join(f'static_assert(offsetof(agh_depth_fusion_counts, {n}) == {getattr(K, n).offset}, "{n}");\n' for n, _ in K._fields_)
    src = tmp_path / "sig.cpp"
    src.write_text((SRC % (C.sizeof(P), C.sizeof(K))).replace("int main()", offsets + "int main()"))
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    csrc = tmp_path / "c.c"  # (the header stays a C header)
    csrc.write_text('#include "agh.h"\nint main(void) { agh_depth_fusion_params p; agh_default_depth_fusion_params(&p); '
                    'return p.min_valid; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(csrc)])
    for method in ("fuse_depth", "depth_fusion_counts", "fused_depth"):
        assert callable(getattr(binding.Context, method)), method


def test_every_export_is_in_the_library_and_the_library_has_the_kernel():
    from agile_grasp_amd import binding, build

    lib = binding.load_library()
    for fn in binding.EXPORTS:
        assert hasattr(lib, fn), fn
    blob = open(lib._name, "rb").read()
    assert b"k_depth_fuse" in blob and b"k_deproject" in blob  # (the native kernel, not a fall-back)
    # depth_fuse.hip is part of depth.hip's translation unit, and a change to it rebuilds the library
    depth = open(os.path.join(ROOT, "agile_grasp_amd", "csrc", "depth.hip")).read()
    assert '#include "depth_fuse.hip"' in depth and "depth.hip" in build.SRC and "depth_fuse.hip" not in build.SRC
    assert "depth_fuse.hip" in open(build.__file__).read().split("def needs_build")[1].split("def build")[0]


def test_defaults_a_null_context_and_the_device_image_handle():
    from agile_grasp_amd import binding

    lib = binding.load_library()
    fp = binding.depth_fusion_params()
    assert (fp.min_valid, fp.reserved, fp.max_spread_abs, fp.max_spread_rel) == (2, 0, 0.005, 0.005)
    got = binding.depth_fusion_params(min_valid=3, max_spread_rel=0.0)
    assert (got.min_valid, got.max_spread_abs, got.max_spread_rel) == (3, 0.005, 0.0)
    lib.agh_default_depth_fusion_params(None)  # (ignored)
    with pytest.raises(TypeError):
        binding.depth_fusion_params(spread=0.5)
    bad = binding.AGH_ERR_INVALID_ARGUMENT
    frame, out, counts = binding.AghDepthImage(), binding.AghDepthImage(), binding.AghDepthFusionCounts()
    for fn in (lib.agh_fuse_depth, lib.agh_fuse_depth_device):
        assert fn(None, C.byref(frame), C.c_int32(1), C.byref(fp), C.c_int32(0), C.byref(out)) == bad
    assert lib.agh_get_depth_fusion_counts(None, C.c_int32(0), C.byref(counts)) == bad
    assert lib.agh_get_fused_depth(None, C.c_int32(0), None, C.c_int64(0), C.byref(out)) == bad
    # the handle of a fused image goes through depth_image_records exactly as a CUDA tensor does
    rec = binding.AghDepthImage()
    rec.data, rec.width, rec.height, rec.row_stride_bytes, rec.format = 0x7f0000001000, 65, 3, 65 * 4, binding.DEPTH_F32
    handle = binding.DeviceImage(rec)
    recs, keep, on_device = binding.depth_image_records([dict(data=handle, fx=1.0, fy=1.0, cx=0.0, cy=0.0, pose=[0.0] * 12)])
    assert on_device and keep == [handle]
    assert (recs[0].data, recs[0].width, recs[0].height, recs[0].row_stride_bytes, recs[0].format) == (0x7f0000001000, 65, 3, 260, binding.DEPTH_F32)
    rec.format, rec.row_stride_bytes = binding.DEPTH_U16, 65 * 2
    recs, _, _ = binding.depth_image_records([dict(data=binding.DeviceImage(rec), fx=1.0, fy=1.0, cx=0.0, cy=0.0, pose=[0.0] * 12)])
    assert (recs[0].row_stride_bytes, recs[0].format) == (130, binding.DEPTH_U16)


def test_header_block_mid_chain_lists_and_documents():
    hdr = _header()
    single = hdr[hdr.index("Between begin and end the chain owns"):hdr.index("int agh_localize_begin(")]
    batch = hdr[hdr.index("The context has ONE chain and ONE staged set, of either kind."):hdr.index("int agh_localize_batch_begin(")]
    allowed, refused = single.split("may be called on the context")
    for name in NAMES:
        assert re.search(name + r"\b(?!_)", refused) and name not in allowed, name
        assert re.search(name + r"\b(?!_)", batch.split("AGH_ERR_STATE, the chain untouched")[0]), name
    start = hdr.index("DEPTH FUSION:")
    assert hdr.index("int agh_get_depth_filter_counts(") < start < hdr.index("A VOXEL FILTER")  # the block stands behind the depth filter's
    block = re.sub(r"\n \*\s+", " ", hdr[start:hdr.index("typedef struct agh_depth_fusion_params")])
    for phrase in ("ONE fixed camera", "n_frames (1 .. 16)", "row strides may differ per frame", "BIT-EQUAL", "mixing cameras must not pass silently",
                   "sa = (float) max_spread_abs", "sr = (float) max_spread_rel", "independently of every other pixel", "ascending frame index",
                   "1. READING AND VALIDITY", "valid iff raw != 0", "0 < z < +inf", "both zeros and +inf are invalid",
                   "2. MEDIAN", "LOWER median", "(m - 1) / 2", "the nearer surface wins",
                   "3. CONSENSUS", "tol = sa + (sr * zm)", "left to right, never contracted", "fabsf(z - zm) <= tol", "the comparison is closed",
                   "The median is always a member", "the result is the median",
                   "4. DECISION", "m == 0: EMPTY", "m < min_valid: UNSUPPORTED", "k < min_valid: INCONSISTENT", "Otherwise FUSED",
                   "U16 writes 0, F32 writes a quiet NaN",
                   "5. VALUE", "(sum + k / 2) / k", "16 x 65535", "in frame order", "correctly rounded float32 division", "still counts as FUSED",
                   "6. OUTPUT", "tight rows", "row_stride_bytes = width x element size", "of frame 0", "every agh_*depth*_device call of the same context",
                   "until that slot is fused again or the context is destroyed",
                   "7. COUNTS", "n_pixels = n_empty + n_unsupported + n_inconsistent + n_fused", "LAST frame was invalid",
                   "SLOTS run 0 .. 127", "regrown when an image is larger",
                   "returns without waiting for the kernel", "needs no synchronisation in between", "have been READ, pageable or page-locked",
                   "until the next synchronisation of the context", "pinned memory", "AGH_ERR_CAPACITY",
                   "nothing launched and the slot's previous image untouched", "the default of 2 with ONE frame is therefore refused",
                   "non-finite or negative", "a non-zero reserved", "differs from frame 0",
                   "MID-CHAIN", "AGH_ERR_STATE without touching anything",
                   "Not built: fusing the next burst under a chain in flight", "a ring of frames", "motion compensation", "spatial hole filling",
                   "confidence outputs", "tests/depth_fusion_cases.py"):
        assert phrase in block, phrase
    for doc, phrases in (("DESIGN.md", ("### Depth fusion", "k_depth_fuse", "VGPRs", "ScratchSize", "Not built", "a burst is fused ahead of it: agh_fuse_depth")),
                         ("README.md", ("agh_fuse_depth", "fuse_depth", "fuseDepth")),
                         ("INTEGRATION.md", ("fuseDepth", "agh_fuse_depth_device", "agh_get_depth_fusion_counts"))):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(p in text for p in phrases), (doc, [p for p in phrases if p not in text])
    assert "a burst is fused ahead of it: agh_fuse_depth" in re.sub(r"\n \*\s+", " ", hdr)
