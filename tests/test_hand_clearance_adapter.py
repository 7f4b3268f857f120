"""The adapter's hand-clearance methods: Localization::setHandClearance and its family, HandSearch's same four, and the example's
--clearance flag compile in both type branches (tests/cpp/hand_clearance_adapter_test.cpp, examples/localize_pcd.cpp); and they
RUN through localizeHandles on the two-view box capture of tests/hand_filter_cases.py as points -- the counts and the kept hands
are the numpy model's, the setting is sticky across a re-created search, refused while a chain is pending, and cleared it gives
the chain without it back."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT, _dump_raw

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")
METHODS = ("setHandClearance", "clearHandClearance", "handClearance(", "handClearanceCounts")


@pytest.mark.parametrize("source", ["tests/cpp/hand_clearance_adapter_test.cpp", "examples/localize_pcd.cpp"])
@pytest.mark.parametrize("real_types", [False, True])
def test_adapter_and_example_compile_in_both_type_branches(real_types, source):
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")]
    if real_types:
        cmd += ["-DAGILE_GRASP_AMD_HAVE_PCL_EIGEN=1", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs")]
    subprocess.check_call(cmd + [os.path.join(ROOT, *source.split("/"))])
    for hdr in ("hand_search.h", "localization.h"):
        text = open(os.path.join(ROOT, "include", "agile_grasp_amd", hdr)).read()
        assert all(n in text for n in METHODS), hdr
    example = open(os.path.join(ROOT, "examples", "localize_pcd.cpp")).read()
    assert "--clearance near,far,half_w,half_h[,max_points]" in example and "setHandClearance" in example


def _build(tmp_path):
    from agile_grasp_amd import build

    build.build()
    exe = str(tmp_path / "hand_clearance_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "hand_clearance_adapter_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_adapter_program_links(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2  # (no arguments: it leaves before it touches a device)


@pytest.mark.gpu
def test_adapter_hand_clearance_counts_stickiness_and_refusals(tmp_path, svm_model):
    from agile_grasp_amd import binding
    from tests import depth_captures as D
    from tests import hand_clearance_cases as HC
    from tests import hand_filter_cases as HF

    sc = HF.box_scene(2)
    cp = HC.params()
    pts = D.deproject_ref(sc["images"])
    fin = np.isfinite(pts).all(1)
    left = sc["images"][0]["data"].size
    pts, left = pts[fin], int(fin[:left].sum())  # (the adapter removes NaN rows itself: hand it the finite ones, the split kept)
    path = str(tmp_path / "raw.bin")
    _dump_raw(path, pts, left, sc["samples"], sc["ws"], sc["origins"])
    args = [repr(cp[k]) for k in ("near_offset", "far_offset", "half_width", "half_height")] + [str(cp["max_points"])]
    out = subprocess.run([_build(tmp_path), SVM, path] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-600:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()
             if ln.split() and ln.split()[0] in ("COUNTS", "PLAIN", "CLEAR", "LOCALIZATION", "SEARCH")}
    # the same capture through the C ABI, stage-wise, with the numpy model between the search and the classifier
    ctx = binding.Context(sc["origins"])
    ctx.load_svm(*svm_model)
    ctx.preprocess(pts, left, sc["ws"])
    vox, _ = ctx.cloud()
    hyps = ctx.find_hands(sc["samples"])
    keep = ctx.classify().astype(bool)
    dropped = HC.drop(hyps, vox[sc["samples"][hyps["sample"]]], vox, cp)
    c = HC.counts(dropped)
    assert HC.bites(dropped)
    assert [int(v) for v in lines["COUNTS"]] == c
    want = hyps[keep & ~dropped]
    got = [[float(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines() if ln.startswith("K ")]
    assert got == [[float(h["surface"][0]), float(h["surface"][1]), float(h["surface"][2]), float(h["width"])] for h in want]
    assert int(lines["CLEAR"][0]) == len(want) >= 1 and int(lines["PLAIN"][0]) == int(keep.sum()) > len(want)
    assert lines["LOCALIZATION"] == ["1"] * 13
    assert lines["SEARCH"] == ["1", "1", "0", "1"]  # (the last chain, after the clear, ran without one: no counts)
    ctx.close()
