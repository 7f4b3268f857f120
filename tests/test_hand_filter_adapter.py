"""The adapter's hand-filter methods RUN (tests/test_hand_filter_abi.py only compiles them): Localization::setHandFilter and its
family through localizeHandles on the two-view box capture of tests/hand_filter_cases.py as points -- the counts and the kept
hands are the numpy model's, the setting is sticky across a re-created search, refused while a chain is pending, a points call
with the observed-space criterion fails, and cleared it gives the unfiltered chain back (tests/cpp/hand_filter_adapter_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_cpp_adapter import GOLD, ROOT, _dump_raw

SVM = os.path.join(GOLD, "svm_032015_linear_20_20_same")


def _build(tmp_path):
    from agile_grasp_amd import build

    build.build()
    exe = str(tmp_path / "hand_filter_adapter_test")
    libdir = os.path.join(ROOT, "agile_grasp_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "hand_filter_adapter_test.cpp"), "-o", exe, "-L" + libdir,
                           "-lagile_grasp_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_adapter_hand_filter_counts_stickiness_and_refusals(tmp_path, svm_model):
    from agile_grasp_amd import binding
    from tests import depth_captures as D
    from tests import hand_filter_cases as HF

    sc = HF.box_scene(2)
    f = HF.scene_filters(sc)["all"]
    fp = HF.params(**{k: v for k, v in f.items() if k != "view_on"})
    pts = D.deproject_ref(sc["images"])
    fin = np.isfinite(pts).all(1)
    left = sc["images"][0]["data"].size
    pts, left = pts[fin], int(fin[:left].sum())  # (the adapter removes NaN rows itself: hand it the finite ones, the split kept)
    path = str(tmp_path / "raw.bin")
    _dump_raw(path, pts, left, sc["samples"], sc["ws"], sc["origins"])
    args = [f"{x!r}" for x in fp["approach_dir"]] + [repr(fp["min_approach_cos"]), repr(fp["min_width"]), repr(fp["max_width"])]
    out = subprocess.run([_build(tmp_path), SVM, path] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-2000:])
    print(out.stdout[-600:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()
             if ln.split() and ln.split()[0] in ("COUNTS", "PLAIN", "FILTERED", "LOCALIZATION", "SEARCH")}
    # the same capture through the C ABI, stage-wise, with the numpy model between the search and the classifier
    ctx = binding.Context(sc["origins"])
    ctx.load_svm(*svm_model)
    ctx.preprocess(pts, left, sc["ws"])
    vox, _ = ctx.cloud()
    hyps = ctx.find_hands(sc["samples"])
    keep = ctx.classify().astype(bool)
    reason = HF.drop_reasons(hyps, vox[sc["samples"][hyps["sample"]]], fp)
    c = HF.counts(reason)
    assert c[1] >= 5 and c[2] >= 5 and c[4] >= 5
    assert [int(v) for v in lines["COUNTS"]] == c
    want = hyps[keep & (reason == 0)]
    got = [[float(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines() if ln.startswith("K ")]
    assert got == [[float(h["surface"][0]), float(h["surface"][1]), float(h["surface"][2]), float(h["width"])] for h in want]
    assert int(lines["FILTERED"][0]) == len(want) >= 1 and int(lines["PLAIN"][0]) == int(keep.sum()) > len(want)
    assert lines["LOCALIZATION"] == ["1"] * 13
    assert lines["SEARCH"] == ["1", "1", "0", "1"]  # (the last chain, after the clear, ran unfiltered: no counts)
    ctx.close()
