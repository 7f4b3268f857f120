"""The depth filter (agh_set_depth_filter) on and off, on the same build: two 640 x 480 uint16 depth images of the raw-cloud scene
(tests/depth_captures.render_depth) with about 1 % of their pixels turned into flying pixels -- every tenth pixel in both
directions that the filter keeps and whose raw value exceeds 400, pulled 150 units (15 cm) towards the camera -- 2000 drawn
samples, classifier on.  Per call, ms:
  depth            agh_localize_depth, no filter
  depth_filtered   the same call with the default filter set (3 x 3 window, 3 supporters, 1 cm + 1 % of the depth)
  batch            agh_localize_depth_batch over eight such captures (capture k: every reading 4 k mm further away), no filter
  batch_filtered   the same call with the filter set
The variants take turns (A B C D A B C D ...) in one process on one context, --reps rounds after 3 warm-up rounds; the filter is
set or cleared outside the timed part.  `depth` runs twice per round (depth and depth_again): the spread between its own two
medians is the yardstick for every difference.  The hypothesis counts of both settings are recorded.  Every sample is written to
--out as JSON, the medians are printed as one JSON line.
--trace N: just N single calls without and N with the filter, the workload of a kernel trace taken in a run of its own
  (rocprofv3 --kernel-trace --stats -d DIR -- python scripts/localize_depth_filter_bench.py --trace 20); --kernels FILE merges the
  k_deproject* rows of scripts/rocpd_summary.py's CSV for that run into --out (k_deproject_filtered's time against k_deproject's on
  the same images in the same trace: a ratio that is reported, not gated -- a few-microsecond kernel is within launch noise)."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding, synthetic
from tests import depth_captures as D
from tests import depth_filter_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inject(images, fp, step=10):
    out, n_inj = [], 0
    for im in images:
        d = np.array(im["data"])
        grid = np.zeros(d.shape, bool)
        grid[::step, ::step] = True
        inj = grid & FC.filter_image(im, fp)["keep"] & (d > 400)
        d[inj] -= 150
        n_inj += int(inj.sum())
        out.append(dict(im, data=d))
    return out, n_inj


def shifted(images, k):
    return [dict(im, data=np.where(im["data"] > 0, im["data"] + 4 * k, 0).astype(np.uint16)) for im in images]


def merge_kernels(path, out_path):
    rows = {}
    for r in csv.DictReader(line for line in open(path) if not line.startswith("#")):
        if "k_deproject" in r["kernel"]:
            rows[r["kernel"].replace(".kd", "")] = {"calls": int(r["calls"]), "avg_us": float(r["avg_us"]), "min_us": float(r["min_us"]),
                                                    "max_us": float(r["max_us"])}
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out["kernel_trace"] = rows
    if "k_deproject" in rows and "k_deproject_filtered" in rows:
        out["kernel_trace"]["filtered_over_plain"] = round(rows["k_deproject_filtered"]["avg_us"] / rows["k_deproject"]["avg_us"], 3)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_depth_filter_bench.json"))
    ap.add_argument("--trace", type=int, default=0, help="N: just N single calls without and N with the filter (a kernel trace's workload)")
    ap.add_argument("--kernels", default=None, help="a scripts/rocpd_summary.py CSV of a --trace run: merge its k_deproject* rows into --out")
    a = ap.parse_args()
    if a.kernels:
        return merge_kernels(a.kernels, a.out)

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    clean = [D.render_depth(views[k], k, 640, 480, D.U16, 520.0) for k in range(2)]
    fp = FC.params()
    images, n_inj = inject(clean, fp)
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in images])
    caps = [shifted(images, k) for k in range(8)]
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    kw = dict(n_samples=2000, sample_seed=7, classify=True, min_inliers=3, min_length=0.005)
    bkw = dict(n_samples=[2000] * 8, sample_seeds=[7 + k for k in range(8)], classify=True, min_inliers=3, min_length=0.005)
    counts = {}

    def variant(filtered, fn):
        def run():
            if filtered:
                ctx.set_depth_filter(**fp)
            else:
                ctx.clear_depth_filter()
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            if filtered:
                counts["last"] = ctx.depth_filter_counts()
            return r, dt
        return run

    single = lambda: ctx.localize_depth(images, ws, **kw)
    batch = lambda: ctx.localize_depth_batch(caps, [ws] * 8, **bkw)
    if a.trace:
        for filtered in (False, True):
            run = variant(filtered, single)
            for _ in range(a.trace):
                run()
        print(json.dumps({"trace_calls_each": a.trace}))
        return
    variants = [("depth", variant(False, single)), ("depth_filtered", variant(True, single)), ("batch", variant(False, batch)),
                ("batch_filtered", variant(True, batch)), ("depth_again", variant(False, single))]
    samples = {name: [] for name, _ in variants}
    first = {}
    for rep in range(-3, a.reps):
        for name, fn in variants:
            r, dt = fn()
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
            if name not in first:
                first[name] = r
                if name == "depth_filtered":
                    counts["single"] = counts["last"]
                if name == "batch_filtered":
                    counts["batch"] = counts["last"]
    # the filter's counts are the model's, and the unfiltered call sees the injected pixels as voxels
    model = np.stack([FC.filter_image(im, fp)["counts"] for im in images])
    assert np.array_equal(counts["single"], model) and len(counts["batch"]) == 16
    assert first["depth"]["n_voxels"] != first["depth_filtered"]["n_voxels"]
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}

    def summary(r):
        return {"n_voxels": int(r["n_voxels"]), "n_hypotheses": int(r["n_hypotheses"]), "n_hands": len(r["hands"]), "n_handles": len(r["handles"])}

    out = {"capture": "2 x 640x480 uint16, f = 520 px", "n_pixels": int(sum(im["data"].size for im in images)),
           "n_injected": n_inj, "injected_fraction_of_valid": round(n_inj / float(model[:, 0].sum()), 4),
           "filter": {k: (v if np.isfinite(v) else "inf") for k, v in fp.items()},
           "filter_counts": {n: [int(x) for x in model[:, i]] for i, n in enumerate(FC.COUNT_NAMES)},
           "n_samples": 2000, "single": {"unfiltered": summary(first["depth"]), "filtered": summary(first["depth_filtered"])},
           "batch": {"unfiltered": {"n_hypotheses": [int(r["n_hypotheses"]) for r in first["batch"]]},
                     "filtered": {"n_hypotheses": [int(r["n_hypotheses"]) for r in first["batch_filtered"]]}},
           "reps": a.reps, "median_ms": med, "samples_ms": samples}
    if os.path.exists(a.out):  # (a kernel trace merged earlier stays)
        old = json.load(open(a.out))
        if "kernel_trace" in old:
            out["kernel_trace"] = old["kernel_trace"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
