"""The hand filter (agh_set_hand_filter) on and off, on the same build: two 640 x 480 uint16 depth images of the raw-cloud scene
(tests/depth_captures.render_depth), 2000 drawn samples, classifier on.  Per call, ms:
  depth / batch             agh_localize_depth / agh_localize_depth_batch over eight such captures (capture k: every reading
                            4 k mm further away), no filter
  depth_ca / batch_ca       the same calls with the approach cone (top-down, cos >= 0.5) and the aperture (2 .. 6.2 cm)
  depth_all / batch_all     ... and the observed-space criterion (4 probes per finger, 1 cm margin, at most 9 unobserved)
  depth_host / batch_host   the host route the filter replaces: the unfiltered call with min_inliers = 2^30, so that its handle
                            search forms no handle (the library has no chain form without one: its pair matrix is still built,
                            which this route pays and a true "chain without handle search" would not), the cone and the aperture
                            on the returned hands in numpy, agh_find_handles on the survivors (per capture for the batch).  It
                            classifies every hand.
The variants take turns (A B C ... A B C ...) in one process on one context, --reps rounds after 3 warm-up rounds; the filter is
set or cleared outside the timed part.  `depth` runs twice per round (depth and depth_again): the spread between its own two
medians is the yardstick for every difference.  Medians, minima and maxima are printed as one JSON line; every sample, the
hypothesis, hand and handle counts and the filter's counts go to --out as JSON.
--off-only: just the unfiltered variants, through nothing but calls an older build has too; with --root DIR the package of
  another checkout (the parent commit's build) is timed by this same script in the same session; --merge-parent FILE puts such a
  run's medians into --out as "parent_off_leg" (this build's own second --off-only run is kept as "second_off_leg").
--trace N: just N single calls with all three criteria, the workload of a kernel trace taken in a run of its own
  (rocprofv3 --kernel-trace --stats -d DIR -- python scripts/localize_hand_filter_bench.py --trace 20); --kernels FILE merges
  the k_hand_filter, k_hog_svm and k_compact_kept rows of scripts/rocpd_summary.py's CSV for that run into --out."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def merge_kernels(path, out_path):
    rows = {}
    for r in csv.DictReader(line for line in open(path) if not line.startswith("#")):
        if any(k in r["kernel"] for k in ("k_hand_filter", "k_hog_svm", "k_compact_kept")):
            rows[r["kernel"].replace(".kd", "").split("(")[0]] = {"calls": int(r["calls"]), "avg_us": float(r["avg_us"]),
                                                                  "min_us": float(r["min_us"]), "max_us": float(r["max_us"])}
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out["kernel_trace"] = rows
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_hand_filter_bench.json"))
    ap.add_argument("--root", default=ROOT, help="the checkout whose agile_grasp_amd is timed (default: this one)")
    ap.add_argument("--off-only", action="store_true", help="only the unfiltered variants (an older build has no filter)")
    ap.add_argument("--trace", type=int, default=0, help="N: just N single calls with all three criteria")
    ap.add_argument("--kernels", default=None, help="a scripts/rocpd_summary.py CSV of a --trace run: merge its rows into --out")
    ap.add_argument("--merge-parent", default=None, help="the --out of an --off-only run of the parent's build: merge its medians")
    a = ap.parse_args()
    if a.kernels:
        return merge_kernels(a.kernels, a.out)
    if a.merge_parent:
        out = json.load(open(a.out))
        out.setdefault("parent_off_leg", []).append(json.load(open(a.merge_parent))["ms"])
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    sys.path.insert(0, ROOT)  # (tests.depth_captures is this checkout's, whichever package is timed)
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np

    from agile_grasp_amd import binding, synthetic
    from tests import depth_captures as D

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    images = [D.render_depth(views[k], k, 640, 480, D.U16, 520.0) for k in range(2)]
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in images])

    def shifted(k):
        return [dict(im, data=np.where(im["data"] > 0, im["data"] + 4 * k, 0).astype(np.uint16)) for im in images]

    caps = [shifted(k) for k in range(8)]
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    kw = dict(n_samples=2000, sample_seed=7, classify=True, min_inliers=3, min_length=0.005)
    bkw = dict(n_samples=[2000] * 8, sample_seeds=[7 + k for k in range(8)], classify=True, min_inliers=3, min_length=0.005)
    p = synthetic.to_scene_frame(np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 0.0]]))
    down = (p[0] - p[1]) / np.linalg.norm(p[0] - p[1])
    ca = dict(approach_on=1, approach_dir=tuple(float(x) for x in down), min_approach_cos=0.5, width_on=1, min_width=0.02, max_width=0.062)
    filters = {"off": None, "ca": ca, "all": dict(ca, view_on=1, probes_per_finger=4, depth_margin=0.01, max_unobserved=9)}
    counts = {}

    def host_filter(hands):
        a3 = hands["approach"]
        dot = (a3[:, 0] * down[0] + a3[:, 1] * down[1]) + a3[:, 2] * down[2]
        return hands[~(dot < ca["min_approach_cos"]) & ~((hands["width"] < ca["min_width"]) | (hands["width"] > ca["max_width"]))]

    def variant(mode, fn, host=False):
        def run():
            if not a.off_only:
                if filters[mode] is None:
                    ctx.clear_hand_filter()
                else:
                    ctx.set_hand_filter(**filters[mode])
            t0 = time.perf_counter()
            r = fn()
            if host:
                for q in (r if isinstance(r, list) else [r]):
                    q["hands"] = host_filter(q["hands"])
                    q["handles"], q["inlier_idx"] = ctx.find_handles(q["hands"], 3, 0.005)
            dt = time.perf_counter() - t0
            if filters[mode] is not None:
                counts["last"] = ctx.hand_filter_counts()
            return r, dt
        return run

    single = lambda: ctx.localize_depth(images, ws, **kw)
    batch = lambda: ctx.localize_depth_batch(caps, [ws] * 8, **bkw)
    single_no_handles = lambda: ctx.localize_depth(images, ws, **dict(kw, min_inliers=1 << 30))
    batch_no_handles = lambda: ctx.localize_depth_batch(caps, [ws] * 8, **dict(bkw, min_inliers=1 << 30))
    if a.trace:
        run = variant("all", single)
        for _ in range(a.trace):
            run()
        print(json.dumps({"trace_calls": a.trace}))
        return
    variants = [("depth", variant("off", single)), ("depth_ca", variant("ca", single)), ("depth_all", variant("all", single)),
                ("depth_host", variant("off", single_no_handles, host=True)), ("batch", variant("off", batch)),
                ("batch_ca", variant("ca", batch)), ("batch_all", variant("all", batch)),
                ("batch_host", variant("off", batch_no_handles, host=True)), ("depth_again", variant("off", single))]
    if a.off_only:
        variants = [v for v in variants if v[0] in ("depth", "batch", "depth_again")]
    samples = {name: [] for name, _ in variants}
    first = {}
    for rep in range(-3, a.reps):
        for name, fn in variants:
            r, dt = fn()
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
            if name not in first:
                first[name] = r
                if name.endswith(("_ca", "_all")):
                    counts[name] = counts["last"]
    stats = {name: {"median": round(float(np.median(t)), 4), "min": min(t), "max": max(t)} for name, t in samples.items()}

    def summary(r):
        if isinstance(r, list):
            return [summary(q) for q in r]
        return {"n_voxels": int(r["n_voxels"]), "n_hypotheses": int(r["n_hypotheses"]), "n_hands": len(r["hands"]), "n_handles": len(r["handles"])}

    out = {"capture": "2 x 640x480 uint16, f = 520 px", "n_samples": 2000, "sample_seed": 7, "reps": a.reps,
           "root": os.path.relpath(os.path.abspath(a.root), ROOT), "results": {name: summary(r) for name, r in first.items()},
           "ms": stats, "samples_ms": samples}
    if not a.off_only:
        out["filters"] = {k: v for k, v in filters.items() if v}
        names = ("n_hypotheses", "n_dropped_approach", "n_dropped_width", "n_dropped_unobserved", "n_kept")
        out["filter_counts"] = {k: [dict(zip(names, (int(x) for x in row))) for row in v] for k, v in counts.items() if k != "last"}
        # the device route with cone + aperture returns what the host route returns
        assert summary(first["depth_ca"]) == summary(first["depth_host"]) and summary(first["batch_ca"]) == summary(first["batch_host"])
    if os.path.exists(a.out):  # (a kernel trace or a parent leg merged earlier stays)
        old = json.load(open(a.out))
        for key in ("kernel_trace", "parent_off_leg", "second_off_leg"):
            if key in old:
                out[key] = old[key]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
