"""The hand clearance (agh_set_hand_clearance) on and off, on the same build: two 640 x 480 uint16 depth images of the raw-cloud
scene (tests/depth_captures.render_depth), 2000 drawn samples, classifier on.  Per call, ms:
  depth / batch             agh_localize_depth / agh_localize_depth_batch over eight such captures (capture k: every reading
                            4 k mm further away), nothing set
  depth_on / batch_on       the same calls with the default corridor (0 .. 12 cm behind the palm, +- 5 cm, +- 4 cm, empty)
  depth_both / batch_both   ... together with the hand filter's approach cone (top-down, cos >= 0.5) and aperture (2 .. 6.2 cm)
  depth_host / batch_host   the host route the clearance replaces: the call with nothing set and min_inliers = 2^30, so that its
                            handle search forms no handle (the library has no chain form without one: its pair matrix is still
                            built, which this route pays), agh_get_cloud, the contract's test on the returned hands on the host --
                            a k-d tree over the voxels (scipy, if it is there; else a bounding-box mask per hand in numpy), the
                            ball around each corridor, then the model's exact test -- and agh_find_handles on the survivors (per
                            capture for the batch).  It classifies every hand.
The variants take turns (A B C ... A B C ...) in one process on one context, --reps rounds after 3 warm-up rounds; the settings are
set or cleared outside the timed part.  `depth` runs twice per round (depth and depth_again): the spread between its own two
medians is the yardstick for every difference.  Medians, minima and maxima are printed as one JSON line; every sample, the
hypothesis, hand and handle counts and the clearance's counts go to --out as JSON.
--off-only: just the variants with nothing set, through nothing but calls an older build has too; with --root DIR the package of
  another checkout (the parent commit's build) is timed by this same script in the same session; --merge-parent FILE puts such a
  run's medians into --out as "parent_off_leg".
--trace N: just N single calls with the default corridor, the workload of a kernel trace taken in a run of its own
  (rocprofv3 --kernel-trace --stats -d DIR -- python scripts/localize_clearance_bench.py --trace 20); --kernels FILE merges
  the k_hand_clearance, k_hog_svm and k_compact_kept rows of scripts/rocpd_summary.py's CSV for that run into --out."""
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
        if any(k in r["kernel"] for k in ("k_hand_clearance", "k_hand_filter", "k_hog_svm", "k_compact_kept")):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_clearance_bench.json"))
    ap.add_argument("--root", default=ROOT, help="the checkout whose agile_grasp_amd is timed (default: this one)")
    ap.add_argument("--off-only", action="store_true", help="only the variants with nothing set (an older build has no clearance)")
    ap.add_argument("--trace", type=int, default=0, help="N: just N single calls with the default corridor")
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
    sys.path.insert(0, ROOT)  # (tests.depth_captures and the model are this checkout's, whichever package is timed)
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
    # mode -> (clearance, hand filter)
    modes = {"off": (None, None), "on": ({}, None), "both": ({}, ca)}
    counts = {}

    if not a.off_only:
        from tests import hand_clearance_cases as HC

        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        cp = HC.params()
        mid = 0.5 * (cp["near_offset"] + cp["far_offset"])
        reach = float(np.sqrt((0.5 * (cp["far_offset"] - cp["near_offset"])) ** 2 + cp["half_width"] ** 2 + cp["half_height"] ** 2)) * 1.0001

        def host_clear(hands, sample_points, vox):
            """the hands with an empty corridor: the model's exact test on the candidates a ball around the corridor holds"""
            if len(hands) == 0:
                return hands
            palms = HC.palm_points(hands, sample_points)
            centres = palms - mid * hands["approach"].astype(np.float64)
            v64 = vox.astype(np.float64)
            if cKDTree is not None:
                cand = cKDTree(v64).query_ball_point(centres, reach)
            else:
                cand = [np.flatnonzero((np.abs(v64 - c) <= reach).all(1)) for c in centres]
            keep = np.ones(len(hands), bool)
            for i, idx in enumerate(cand):
                if len(idx):
                    xb, yb, zb = HC.body_coords(hands[i:i + 1], palms[i:i + 1], vox[np.asarray(idx)])
                    keep[i] = int(HC.in_corridor(xb, yb, zb, cp).sum()) <= cp["max_points"]
            return hands[keep]

    def variant(mode, fn, host=False):
        def run():
            if not a.off_only:
                clearance, hand_filter = modes[mode]
                if clearance is None:
                    ctx.clear_hand_clearance()
                else:
                    ctx.set_hand_clearance(**clearance)
                if hand_filter is None:
                    ctx.clear_hand_filter()
                else:
                    ctx.set_hand_filter(**hand_filter)
            t0 = time.perf_counter()
            r = fn()
            if host:
                vox, _ = ctx.cloud()
                first = 0
                for q in (r if isinstance(r, list) else [r]):
                    mine = vox[first:first + q["n_voxels"]]
                    first += q["n_voxels"]
                    q["hands"] = host_clear(q["hands"], mine[q["samples"][q["hands"]["sample"]]], mine)
                    q["handles"], q["inlier_idx"] = ctx.find_handles(q["hands"], 3, 0.005)
            dt = time.perf_counter() - t0
            if not a.off_only and modes[mode][0] is not None:
                counts["last"] = ctx.hand_clearance_counts()
            return r, dt
        return run

    single = lambda: ctx.localize_depth(images, ws, **kw)
    batch = lambda: ctx.localize_depth_batch(caps, [ws] * 8, **bkw)
    single_no_handles = lambda: ctx.localize_depth(images, ws, **dict(kw, min_inliers=1 << 30))
    batch_no_handles = lambda: ctx.localize_depth_batch(caps, [ws] * 8, **dict(bkw, min_inliers=1 << 30))
    if a.trace:
        run = variant("on", single)
        for _ in range(a.trace):
            run()
        print(json.dumps({"trace_calls": a.trace}))
        return
    variants = [("depth", variant("off", single)), ("depth_on", variant("on", single)), ("depth_both", variant("both", single)),
                ("depth_host", variant("off", single_no_handles, host=True)), ("batch", variant("off", batch)),
                ("batch_on", variant("on", batch)), ("batch_both", variant("both", batch)),
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
                if name.endswith(("_on", "_both")):
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
        out["clearance"] = cp
        out["hand_filter"] = ca
        out["host_route"] = "scipy cKDTree" if cKDTree is not None else "numpy bounding-box mask"
        names = ("n_tested", "n_dropped", "n_kept")
        out["clearance_counts"] = {k: [dict(zip(names, (int(x) for x in row))) for row in v] for k, v in counts.items() if k != "last"}
        # the device route returns what the host route returns
        assert summary(first["depth_on"]) == summary(first["depth_host"]) and summary(first["batch_on"]) == summary(first["batch_host"])
    if os.path.exists(a.out):  # (a kernel trace or a parent leg merged earlier stays)
        old = json.load(open(a.out))
        for key in ("kernel_trace", "parent_off_leg"):
            if key in old:
                out[key] = old[key]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
