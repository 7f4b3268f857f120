"""The voxel filter (agh_set_voxel_filter) on and off, on the same build: the 700k-point raw capture (synthetic.make_raw_cloud(700_000,
5)) with about 0.5 % stray points injected -- uniform in the box of each camera's kept points, appended to that camera's stretch
-- 2000 drawn samples, classifier on.  Per call, ms:
  single            agh_localize, no filter
  single_filtered   the same call with the default filter set (radius 2 voxels, 4 neighbours)
  batch             agh_localize_batch over eight such captures (seeds 5 .. 12), no filter
  batch_filtered    the same call with the filter set
The variants take turns (A B C D A B C D ...) in one process on one context, --reps rounds after 3 warm-up rounds; the filter is
set or cleared outside the timed part.  `single` runs twice per round (single and single_again): the spread between its own two
medians is the yardstick for every difference.  Medians, minima and maxima are printed as one JSON line; every sample and the
hypothesis counts of the same drawn-sample seed in both modes go to --out as JSON.
--off-only: just the unfiltered variants, through nothing but calls an older build has too; with --root DIR the package of
  another checkout (the parent commit's build) is timed by this same script in the same session.
--trace N: just N single calls without and N with the filter, the workload of a kernel trace taken in a run of its own
  (rocprofv3 --kernel-trace --stats -d DIR -- python scripts/localize_voxel_filter_bench.py --trace 20); --kernels FILE merges
  the k_vox_* rows of scripts/rocpd_summary.py's CSV for that run into --out (k_vox_prune against k_vox_popcount + k_vox_emit of
  the same trace, which make the same passes over the same bitmap: reported, not gated)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inject(np, rc, frac, seed):
    rng = np.random.default_rng(seed)
    ws = rc.workspace
    parts, n_each = [], int(round(frac * len(rc.xyz) / 2))
    for lo, hi in ((0, rc.size_left), (rc.size_left, len(rc.xyz))):
        p = rc.xyz[lo:hi]
        with np.errstate(invalid="ignore"):
            ok = ((p[:, 0] >= ws[0]) & (p[:, 0] <= ws[1]) & (p[:, 1] >= ws[2]) & (p[:, 1] <= ws[3]) & (p[:, 2] >= ws[4])
                  & (p[:, 2] <= ws[5]))
        parts += [p, rng.uniform(p[ok].min(0), p[ok].max(0), (n_each, 3)).astype(np.float32)]
    return np.ascontiguousarray(np.concatenate(parts)), rc.size_left + n_each, 2 * n_each


def merge_kernels(path, out_path):
    rows = {}
    for r in csv.DictReader(line for line in open(path) if not line.startswith("#")):
        if "k_vox_" in r["kernel"]:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_voxel_filter_bench.json"))
    ap.add_argument("--root", default=ROOT, help="the checkout whose agile_grasp_amd is timed (default: this one)")
    ap.add_argument("--off-only", action="store_true", help="only the unfiltered variants (an older build has no filter)")
    ap.add_argument("--trace", type=int, default=0, help="N: just N single calls without and N with the filter")
    ap.add_argument("--kernels", default=None, help="a scripts/rocpd_summary.py CSV of a --trace run: merge its k_vox_* rows into --out")
    a = ap.parse_args()
    if a.kernels:
        return merge_kernels(a.kernels, a.out)
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np

    from agile_grasp_amd import binding, synthetic

    caps = [synthetic.make_raw_cloud(700_000, 5 + k) for k in range(8)]
    injected = [inject(np, rc, 0.005, 100 + k) for k, rc in enumerate(caps)]
    xyz, size_left, n_inj = injected[0]
    ws = caps[0].workspace
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(caps[0].cam_origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    kw = dict(n_samples=2000, sample_seed=7, classify=True, min_inliers=3, min_length=0.005)
    bkw = dict(n_samples=[2000] * 8, sample_seeds=[7 + k for k in range(8)], classify=True, min_inliers=3, min_length=0.005)
    counts = {}

    def variant(filtered, fn):
        def run():
            if not a.off_only:
                if filtered:
                    ctx.set_voxel_filter()
                else:
                    ctx.clear_voxel_filter()
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            if filtered:
                counts["last"] = ctx.voxel_filter_counts()
            return r, dt
        return run

    single = lambda: ctx.localize(xyz, size_left, ws, **kw)
    batch = lambda: ctx.localize_batch([c[0] for c in injected], [c[1] for c in injected], [rc.workspace for rc in caps], **bkw)
    if a.trace:
        for filtered in (False, True):
            run = variant(filtered, single)
            for _ in range(a.trace):
                run()
        print(json.dumps({"trace_calls_each": a.trace}))
        return
    variants = [("single", variant(False, single)), ("single_filtered", variant(True, single)), ("batch", variant(False, batch)),
                ("batch_filtered", variant(True, batch)), ("single_again", variant(False, single))]
    if a.off_only:
        variants = [v for v in variants if not v[0].endswith("_filtered")]
    samples = {name: [] for name, _ in variants}
    first = {}
    for rep in range(-3, a.reps):
        for name, fn in variants:
            r, dt = fn()
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
            if name not in first:
                first[name] = r
                if name.endswith("_filtered"):
                    counts[name] = counts["last"]
    stats = {name: {"median": round(float(np.median(t)), 4), "min": min(t), "max": max(t)} for name, t in samples.items()}

    def summary(r):
        return {"n_voxels": int(r["n_voxels"]), "n_hypotheses": int(r["n_hypotheses"]), "n_hands": len(r["hands"]), "n_handles": len(r["handles"])}

    out = {"capture": "synthetic.make_raw_cloud(700_000, 5) + stray points", "n_points": int(len(xyz)), "n_injected": int(n_inj),
           "n_samples": 2000, "sample_seed": 7, "reps": a.reps, "root": os.path.relpath(os.path.abspath(a.root), ROOT),
           "single": {"unfiltered": summary(first["single"])}, "batch": {"unfiltered": [summary(r) for r in first["batch"]]},
           "ms": stats, "samples_ms": samples}
    if not a.off_only:
        fp = binding.voxel_filter_params()  # (what set_voxel_filter() without arguments sets)
        out["filter"] = {"radius": int(fp.radius), "min_neighbors": int(fp.min_neighbors)}
        out["single"]["filtered"] = summary(first["single_filtered"])
        out["batch"]["filtered"] = [summary(r) for r in first["batch_filtered"]]
        names = ("n_occupied_0", "n_occupied_1", "n_pruned_0", "n_pruned_1", "n_kept_0", "n_kept_1")
        out["filter_counts"] = {"single": dict(zip(names, (int(x) for x in counts["single_filtered"][0]))),
                                "batch": [dict(zip(names, (int(x) for x in row))) for row in counts["batch_filtered"]]}
        assert first["single"]["n_voxels"] - first["single_filtered"]["n_voxels"] == int(counts["single_filtered"][0][2:4].sum())
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
