"""The handle ranking (agh_set_handle_ranking) on and off, on the same build: two 640 x 480 uint16 depth images of the raw-cloud
scene (tests/depth_captures.render_depth), 2000 drawn samples, classifier on.  Per call, ms:
  depth / batch             agh_localize_depth / agh_localize_depth_batch over eight such captures (capture k: every reading
                            4 k mm further away), nothing set
  depth_rank / batch_rank   the same calls with the default ranking (support and margin, weight 1 each, all handles)
  depth_host / batch_host   the host route the ranking replaces: the call with nothing set, agh_get_hog for the decision sums of
                            every hypothesis (it classifies them once more), the kept hands' margins from them, and the numpy model
                            of tests/handle_ranking_cases.py on the call's hands, handles and inlier lists (per capture for the batch)
The variants take turns (A B C ... A B C ...) in one process on one context, --reps rounds after 3 warm-up rounds; the setting is
set or cleared outside the timed part.  `depth` runs twice per round (depth and depth_again): the spread between its own two
medians is the yardstick for every difference.  Medians, minima and maxima are printed as one JSON line; every sample and the
hypothesis, hand and handle counts go to --out as JSON.
--off-only: just the variants with nothing set, through nothing but calls an older build has too; with --root DIR the package of
  another checkout (the parent commit's build) is timed by this same script in the same session; --merge-parent FILE puts such a
  run's medians into --out as "parent_off_leg" (with --merge-as self_off_leg: this build's own --off-only run, taken between two of
  the parent's)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_rank_bench.json"))
    ap.add_argument("--root", default=ROOT, help="the checkout whose agile_grasp_amd is timed (default: this one)")
    ap.add_argument("--off-only", action="store_true", help="only the variants with nothing set (an older build has no ranking)")
    ap.add_argument("--merge-parent", default=None, help="the --out of an --off-only run of the parent's build: merge its medians")
    ap.add_argument("--merge-as", default="parent_off_leg", choices=("parent_off_leg", "self_off_leg"))
    a = ap.parse_args()
    if a.merge_parent:
        out = json.load(open(a.out))
        out.setdefault(a.merge_as, []).append(json.load(open(a.merge_parent))["ms"])
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
    if not a.off_only:
        from tests import handle_ranking_cases as R

    def host_rank(r):
        """the model on the call's own outputs, the margins from agh_get_hog's sums: the kept hypotheses are those with sum <= 0,
        in the order of the hands"""
        lists = r if isinstance(r, list) else [r]
        _, sums = ctx.hog()
        assert len(sums) == sum(q["n_hypotheses"] for q in lists)
        margins = -sums[sums <= 0]
        assert len(margins) == sum(len(q["hands"]) for q in lists)
        first = 0
        for q in lists:
            m = margins[first:first + len(q["hands"])]
            first += len(q["hands"])
            q["handles"], q["scores"], _ = R.rank(R.DEFAULTS, q["hands"], m, q["handles"], q["inlier_idx"])

    def variant(rank, fn, host=False):
        def run():
            if not a.off_only:
                if rank:
                    ctx.set_handle_ranking()
                else:
                    ctx.clear_handle_ranking()
            t0 = time.perf_counter()
            r = fn()
            if host:
                host_rank(r)
            dt = time.perf_counter() - t0
            if rank:
                scores, first = ctx.handle_scores(), 0
                for q in (r if isinstance(r, list) else [r]):
                    q["scores"] = scores[first:first + len(q["handles"])]
                    first += len(q["handles"])
            return r, dt
        return run

    single = lambda: ctx.localize_depth(images, ws, **kw)
    batch = lambda: ctx.localize_depth_batch(caps, [ws] * 8, **bkw)
    variants = [("depth", variant(False, single)), ("depth_rank", variant(True, single)), ("depth_host", variant(False, single, host=True)),
                ("batch", variant(False, batch)), ("batch_rank", variant(True, batch)), ("batch_host", variant(False, batch, host=True)),
                ("depth_again", variant(False, single))]
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
    stats = {name: {"median": round(float(np.median(t)), 4), "min": min(t), "max": max(t)} for name, t in samples.items()}

    def summary(r):
        if isinstance(r, list):
            return [summary(q) for q in r]
        return {"n_voxels": int(r["n_voxels"]), "n_hypotheses": int(r["n_hypotheses"]), "n_hands": len(r["hands"]), "n_handles": len(r["handles"])}

    out = {"capture": "2 x 640x480 uint16, f = 520 px", "n_samples": 2000, "sample_seed": 7, "reps": a.reps,
           "root": os.path.relpath(os.path.abspath(a.root), ROOT), "results": {name: summary(r) for name, r in first.items()},
           "ms": stats, "samples_ms": samples}
    if not a.off_only:
        out["ranking"] = {k: (list(v) if isinstance(v, tuple) else (str(v) if v == -np.inf else v)) for k, v in R.DEFAULTS.items()}
        # the device route returns what the host route returns, and it is another order than the unranked call's
        for dev, host, off in (("depth_rank", "depth_host", "depth"), ("batch_rank", "batch_host", "batch")):
            lists = lambda r: r if isinstance(r, list) else [r]
            for d, h in zip(lists(first[dev]), lists(first[host])):
                assert R.same_bytes(d["handles"], h["handles"]) and R.same_scores(d["scores"], h["scores"]), dev
            out.setdefault("reordered_lists", {})[dev] = sum(
                1 for d, o in zip(lists(first[dev]), lists(first[off])) if not R.same_bytes(d["handles"], o["handles"]))
    if os.path.exists(a.out):  # (a parent leg merged earlier stays)
        old = json.load(open(a.out))
        for key in ("parent_off_leg", "self_off_leg"):
            if key in old:
                out[key] = old[key]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
