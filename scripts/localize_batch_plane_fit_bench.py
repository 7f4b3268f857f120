"""agh_localize_depth_batch_clustered_fit on a BATCH of 8 captures: the workload of scripts/localize_batch_cluster_bench.py -- two
640 x 480 uint16 depth images per capture of the six-box table, capture k its own 90 % of the scene's points, K = 8 lists and
S = 300 samples per object per capture, classifier on -- with NO plane given: 128 candidates at 1 cm per capture, capture k's
fit seeded with 1 + k.  ms per call (the median of --reps calls after 3 warm-up rounds, the routes taking turns in one process):
  fit         agh_localize_depth_batch_clustered_fit: one chain, one fit stage and one cluster stage for all captures, one
              synchronisation
  given       (a) agh_localize_depth_batch_clustered given the planes the fit reported: the floor, the same chain without the
              fit stage
  single      (b) agh_localize_depth_clustered_fit eight times, one after the other: the route the batch replaces
The three routes must return the same per-list results (hypotheses, kept hands, handles, and every sample index), and route (b)
the same planes bit for bit; the script asserts it in every round.  No threshold is set: the comparisons are routes (a) and (b)
in the same run.  Every sample is written to --out as JSON, the medians are printed as one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding
from scripts.localize_cluster_bench import box_scene
from tests import depth_captures as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, K, CAPTURES = 300, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_batch_plane_fit_bench.json"))
    ap.add_argument("--only", default="", help="ROUTE:N -- just N calls of one route (a kernel trace's workload), nothing written")
    a = ap.parse_args()

    xyz, _plane = box_scene()
    captures = []
    for k in range(CAPTURES):
        keep = np.random.default_rng(k).random(len(xyz)) < 0.9
        captures.append([D.render_depth(xyz[keep], cam, 640, 480, D.U16, 520.0) for cam in range(2)])
    origins = np.stack([im["pose"][:, 3] for im in captures[0]])
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    pts = [ctx.deproject(images) for images in captures]
    fin = np.concatenate([p[np.isfinite(p).all(1)] for p in pts])
    ws = np.stack([fin.min(0) - 0.01, fin.max(0) + 0.01], axis=1).reshape(6).astype(np.float64)
    wss = [ws] * CAPTURES
    fields = dict(min_height=0.01, max_height=0.5, tolerance=0.01, min_voxels=50, max_objects=K)
    cp = binding.cluster_params(**fields)  # (its plane is not read by the fitted routes)
    fps = [binding.plane_fit_params(n_candidates=128, distance_threshold=0.01, seed=1 + k) for k in range(CAPTURES)]
    seeds = [7 + k for k in range(CAPTURES)]
    kw = dict(classify=True, min_inliers=3, min_length=0.005, n_samples=S)

    def fit():
        return ctx.localize_depth_batch_clustered_fit(captures, wss, fps, [cp] * CAPTURES, sample_seeds=seeds, **kw)

    first = fit()
    fits, info = ctx.batch_plane_fit(), ctx.batch_cluster_info()
    assert all(f["found"] and f["refined"] for f in fits)
    planes = [f["plane"].copy() for f in fits]
    given_cps = [binding.cluster_params(plane=tuple(p), **fields) for p in planes]

    def given():
        return ctx.localize_depth_batch_clustered(captures, wss, given_cps, sample_seeds=seeds, **kw)

    def single():
        out = []
        for k in range(CAPTURES):
            out.append(ctx.localize_depth_clustered_fit(captures[k], ws, fps[k], cp, sample_seed=seeds[k], **kw))
            assert ctx.plane_fit()["plane"].tobytes() == planes[k].tobytes(), k  # the batch's plane, bit for bit
        return out

    routes = [("fit", fit), ("given", given), ("single", single)]
    if a.only:
        name, n = a.only.split(":")
        for _ in range(int(n)):
            dict(routes)[name]()
        return

    def digest(res):
        return [(r["n_hypotheses"], len(r["hands"]), len(r["handles"]), r["samples"].tobytes()) for objs in res for r in objs]

    want = digest(first)
    samples = {name: [] for name, _ in routes}
    for rep in range(-3, a.reps):
        for name, fn in routes:
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            assert digest(res) == want, name  # the same lists, hypotheses, kept hands and handles per list on every route
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
    out = {"batch": "8 captures of 2 x 640x480 uint16, f = 520 px, a table with six boxes, 90 % of its points per capture",
           "n_candidates": 128, "distance_threshold": 0.01, "n_samples_per_object": S, "max_objects_per_capture": K,
           "lists": K * CAPTURES, "reps": a.reps, "n_voxels": [f["n_voxels"] for f in fits], "n_inliers": [f["n_inliers"] for f in fits],
           "n_refit": [f["n_refit"] for f in fits], "planes": [p.tolist() for p in planes],
           "n_foreground": info["n_foreground"].tolist(), "n_objects": info["n_objects"].tolist(),
           "hypotheses": [w[0] for w in want], "hands": [w[1] for w in want], "handles": [w[2] for w in want], "median_ms": med,
           "min_max_ms": {name: [min(t), max(t)] for name, t in samples.items()},
           "fit_minus_given_ms": round(med["fit"] - med["given"], 4), "single_over_fit": round(med["single"] / med["fit"], 4),
           "fit_per_capture_ms": round(med["fit"] / CAPTURES, 4), "samples_ms": samples}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
