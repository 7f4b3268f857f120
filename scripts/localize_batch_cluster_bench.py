"""agh_localize_depth_batch_clustered on a BATCH of 8 captures: two 640 x 480 uint16 depth images each
(tests/depth_captures.render_depth, f = 520 px) of the six-box table of scripts/localize_cluster_bench.py -- capture k sees its
own 90 % of the scene's points, drawn with seed k --, the table plane known, K = 8 lists and S = 300 samples per object per
capture, classifier on.  ms per call (the median of --reps calls after 3 warm-up rounds, the routes taking turns in one process):
  batch       agh_localize_depth_batch_clustered: one chain, one cluster stage for all captures, one synchronisation
  single      (a) agh_localize_depth_clustered eight times, one after the other: the route the batch replaces
  labeled     (b) agh_localize_depth_batch_labeled fed the label images that agh_get_batch_cluster_labels implies: the floor, the
              same chain without the cluster stage (the label images are made once, outside the timing)
The three routes must return the same per-list results (hypotheses, kept hands, handles, and every sample index); the script
asserts it in every round.  No threshold is set: the comparison is route (a) in the same run.  Every sample is written to --out
as JSON, the medians are printed as one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding
from scripts.localize_cluster_bench import box_scene, raw_labels
from tests import depth_captures as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, K, CAPTURES = 300, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_batch_cluster_bench.json"))
    ap.add_argument("--only", default="", help="ROUTE:N -- just N calls of one route (a kernel trace's workload), nothing written")
    a = ap.parse_args()

    xyz, plane = box_scene()
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
    cp = binding.cluster_params(plane=plane, min_height=0.01, max_height=0.5, tolerance=0.01, min_voxels=50, max_objects=K)
    seeds = [7 + k for k in range(CAPTURES)]
    kw = dict(classify=True, min_inliers=3, min_length=0.005, n_samples=S)

    def batch():
        return ctx.localize_depth_batch_clustered(captures, wss, [cp] * CAPTURES, sample_seeds=seeds, **kw)

    def single():
        return [ctx.localize_depth_clustered(captures[k], ws, cp, sample_seed=seeds[k], **kw) for k in range(CAPTURES)]

    first = batch()
    info, vox_labels = ctx.batch_cluster_info(), ctx.batch_cluster_labels()
    off = np.concatenate([[0], np.cumsum([objs[0]["n_voxels"] for objs in first])])
    label_images = []
    for k, images in enumerate(captures):
        n0 = images[0]["data"].size
        packed = raw_labels(pts[k], D.image_index(images), ws, vox_labels[off[k]:off[k + 1]])
        label_images.append([packed[:n0].reshape(images[0]["data"].shape), packed[n0:].reshape(images[1]["data"].shape)])

    def labeled():
        return ctx.localize_depth_batch_labeled(captures, label_images, wss, [K] * CAPTURES, sample_seeds=seeds, **kw)

    routes = [("batch", batch), ("single", single), ("labeled", labeled)]
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
           "n_samples_per_object": S, "max_objects_per_capture": K, "lists": K * CAPTURES, "reps": a.reps,
           "n_voxels": [objs[0]["n_voxels"] for objs in first], "n_foreground": info["n_foreground"].tolist(),
           "n_components": info["n_components"].tolist(), "n_objects": info["n_objects"].tolist(),
           "object_voxels": info["n_voxels"].tolist(), "hypotheses": [w[0] for w in want], "hands": [w[1] for w in want],
           "handles": [w[2] for w in want], "median_ms": med,
           "min_max_ms": {name: [min(t), max(t)] for name, t in samples.items()},
           "single_over_batch": round(med["single"] / med["batch"], 4),
           "batch_minus_labeled_ms": round(med["batch"] - med["labeled"], 4), "samples_ms": samples}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
