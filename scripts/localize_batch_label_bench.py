"""agh_localize_depth_batch_labeled on a batch of 8 captures: each two 640 x 480 uint16 depth images of a raw-cloud scene
(tests/depth_captures.render_depth; capture k's readings 4 k mm further away), image 0 tiled 2 x 3 into 6 objects (image 1's
labels NULL): 48 lists, 300 samples per object, classifier on.  Per call (8 captures), ms:
  batch_labeled          (a) agh_localize_depth_batch_labeled from the host images and the host label images
  batch_labeled_device   (b) agh_localize_depth_batch_labeled_device: images and label images in device memory
  singles                (c) 8 x agh_localize_depth_labeled, one after the other: the route the batch call replaces
  batch_explicit         (d) agh_localize_depth_batch with, per capture, the concatenated lists (a) reported as explicit
                             sample_idx: the floor (no label stage, one list per capture in the tail)
The routes take turns in one process, --reps rounds after 3 warm-up rounds.  (a), (b) and (c) must give equal hypothesis and
kept-hand counts per list, and (d) their sums per capture (asserted).  Every sample is written to --out as JSON; the medians,
min..max, (a) / (c) and (a) - (d) are printed as one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding, synthetic
from tests import depth_captures as D
from tests import label_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURES, ROWS, COLS, S = 8, 2, 3, 300
K = ROWS * COLS


def shifted(images, k):
    """another capture of the same layout: every reading 4 k mm further away"""
    return [dict(im, data=np.where(im["data"] > 0, im["data"] + 4 * k, 0).astype(np.uint16)) for im in images]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_batch_label_bench.json"))
    a = ap.parse_args()
    import torch

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    images = [D.render_depth(views[k], k, 640, 480, D.U16, 520.0) for k in range(2)]
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in images])
    caps = [shifted(images, k) for k in range(CAPTURES)]
    tiles = L.tiled_labels(images[0]["data"].shape, ROWS, COLS)
    labels = [[tiles, None] for _ in caps]
    n_objects = [K] * CAPTURES
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    seeds = [7 + k for k in range(CAPTURES)]
    kw = dict(classify=True, min_inliers=3, min_length=0.005)
    dev_caps = [[dict(im, data=torch.from_numpy(np.ascontiguousarray(im["data"]).view(np.int16)).cuda()) for im in c] for c in caps]
    dev_labels = [[torch.from_numpy(tiles).cuda(), None] for _ in caps]
    first = ctx.localize_depth_batch_labeled(caps, labels, ws, n_objects, n_samples=S, sample_seeds=seeds, **kw)
    n_eligible = ctx.batch_label_counts().tolist()
    lists = [np.concatenate([r["samples"] for r in objs]) for objs in first]

    def counts(res):
        return [[(r["n_hypotheses"], len(r["hands"])) for r in objs] for objs in res]

    def sums(per_list):
        return [(sum(c[0] for c in objs), sum(c[1] for c in objs)) for objs in per_list]

    want = counts(first)
    routes = [
        ("batch_labeled", lambda: counts(ctx.localize_depth_batch_labeled(caps, labels, ws, n_objects, n_samples=S, sample_seeds=seeds, **kw)),
         want),
        ("batch_labeled_device", lambda: counts(ctx.localize_depth_batch_labeled(dev_caps, dev_labels, ws, n_objects, n_samples=S,
                                                                                 sample_seeds=seeds, **kw)), want),
        ("singles", lambda: counts([ctx.localize_depth_labeled(caps[k], labels[k], ws, K, n_samples=S, sample_seed=seeds[k], **kw)
                                    for k in range(CAPTURES)]), want),
        ("batch_explicit", lambda: [(r["n_hypotheses"], len(r["hands"])) for r in ctx.localize_depth_batch(caps, ws, samples=lists, **kw)],
         sums(want)),
    ]
    samples = {name: [] for name, _, _ in routes}
    for rep in range(-3, a.reps):
        for name, fn, expect in routes:
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            assert res == expect, name  # equal hypothesis and kept-hand counts per list (the floor: per capture)
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
    spread = {name: [min(t), max(t)] for name, t in samples.items()}
    out = {"batch": f"{CAPTURES} captures of 2 x 640x480 uint16, f = 520 px, image 0 tiled {ROWS} x {COLS} into {K} objects",
           "n_lists": CAPTURES * K, "n_samples_per_object": S, "reps": a.reps, "n_voxels": [objs[0]["n_voxels"] for objs in first],
           "n_eligible": n_eligible, "hypotheses": [[c[0] for c in objs] for objs in want], "hands": [[c[1] for c in objs] for objs in want],
           "median_ms": med, "min_max_ms": spread, "batch_over_singles": round(med["batch_labeled"] / med["singles"], 4),
           "batch_minus_explicit_ms": round(med["batch_labeled"] - med["batch_explicit"], 4),
           "per_capture_ms": {name: round(v / CAPTURES, 4) for name, v in med.items()}, "samples_ms": samples}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
