"""agh_localize_depth_batch_masked on a batch of 8 captures: each two 640 x 480 uint16 depth images of a raw-cloud scene
(tests/depth_captures.render_depth; capture k's readings 4 k mm further away), a rectangular object mask on image 0 (image 1's mask
NULL), 2000 samples per capture, classifier on.  Per call (8 captures), ms:
  batch_masked          (a) agh_localize_depth_batch_masked from the host images and the host masks
  batch_masked_device   (b) agh_localize_depth_batch_masked_device: images and masks in device memory
  singles               (c) 8 x agh_localize_depth_masked, one after the other: the route the batch call replaces
  batch_explicit        (d) agh_localize_depth_batch with the lists (a) reported as explicit sample_idx: the floor (no mask stage)
The routes take turns in one process, --reps rounds after 3 warm-up rounds.  The four must give equal hypothesis and kept-hand
counts per capture (asserted).  Every sample is written to --out as JSON; the medians, min..max, (a) / (c) and (a) - (d) are
printed as one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding, synthetic
from tests import depth_captures as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPTURES, S = 8, 2000


def shifted(images, k):
    """another capture of the same layout: every reading 4 k mm further away"""
    return [dict(im, data=np.where(im["data"] > 0, im["data"] + 4 * k, 0).astype(np.uint16)) for im in images]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_batch_mask_bench.json"))
    a = ap.parse_args()
    import torch

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    images = [D.render_depth(views[k], k, 640, 480, D.U16, 520.0) for k in range(2)]
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in images])
    caps = [shifted(images, k) for k in range(CAPTURES)]
    m0 = np.zeros(images[0]["data"].shape, np.uint8)
    m0[160:320, 240:400] = 1
    masks = [[m0, None] for _ in caps]
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    seeds = [7 + k for k in range(CAPTURES)]
    kw = dict(classify=True, min_inliers=3, min_length=0.005)
    dev_caps = [[dict(im, data=torch.from_numpy(np.ascontiguousarray(im["data"]).view(np.int16)).cuda()) for im in c] for c in caps]
    dev_masks = [[torch.from_numpy(m0).cuda(), None] for _ in caps]
    first = ctx.localize_depth_batch_masked(caps, masks, ws, n_samples=S, sample_seeds=seeds, **kw)
    n_eligible = ctx.batch_mask_counts().tolist()
    lists = [r["samples"] for r in first]

    def counts(res):
        return [(r["n_hypotheses"], len(r["hands"])) for r in res]

    routes = [
        ("batch_masked", lambda: ctx.localize_depth_batch_masked(caps, masks, ws, n_samples=S, sample_seeds=seeds, **kw)),
        ("batch_masked_device", lambda: ctx.localize_depth_batch_masked(dev_caps, dev_masks, ws, n_samples=S, sample_seeds=seeds, **kw)),
        ("singles", lambda: [ctx.localize_depth_masked(caps[k], masks[k], ws, n_samples=S, sample_seed=seeds[k], **kw)
                             for k in range(CAPTURES)]),
        ("batch_explicit", lambda: ctx.localize_depth_batch(caps, ws, samples=lists, **kw)),
    ]
    samples = {name: [] for name, _ in routes}
    for rep in range(-3, a.reps):
        for name, fn in routes:
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            assert counts(res) == counts(first), name  # the four routes: equal hypothesis and kept-hand counts per capture
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
    spread = {name: [min(t), max(t)] for name, t in samples.items()}
    out = {"batch": f"{CAPTURES} captures of 2 x 640x480 uint16, f = 520 px, mask rows 160:320 x columns 240:400 of image 0",
           "n_samples_per_capture": S, "reps": a.reps, "n_voxels": [r["n_voxels"] for r in first], "n_eligible": n_eligible,
           "hypotheses": [c[0] for c in counts(first)], "hands": [c[1] for c in counts(first)], "median_ms": med, "min_max_ms": spread,
           "batch_over_singles": round(med["batch_masked"] / med["singles"], 4),
           "batch_minus_explicit_ms": round(med["batch_masked"] - med["batch_explicit"], 4),
           "per_capture_ms": {name: round(v / CAPTURES, 4) for name, v in med.items()}, "samples_ms": samples}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
