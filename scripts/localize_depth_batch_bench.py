"""agh_localize_depth_batch against the other ways to serve a BATCH of depth captures: 8 captures of two 640 x 480 uint16 depth
images of the raw-cloud scene (tests/depth_captures.render_depth; capture k's readings are 4 k mm further away), 2000 drawn
samples each, classifier on.  Per call over the 8 captures, ms:
  depth_batch          (a) agh_localize_depth_batch from the sixteen host images (9.8 MB)
  points_batch         (b) agh_localize_batch from the back-projected host points, packed, 12 bytes per point (59 MB)
  points_batch_device  (c) agh_localize_batch_device on those points in device memory: the floor, no upload, no back-projection
  depth_singles        (d) agh_localize_depth, the captures one after the other
  depth_batch_device   (e) agh_localize_depth_batch_device on the images in device memory
The variants take turns (A B C ... A B C ...) in one process, --reps rounds after 3 warm-up rounds; points_batch runs twice per
round (points_batch and points_batch_again): the spread between its own two medians is the yardstick for every difference.
Every sample is written to --out as JSON, the medians are printed as one JSON line."""
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
CAPTURES = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_depth_batch_bench.json"))
    a = ap.parse_args()
    import torch

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    images = [D.render_depth(views[k], k, 640, 480, D.U16, 520.0) for k in range(2)]
    caps = [[dict(im, data=np.where(im["data"] > 0, im["data"] + 4 * k, 0).astype(np.uint16)) for im in images] for k in range(CAPTURES)]
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in images])
    pts = [D.deproject_ref(c) for c in caps]
    size_left = images[0]["data"].size
    dev_pts = [torch.from_numpy(p).cuda() for p in pts]
    dev_caps = [[dict(im, data=torch.from_numpy(im["data"].view(np.int16)).cuda()) for im in c] for c in caps]
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    seeds = [7 + k for k in range(CAPTURES)]
    kw = dict(n_samples=2000, sample_seeds=seeds, classify=True, min_inliers=3, min_length=0.005)
    pkw = dict(kw, dense=True)
    skw = dict(n_samples=2000, classify=True, min_inliers=3, min_length=0.005)

    def timed(fn):
        def run():
            t0 = time.perf_counter()
            r = fn()
            return r, time.perf_counter() - t0
        return run

    variants = [
        ("depth_batch", timed(lambda: ctx.localize_depth_batch(caps, ws, **kw))),
        ("points_batch", timed(lambda: ctx.localize_batch(pts, size_left, ws, **pkw))),
        ("points_batch_device", timed(lambda: ctx.localize_batch(dev_pts, size_left, ws, **pkw))),
        ("depth_singles", timed(lambda: [ctx.localize_depth(caps[k], ws, sample_seed=seeds[k], **skw) for k in range(CAPTURES)])),
        ("depth_batch_device", timed(lambda: ctx.localize_depth_batch(dev_caps, ws, **kw))),
        ("points_batch_again", timed(lambda: ctx.localize_batch(pts, size_left, ws, **pkw))),
    ]
    samples = {name: [] for name, _ in variants}
    first = {}
    for rep in range(-3, a.reps):
        for name, fn in variants:
            r, dt = fn()
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
            first.setdefault(name, r)
    ref = first["points_batch"]
    for name, res in first.items():  # the same captures, the same results
        for k in range(CAPTURES):
            r, w = res[k], ref[k]
            assert r["n_voxels"] == w["n_voxels"] and r["n_hypotheses"] == w["n_hypotheses"], (name, k)
            assert len(r["hands"]) == len(w["hands"]) and np.array_equal(r["inlier_idx"], w["inlier_idx"]), (name, k)
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
    out = {"batch": f"{CAPTURES} captures of 2 x 640x480 uint16, f = 520 px", "n_points": int(sum(len(p) for p in pts)),
           "invalid_fraction": round(float(np.mean([(im["data"] == 0).mean() for c in caps for im in c])), 4),
           "bytes": {"depth": int(sum(im["data"].nbytes for c in caps for im in c)), "points12": int(sum(p.nbytes for p in pts))},
           "n_voxels": [r["n_voxels"] for r in ref], "n_samples": 2000, "n_hypotheses": [r["n_hypotheses"] for r in ref],
           "n_hands": [len(r["hands"]) for r in ref], "n_handles": [len(r["handles"]) for r in ref], "reps": a.reps,
           "median_ms": med, "median_ms_per_capture": {k: round(v / CAPTURES, 4) for k, v in med.items()}, "samples_ms": samples}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
