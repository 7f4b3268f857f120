"""agh_localize_labeled on ONE capture of the bench's raw kind (synthetic.make_raw_cloud, 700 000 points, two cameras) with K
labelled regions -- the cells of a grid over the workspace's x / y extent -- and S = 250 samples per object, classifier on.
Per K in --objects, from host memory and from device memory, ms per call (the median of --reps calls after 3 warm-up rounds, the
variants taking turns in one process):
  labeled     (a) agh_localize_labeled: one upload, preprocessing, grid and search, K handle searches side by side
  masked_x_k  (b) K agh_localize_masked calls one after the other, mask = labels == j + 1: the route the labelled call replaces
  explicit    (c) agh_localize with the K lists concatenated as explicit sample_idx: the floor, one handle search over all hands
              (null where that one list exceeds the handle search's 8192 hands)
The claim to record is labeled / masked_x_k per K.  Every sample is written to --out as JSON, the medians are printed as one
JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {2: (2, 1), 8: (4, 2), 32: (8, 4)}


def region_labels(xyz, ws, K):
    """label 1 + the cell of a kx x ky grid over the workspace's x / y extent; 0 outside the workspace and for non-finite points"""
    kx, ky = GRIDS[K]
    with np.errstate(invalid="ignore"):
        inside = ((xyz[:, 0] >= ws[0]) & (xyz[:, 0] <= ws[1]) & (xyz[:, 1] >= ws[2]) & (xyz[:, 1] <= ws[3]) & (xyz[:, 2] >= ws[4])
                  & (xyz[:, 2] <= ws[5]))
    p = np.nan_to_num(xyz[:, :2].astype(np.float64))
    ix = np.clip(((p[:, 0] - ws[0]) / (ws[1] - ws[0]) * kx).astype(np.int64), 0, kx - 1)
    iy = np.clip(((p[:, 1] - ws[2]) / (ws[3] - ws[2]) * ky).astype(np.int64), 0, ky - 1)
    return np.where(inside, 1 + iy * kx + ix, 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--objects", type=int, nargs="+", default=[2, 8, 32])
    ap.add_argument("--samples", type=int, default=250)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_label_bench.json"))
    a = ap.parse_args()
    import torch

    raw = synthetic.make_raw_cloud(700_000, 21)
    ws, S = raw.workspace, a.samples
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(raw.cam_origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    kw = dict(classify=True, min_inliers=3, min_length=0.005)
    d_xyz = torch.from_numpy(raw.xyz).cuda()
    out = {"capture": "synthetic.make_raw_cloud(700000, 21), regions: grid cells over the workspace's x / y extent",
           "n_points": int(len(raw.xyz)), "n_samples_per_object": S, "reps": a.reps, "runs": []}
    for K in a.objects:
        labels = region_labels(raw.xyz, ws, K)
        masks = [(labels == j + 1).astype(np.uint8) for j in range(K)]
        d_labels = torch.from_numpy(labels).cuda()
        d_masks = [torch.from_numpy(m).cuda() for m in masks]
        first = ctx.localize_labeled(raw.xyz, raw.size_left, ws, labels, K, n_samples=S, sample_seed=7, **kw)
        counts = [int(m) for m in ctx.label_counts()]
        explicit = np.concatenate([r["samples"] for r in first])
        info = {"n_objects": K, "n_voxels": first[0]["n_voxels"], "n_eligible": counts,
                "hypotheses": [r["n_hypotheses"] for r in first], "hands": [len(r["hands"]) for r in first],
                "handles": [len(r["handles"]) for r in first]}

        def labeled(xyz, lab):
            return lambda: ctx.localize_labeled(xyz, raw.size_left, ws, lab, K, n_samples=S, sample_seed=7, **kw)

        def masked_x_k(xyz, ms):
            return lambda: [ctx.localize_masked(xyz, raw.size_left, ws, m, n_samples=S, sample_seed=7, **kw) for m in ms]

        def floor(xyz):
            return lambda: ctx.localize(xyz, raw.size_left, ws, samples=explicit, **kw)

        variants = [("labeled_host", labeled(raw.xyz, labels)), ("masked_x_k_host", masked_x_k(raw.xyz, masks)),
                    ("explicit_host", floor(raw.xyz)), ("labeled_device", labeled(d_xyz, d_labels)),
                    ("masked_x_k_device", masked_x_k(d_xyz, d_masks)), ("explicit_device", floor(d_xyz))]
        # the three routes search the same samples: per object the same hypotheses, and the floor their sum
        twins = masked_x_k(raw.xyz, masks)()
        assert [t["n_hypotheses"] for t in twins] == info["hypotheses"] and [len(t["hands"]) for t in twins] == info["hands"]
        try:
            assert floor(raw.xyz)()["n_hypotheses"] == sum(info["hypotheses"])
        except binding.AghError as e:  # (more than 8192 hands in ONE list)
            info["explicit_error"] = str(e)
            variants = [v for v in variants if not v[0].startswith("explicit")]
        samples = {name: [] for name, _ in variants}
        for rep in range(-3, a.reps):
            for name, fn in variants:
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if rep >= 0:
                    samples[name].append(round(dt * 1e3, 4))
        med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
        run = dict(info, median_ms=med, min_max_ms={name: [min(t), max(t)] for name, t in samples.items()},
                   ratio_labeled_to_masked={w: round(med["labeled_" + w] / med["masked_x_k_" + w], 4) for w in ("host", "device")},
                   samples_ms=samples)
        out["runs"].append(run)
        print(json.dumps({k: v for k, v in run.items() if k != "samples_ms"}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
