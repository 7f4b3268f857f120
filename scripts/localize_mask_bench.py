"""agh_localize_depth_masked on ONE capture: two 640 x 480 uint16 depth images of the raw-cloud scene
(tests/depth_captures.render_depth), a rectangular object mask on image 0 (image 1's mask NULL), 2000 samples, classifier on.
Per call, ms:
  masked            agh_localize_depth_masked from the host images and the host mask
  masked_device     agh_localize_depth_masked_device: images and mask in device memory
  explicit          agh_localize_depth with the explicit list the mask produced: the floor (that path has no mask stage)
  route             what the mask replaces: agh_preprocess + agh_get_cloud + matching the masked points' voxels on the host +
                    agh_localize with the explicit list (two preprocessings, a read-back of the cloud)
  depth, points     agh_localize_depth and agh_localize (back-projected packed host points) UNMASKED, drawn samples: the same
                    kernels before and after this feature -- run with --unmasked-only on both commits and compare
  depth_again       `depth` a second time per round: the spread between its own two medians is the yardstick
The variants take turns in one process, --reps rounds after 3 warm-up rounds.  Every sample is written to --out as JSON, the
medians are printed as one JSON line.  The cost of the mask stage is masked (or masked_device) minus explicit."""
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
CELL = 0.003


def host_match(ctx, pts, cams, packed, ws):
    """The route's host side: the voxelised cloud read back, the masked kept points' voxels computed as the voxeliser does and
    looked up in it; returns the ascending indices of the voxels found."""
    vox, vcam = ctx.cloud()
    with np.errstate(invalid="ignore"):
        kept = ((pts[:, 0] >= ws[0]) & (pts[:, 0] <= ws[1]) & (pts[:, 1] >= ws[2]) & (pts[:, 1] <= ws[3]) & (pts[:, 2] >= ws[4])
                & (pts[:, 2] <= ws[5]))
    found = []
    base = 0
    for c in (0, 1):
        sel = kept & (cams == c)
        n_c = int((vcam == c).sum())
        if sel.any():
            mn = pts[sel].min(0).astype(np.float64)
            q = pts[sel & (packed != 0)].astype(np.float64)
            key = (np.floor((q - mn) / CELL) * CELL + 1.0 * mn).astype(np.float32)
            rows = np.ascontiguousarray(vox[base:base + n_c]).view([("", np.float32)] * 3).reshape(-1)
            want = np.unique(np.ascontiguousarray(key).view([("", np.float32)] * 3).reshape(-1))
            found.append(base + np.flatnonzero(np.isin(rows, want)))
        base += n_c
    return np.concatenate(found).astype(np.int32) if found else np.zeros(0, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--unmasked-only", action="store_true", help="only the unmasked calls (runs on a commit without the feature)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_mask_bench.json"))
    a = ap.parse_args()
    import torch

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    images = [D.render_depth(views[k], k, 640, 480, D.U16, 520.0) for k in range(2)]
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in images])
    pts = D.deproject_ref(images)
    cams = D.image_index(images)
    size_left = images[0]["data"].size
    m0 = np.zeros(images[0]["data"].shape, np.uint8)
    m0[160:320, 240:400] = 1
    masks = [m0, None]
    packed = np.concatenate([m0.reshape(-1), np.zeros(images[1]["data"].size, np.uint8)])
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    S = 2000
    kw = dict(classify=True, min_inliers=3, min_length=0.005)

    def timed(fn):
        def run():
            t0 = time.perf_counter()
            r = fn()
            return r, time.perf_counter() - t0
        return run

    variants = [("depth", timed(lambda: ctx.localize_depth(images, ws, n_samples=S, sample_seed=7, **kw))),
                ("points", timed(lambda: ctx.localize(pts, size_left, ws, n_samples=S, sample_seed=7, dense=True, **kw)))]
    info = {}
    if not a.unmasked_only:
        dev_images = [dict(im, data=torch.from_numpy(np.ascontiguousarray(im["data"]).view(np.int16)).cuda()) for im in images]
        dev_masks = [torch.from_numpy(m0).cuda(), None]
        first = ctx.localize_depth_masked(images, masks, ws, n_samples=S, sample_seed=7, **kw)
        explicit = first["samples"]
        info = {"n_eligible": ctx.sample_mask_count(), "masked_hypotheses": first["n_hypotheses"], "masked_hands": len(first["hands"]),
                "masked_handles": len(first["handles"])}

        def route():
            ctx.preprocess(pts, size_left, ws, CELL, dense=True)
            E = host_match(ctx, pts, cams, packed, ws)
            return ctx.localize(pts, size_left, ws, samples=binding.masked_samples(E, S, 7), dense=True, **kw)

        r = route()
        assert np.array_equal(r["samples"], explicit) and r["n_hypotheses"] == first["n_hypotheses"]  # the same list, the same search
        variants += [("masked", timed(lambda: ctx.localize_depth_masked(images, masks, ws, n_samples=S, sample_seed=7, **kw))),
                     ("masked_device", timed(lambda: ctx.localize_depth_masked(dev_images, dev_masks, ws, n_samples=S, sample_seed=7, **kw))),
                     ("explicit", timed(lambda: ctx.localize_depth(images, ws, samples=explicit, **kw))),
                     ("route", timed(route))]
    variants.append(("depth_again", variants[0][1]))
    samples = {name: [] for name, _ in variants}
    firsts = {}
    for rep in range(-3, a.reps):
        for name, fn in variants:
            r, dt = fn()
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
            firsts.setdefault(name, r)
    for name in ("masked", "masked_device", "explicit", "route"):
        if name in firsts:
            assert firsts[name]["n_hypotheses"] == info["masked_hypotheses"] and len(firsts[name]["hands"]) == info["masked_hands"], name
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
    spread = {name: [min(t), max(t)] for name, t in samples.items()}
    out = dict({"capture": "2 x 640x480 uint16, f = 520 px, mask rows 160:320 x columns 240:400 of image 0", "n_points": int(len(pts)),
                "n_voxels": firsts["depth"]["n_voxels"], "n_samples": S, "reps": a.reps, "median_ms": med, "min_max_ms": spread,
                "samples_ms": samples}, **info)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
