"""agh_localize_depth against the points calls on ONE capture: two 640 x 480 uint16 depth images of the raw-cloud scene
(tests/depth_captures.render_depth), 2000 drawn samples, classifier on.  Per call, ms:
  points12          agh_localize from the back-projected host points, packed (12 bytes per point, 7.4 MB)
  points32          the same points in 32-byte rows (pcl::PointXYZRGBA: 19.7 MB)
  depth             agh_localize_depth from the two host images (1.2 MB)
  device            agh_localize_device on the points in device memory: the floor, no upload at all
  points12_staged   agh_localize_begin / _stage / _end, per capture of a stream
  depth_staged      agh_localize_depth_begin / _stage / agh_localize_end, per capture of a stream
The variants take turns (A B C ... A B C ...) in one process, --reps rounds after 3 warm-up rounds; points12 runs twice per round
(points12 and points12_again): the spread between its own two medians is the yardstick for every difference.  Every sample is
written to --out as JSON, the medians are printed as one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_depth_bench.json"))
    a = ap.parse_args()
    import torch

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    images = [D.render_depth(views[k], k, 640, 480, D.U16, 520.0) for k in range(2)]
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in images])
    pts12 = D.deproject_ref(images)
    size_left = images[0]["data"].size
    pts32 = np.zeros((len(pts12), 8), np.float32)
    pts32[:, :3] = pts12
    dev = torch.from_numpy(pts12).cuda()
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    kw = dict(n_samples=2000, sample_seed=7, classify=True, min_inliers=3, min_length=0.005)
    pkw = dict(kw, dense=True)
    # a stream takes two capture objects in turns, the next one staged under this one's kernels
    pts_pair = [pts12, pts12.copy()]
    img_pair = [images, [dict(im, data=im["data"].copy()) for im in images]]
    state = {"points": 0, "depth": 0, "chain": None}

    def drain():
        if state["chain"] is not None:
            ctx.localize_end()
            state["chain"] = None

    def blocking(fn):
        def run():
            drain()  # (a stream variant's chain in flight is collected outside the timed part)
            t0 = time.perf_counter()
            r = fn()
            return r, time.perf_counter() - t0
        return run

    def staged(kind):
        def run():
            if state["chain"] != kind:  # (the other kind's chain, or none: begin this kind's outside the timed part)
                drain()
                if kind == "points":
                    ctx.localize_begin(pts_pair[state[kind] & 1], size_left, ws, **pkw)
                else:
                    ctx.localize_depth_begin(img_pair[state[kind] & 1], ws, **kw)
                state["chain"] = kind
            t0 = time.perf_counter()
            nxt = (state[kind] + 1) & 1
            if kind == "points":
                ctx.localize_stage(pts_pair[nxt])
                r = ctx.localize_end()
                ctx.localize_begin(pts_pair[nxt], size_left, ws, **pkw)
            else:
                ctx.localize_depth_stage(img_pair[nxt])
                r = ctx.localize_end()
                ctx.localize_depth_begin(img_pair[nxt], ws, **kw)
            state[kind] += 1
            return r, time.perf_counter() - t0
        return run

    variants = [
        ("points12", blocking(lambda: ctx.localize(pts12, size_left, ws, **pkw))),
        ("points32", blocking(lambda: ctx.localize(pts32, size_left, ws, **pkw))),
        ("depth", blocking(lambda: ctx.localize_depth(images, ws, **kw))),
        ("device", blocking(lambda: ctx.localize(dev, size_left, ws, **pkw))),
        ("points12_again", blocking(lambda: ctx.localize(pts12, size_left, ws, **pkw))),
        ("points12_staged", staged("points")),
        ("depth_staged", staged("depth")),
    ]
    samples = {name: [] for name, _ in variants}
    first = {}
    for rep in range(-3, a.reps):
        for name, fn in variants:
            r, dt = fn()
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
            first.setdefault(name, r)
    drain()
    ref = first["points12"]
    for name, r in first.items():  # the same capture, the same results
        assert r["n_voxels"] == ref["n_voxels"] and r["n_hypotheses"] == ref["n_hypotheses"], name
        assert len(r["hands"]) == len(ref["hands"]) and np.array_equal(r["inlier_idx"], ref["inlier_idx"]), name
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
    out = {"capture": "2 x 640x480 uint16, f = 520 px", "n_points": int(len(pts12)),
           "invalid_fraction": round(float(np.mean([(im["data"] == 0).mean() for im in images])), 4),
           "bytes": {"depth": int(sum(im["data"].nbytes for im in images)), "points12": int(pts12.nbytes), "points32": int(pts32.nbytes)},
           "n_voxels": ref["n_voxels"], "n_samples": 2000, "n_hypotheses": ref["n_hypotheses"], "n_hands": len(ref["hands"]),
           "n_handles": len(ref["handles"]), "reps": a.reps, "median_ms": med, "samples_ms": samples}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
