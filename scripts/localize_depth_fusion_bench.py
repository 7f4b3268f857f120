"""Depth fusion (agh_fuse_depth) at a cell's shape: two cameras, 640 x 480 uint16, a burst of 8 frames each -- the two views of
the raw-cloud scene (tests/depth_captures.render_depth, the depth bench's) under the noise model of
tests/depth_fusion_cases.burst.  Per call, ms, each the median of --reps calls with its min and max, one process, one context:
  fuse_device        agh_fuse_depth_device, one camera's burst (frames in device memory, read in place); timed to the
                     synchronisation behind it
  fuse_host          agh_fuse_depth, one camera's burst from pageable host memory, likewise
  localize_fused     agh_localize_depth_device on the fused pair (the two slots' records)
  localize_frame0    the same call on frame 0 of each burst, in device memory
  fuse_and_localize  both cameras' agh_fuse_depth_device and the chain behind them, no synchronisation in between
  numpy_model        tests/depth_fusion_cases.fuse for one camera's burst: the host route the call replaces
The variants take turns in every round, after 3 warm-up rounds.  The fused image and its counts are checked against the numpy
model, and the hypotheses, hands and handles of both localize variants are recorded.  Everything goes to --out as JSON; the
medians are printed as one JSON line.
--trace N: just N agh_fuse_depth_device calls per camera, the workload of a kernel trace taken in a run of its own
  (rocprofv3 --kernel-trace --stats -d DIR -- python scripts/localize_depth_fusion_bench.py --trace 20); --kernels FILE merges the
  k_depth_fuse row of scripts/rocpd_summary.py's CSV for that run into --out, with the bytes the kernel moves (8 frames in, one
  image out) over its average time as a fraction of the 8 TB/s HBM peak: reported, not gated."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding, synthetic
from tests import depth_captures as D
from tests import depth_fusion_cases as FU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, T = 640, 480, 8
HBM_PEAK = 8.0e12  # bytes per second, the MI355X's specified peak
FP = dict(min_valid=3)


def merge_kernels(path, out_path):
    rows = {}
    for r in csv.DictReader(line for line in open(path) if not line.startswith("#")):
        if "k_depth_fuse" in r["kernel"]:
            rows[r["kernel"].replace(".kd", "")] = {"calls": int(r["calls"]), "avg_us": float(r["avg_us"]), "min_us": float(r["min_us"]),
                                                    "max_us": float(r["max_us"])}
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out["kernel_trace"] = rows
    if "k_depth_fuse" in rows:
        moved = (T + 1) * W * H * 2
        rate = moved / (rows["k_depth_fuse"]["avg_us"] * 1e-6)
        out["kernel_trace"]["bytes_moved"] = moved
        out["kernel_trace"]["bytes_per_second"] = round(rate)
        out["kernel_trace"]["fraction_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_depth_fusion_bench.json"))
    ap.add_argument("--trace", type=int, default=0, help="N: just N device-form fuses per camera (a kernel trace's workload)")
    ap.add_argument("--kernels", default=None, help="a scripts/rocpd_summary.py CSV of a --trace run: merge its k_depth_fuse row into --out")
    a = ap.parse_args()
    if a.kernels:
        return merge_kernels(a.kernels, a.out)
    import torch

    raw = synthetic.make_raw_cloud(1_500_000, 21, nan_frac=0.0)
    views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
    clean = [D.render_depth(views[k], k, W, H, D.U16, 520.0) for k in range(2)]
    bursts = [FU.burst(im, T, seed=41 + k) for k, im in enumerate(clean)]
    ws = raw.workspace
    origins = np.stack([im["pose"][:, 3] for im in clean])
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    dev = [[dict(f, data=torch.from_numpy(np.ascontiguousarray(f["data"]).view(np.int16)).cuda()) for f in b["frames"]] for b in bursts]
    kw = dict(n_samples=2000, sample_seed=7, classify=True, min_inliers=3, min_length=0.005)

    if a.trace:
        for _ in range(a.trace):
            for k in range(2):
                ctx.fuse_depth(dev[k], slot=k, **FP)
        ctx.synchronize()
        print(json.dumps({"trace_calls_per_camera": a.trace}))
        return

    # the fused images and their counts are the model's
    models = [FU.fuse([f["data"] for f in b["frames"]], **FP) for b in bursts]
    fused = [ctx.fuse_depth(dev[k], slot=k, **FP) for k in range(2)]
    for k in range(2):
        assert FU.same_image(ctx.fused_depth(k), models[k]["image"]), k
        c = ctx.depth_fusion_counts(k)
        assert [getattr(c, n) for n in FU.COUNT_FIELDS] == models[k]["counts"], k
    frame0 = [dev[k][0] for k in range(2)]

    def timed(fn, sync=False):
        def run():
            t0 = time.perf_counter()
            r = fn()
            if sync:
                ctx.synchronize()
            return r, time.perf_counter() - t0
        return run

    def both():
        pair = [ctx.fuse_depth(dev[k], slot=k, **FP) for k in range(2)]
        return ctx.localize_depth(pair, ws, **kw)

    variants = [("fuse_device", timed(lambda: ctx.fuse_depth(dev[0], slot=0, **FP), sync=True)),
                ("fuse_host", timed(lambda: ctx.fuse_depth(bursts[0]["frames"], slot=2, **FP), sync=True)),
                ("localize_fused", timed(lambda: ctx.localize_depth(fused, ws, **kw))),
                ("localize_frame0", timed(lambda: ctx.localize_depth(frame0, ws, **kw))),
                ("fuse_and_localize", timed(both)),
                ("numpy_model", timed(lambda: FU.fuse([f["data"] for f in bursts[0]["frames"]], **FP)))]
    samples = {name: [] for name, _ in variants}
    first = {}
    for rep in range(-3, a.reps):
        for name, fn in variants:
            r, dt = fn()
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
            first.setdefault(name, r)
    assert FU.same_image(ctx.fused_depth(2), models[0]["image"])  # (the host form's slot)

    def summary(r):
        return {"n_voxels": int(r["n_voxels"]), "n_hypotheses": int(r["n_hypotheses"]), "n_hands": len(r["hands"]), "n_handles": len(r["handles"])}

    def stats(t):
        return {"median": round(float(np.median(t)), 4), "min": round(float(min(t)), 4), "max": round(float(max(t)), 4)}

    seen = [b["clean"] > 0 for b in bursts]
    out = {"capture": "2 cameras x 8 frames of 640x480 uint16, f = 520 px", "fusion": dict(FU.DEFAULTS, **FP),
           "burst": "noise 2 raw units, 10 % drop-outs, 0.5 % weak pixels, 15 % edge flips, 10 % flying edge pixels",
           "counts": [dict(zip(FU.COUNT_FIELDS, m["counts"])) for m in models],
           "invalid_share_of_clean_valid": {"frame0": [round(float(((b["frames"][0]["data"] == 0) & s).sum() / s.sum()), 5) for b, s in zip(bursts, seen)],
                                            "fused": [round(float(((m["image"] == 0) & s).sum() / s.sum()), 5) for m, s in zip(models, seen)]},
           "n_samples": 2000, "localize": {"fused": summary(first["localize_fused"]), "frame0": summary(first["localize_frame0"]),
                                           "fuse_and_localize": summary(first["fuse_and_localize"])},
           "reps": a.reps, "ms": {name: stats(t) for name, t in samples.items()}, "samples_ms": samples}
    if os.path.exists(a.out):  # (a kernel trace merged earlier stays)
        old = json.load(open(a.out))
        if "kernel_trace" in old:
            out["kernel_trace"] = old["kernel_trace"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
