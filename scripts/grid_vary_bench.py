"""C2's step (agh_set_cloud_device + agh_find_hands_device, one stream) on a cloud whose point count changes with every
step: step k drops the last (k mod 8) * 1500 points, the way a stream of voxelised captures varies.  Prints one JSON line:
ms per step (median, min and max of five timed intervals) and the HIP-event kernel times (an untimed pass) of the grid build and the sweep.
    python scripts/grid_vary_bench.py [--steps 20] [--intervals 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from agile_grasp_amd import binding, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--intervals", type=int, default=5)
    args = ap.parse_args()
    sc = synthetic.config("C2")
    dev = torch.device("cuda:0")
    ctx = binding.Context(sc.cam_origins)
    xyz_t = torch.from_numpy(sc.xyz).to(dev)
    cam_t = torch.from_numpy(sc.cam).to(dev)
    keep = sc.samples[sc.samples < sc.n - 7 * 1500]  # samples valid in every variant
    s_t = torch.from_numpy(np.ascontiguousarray(keep)).to(dev)
    out_t = torch.zeros(8 * keep.size * 160, dtype=torch.uint8, device=dev)
    nout_t = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    views = [(xyz_t[: sc.n - k * 1500], cam_t[: sc.n - k * 1500]) for k in range(8)]
    k = 0

    def step():
        nonlocal k
        x, c = views[k % 8]
        k += 1
        ctx.set_cloud_torch(x, c, stream=stream.cuda_stream)
        ctx.find_hands_torch(s_t, out_t, nout_t, stream=stream.cuda_stream)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # clocks to their steady state
        for _ in range(16):
            step()
        torch.cuda.synchronize()
    ms = []
    for _ in range(args.intervals):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3 / args.steps)
    ctx.set_profile(1)  # kernel times by HIP events in an untimed pass of the same steps
    ctx.timing()
    n_steps = args.steps * args.intervals
    for _ in range(n_steps):
        step()
    torch.cuda.synchronize()
    kt = ctx.timing()
    res = {"workload": "C2 with the point count varying per step (300000 - 1500 (k mod 8))", "steps_per_interval": args.steps,
           "ms_per_step_median": statistics.median(ms), "ms_per_step_min": min(ms), "ms_per_step_max": max(ms),
           "all_ms": [round(v, 5) for v in ms],
           "kernel_us_per_step": {n: round(v * 1e3 / n_steps, 2) for n, v in kt.items() if n in ("grid_build", "hand_sweep")}}
    if hasattr(ctx, "grid_stats"):
        res["grid_stats"] = ctx.grid_stats()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
