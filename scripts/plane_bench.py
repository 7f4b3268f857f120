"""agh_remove_plane wall time on the C2 and C4 voxel clouds (the cloud is re-set before every call, outside the clock;
the grid build the call queues for the kept cloud is waited for inside it).  Prints one JSON line per scene.
Per-kernel times: run under  rocprofv3 --kernel-trace --stats -- python scripts/plane_bench.py."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from agile_grasp_amd import binding, synthetic  # noqa: E402

K = int(os.environ.get("PLANE_BENCH_STEPS", "20"))
for name in ("C2", "C4"):
    sc = synthetic.config(name)
    ctx = binding.Context(sc.cam_origins)
    times = []
    for k in range(K + 3):
        ctx.set_cloud(sc.xyz, sc.cam)
        ctx.synchronize()
        t0 = time.perf_counter()
        res = ctx.remove_plane()
        ctx.synchronize()
        if k >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"scene": name, "points": sc.n, "n_inliers": res["n_inliers"], "n_remaining": res["n_remaining"],
                      "iterations": res["iterations"], "candidates_drawn": int(len(ctx.plane_candidates()["counts"])),
                      "remove_plane_ms_median": float(np.median(times)), "remove_plane_ms_min": float(np.min(times)),
                      "steps": K}), flush=True)
    ctx.close()
