"""agh_localize_depth_clustered_fit on ONE capture: the six-box depth scene of scripts/localize_cluster_bench.py (two 640 x 480
uint16 depth images, f = 520 px), the table plane NOT given, S = 300 samples per object, classifier on, the library's default fit
parameters (128 candidates, 1 cm, refit on, seed 1).  ms per call (the median of --reps calls after 3 warm-up rounds, the routes
taking turns in one process):
  fitted      agh_localize_depth_clustered_fit: the plane found on the device inside the call
  clustered   (a) agh_localize_depth_clustered given the plane the fit reported: the floor, the same chain without the new stage
  stagewise   (b) the route the call replaces: agh_preprocess on the deprojected points, agh_get_cloud, a host fit with the tests'
              numpy model, then agh_localize_clustered with that plane
The host fit of (b) takes a good part of a second, so that route runs in every third round only (--reps 15: five timed calls).
The claims to record are fitted - clustered (what the stage costs) and fitted / stagewise; a separate kernel trace of
--only-fitted N says which of the four kernels carries the cost.  Every sample is written to --out as JSON, the medians are printed
as one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding
from scripts.localize_cluster_bench import K, S, box_scene
from tests import depth_captures as D
from tests import plane_fit_cases as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_plane_fit_bench.json"))
    ap.add_argument("--only-fitted", type=int, default=0, help="N: just N fitted calls (a kernel trace's workload)")
    a = ap.parse_args()

    xyz, true_plane = box_scene()
    images = [D.render_depth(xyz, k, 640, 480, D.U16, 520.0) for k in range(2)]
    origins = np.stack([im["pose"][:, 3] for im in images])
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    pts = ctx.deproject(images)
    fin = pts[np.isfinite(pts).all(1)]
    ws = np.stack([fin.min(0) - 0.01, fin.max(0) + 0.01], axis=1).reshape(6).astype(np.float64)
    cp_fields = dict(min_height=0.01, max_height=0.5, tolerance=0.01, min_voxels=50, max_objects=K)
    cp = binding.cluster_params(**cp_fields)
    fp = binding.plane_fit_params()
    kw = dict(classify=True, min_inliers=3, min_length=0.005, n_samples=S, sample_seed=7)
    n0 = images[0]["data"].size

    first = ctx.localize_depth_clustered_fit(images, ws, fp, cp, **kw)
    if a.only_fitted:
        for _ in range(a.only_fitted):
            ctx.localize_depth_clustered_fit(images, ws, fp, cp, **kw)
        return
    fit, info = ctx.plane_fit(), ctx.cluster_info()
    assert fit["found"] and fit["refined"]
    given = binding.cluster_params(plane=tuple(fit["plane"]), **cp_fields)
    n_true = np.array(true_plane[:3])
    angle = float(np.degrees(np.arccos(min(1.0, abs(float(fit["plane"][:3] @ n_true))))))

    def counts(res):
        return [(r["n_hypotheses"], len(r["hands"]), len(r["handles"])) for r in res]

    def stagewise():
        ctx.preprocess(pts, n0, ws, dense=True)
        vx, _ = ctx.cloud()
        m = PF.fit_model(vx, {}, origins[0])
        assert np.array_equal(m["plane"], fit["plane"])  # (the model's plane IS the device's)
        return ctx.localize_clustered(pts, n0, ws, binding.cluster_params(plane=tuple(m["plane"]), **cp_fields), dense=True, **kw)

    want = counts(first)
    routes = [
        ("fitted", lambda: counts(ctx.localize_depth_clustered_fit(images, ws, fp, cp, **kw))),
        ("clustered", lambda: counts(ctx.localize_depth_clustered(images, ws, given, **kw))),
        ("stagewise", lambda: counts(stagewise())),
    ]
    samples = {name: [] for name, _ in routes}
    for rep in range(-3, a.reps):
        for name, fn in routes:
            if name == "stagewise" and rep % 3 != 0:
                continue
            t0 = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t0
            assert res == want, name  # the same hypotheses, kept hands and handles per object on every route
            if rep >= 0:
                samples[name].append(round(dt * 1e3, 4))
    med = {name: round(float(np.median(t)), 4) for name, t in samples.items()}
    out = {"capture": "2 x 640x480 uint16, f = 520 px, a table with six boxes", "n_samples_per_object": S, "max_objects": K,
           "reps": a.reps, "n_candidates": int(fp.n_candidates), "distance_threshold": float(fp.distance_threshold),
           "n_voxels": int(fit["n_voxels"]), "n_inliers": int(fit["n_inliers"]), "n_refit": int(fit["n_refit"]),
           "best_candidate": int(fit["best_candidate"]), "plane": [float(v) for v in fit["plane"]],
           "angle_to_the_scene_plane_deg": round(angle, 5), "n_objects": int(info["n_objects"]),
           "object_voxels": info["n_voxels"].tolist(), "hypotheses": [c[0] for c in want], "hands": [c[1] for c in want],
           "handles": [c[2] for c in want], "median_ms": med,
           "min_max_ms": {name: [min(t), max(t)] for name, t in samples.items()},
           "fitted_minus_clustered_ms": round(med["fitted"] - med["clustered"], 4),
           "fitted_over_stagewise": round(med["fitted"] / med["stagewise"], 5), "samples_ms": samples}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "samples_ms"}))


if __name__ == "__main__":
    main()
