"""The fused localize chain with and without the workspace-boundary filter (agh_localize_params::filters_boundaries: the
reference's nodes build Localization(.., filters_boundaries = true, ..)) on the 700k-point raw capture of the README's localize
figures, with a workspace face that cuts through the scene so that the filter bites.  Medians over --reps calls, ms:
  fused_plain     agh_localize, no filter
  fused_filtered  agh_localize, filters_boundaries = 1
  staged_filtered agh_localize_begin / _stage (the next capture) / _end, filtered, per capture of a stream
  three_calls     what the adapter did before the chain could filter: preprocess -> find_hands -> classify (the whole list)
                  -> filterHands on the host -> find_handles
One JSON line.  --mode plain|filtered runs only that fused chain (for a kernel trace of one against the other)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def near(hyps, ws):
    s = hyps["surface"]
    m = np.zeros(len(hyps), bool)
    for k in range(6):
        m |= np.abs(s[:, k // 2] - ws[k]) < 0.02
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--mode", default="all", choices=["all", "plain", "filtered"])
    a = ap.parse_args()
    rc = synthetic.make_raw_cloud(700_000, 21)
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(rc.cam_origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    ws = np.array(rc.workspace, np.float64)
    fin = rc.xyz[np.isfinite(rc.xyz).all(1)]
    ws[1] = float(np.percentile(fin[(fin[:, 0] >= ws[0]) & (fin[:, 0] <= ws[1]), 0], 75))  # x max through the scene
    nv = ctx.preprocess(rc.xyz, rc.size_left, ws)
    samples = np.sort(np.random.default_rng(5).permutation(nv)[:2000]).astype(np.int32)
    kw = dict(samples=samples, classify=True, min_inliers=3, min_length=0.005)

    def timed(fn):
        for _ in range(3):
            fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return round(float(np.median(t)) * 1e3, 4)

    out = {"n_voxels": int(nv), "n_samples": len(samples), "ws_xmax": ws[1]}
    if a.mode in ("all", "plain"):
        out["fused_plain_ms"] = timed(lambda: ctx.localize(rc.xyz, rc.size_left, ws, **kw))
    if a.mode in ("all", "filtered"):
        out["fused_filtered_ms"] = timed(lambda: ctx.localize(rc.xyz, rc.size_left, ws, filters_boundaries=True, **kw))
    if a.mode == "all":
        # the stream: two capture objects taking turns, the next one staged under this one's kernels
        caps = [np.ascontiguousarray(rc.xyz), np.ascontiguousarray(rc.xyz.copy())]
        state = {"i": 0}
        ctx.localize_begin(caps[0], rc.size_left, ws, filters_boundaries=True, **kw)

        def staged():
            i = state["i"]
            nxt = caps[(i + 1) & 1]
            ctx.localize_stage(nxt)
            r = ctx.localize_end()
            ctx.localize_begin(nxt, rc.size_left, ws, filters_boundaries=True, **kw)
            state["i"] = i + 1
            return r

        out["staged_filtered_ms"] = timed(staged)
        ctx.localize_end()

        def three_calls():
            ctx.preprocess(rc.xyz, rc.size_left, ws)
            h = ctx.find_hands(samples)
            k = ctx.classify().astype(bool)
            h = h[k & ~near(h, ws)]
            return h, ctx.find_handles(h, 3, 0.005)

        out["three_calls_ms"] = timed(three_calls)
        # the same results, and how much the filter bit
        r = ctx.localize(rc.xyz, rc.size_left, ws, filters_boundaries=True, **kw)
        h, (hd, idx) = three_calls()
        assert len(r["hands"]) == len(h) and np.array_equal(r["inlier_idx"], idx) and len(r["handles"]) == len(hd)
        ctx.preprocess(rc.xyz, rc.size_left, ws)
        hy = ctx.find_hands(samples)
        kp = ctx.classify().astype(bool)
        m = near(hy, ws)
        out.update(n_hypotheses=len(hy), n_filtered=int(m.sum()), filtered_share=round(float(m.mean()), 4),
                   n_kept_plain=int(kp.sum()), n_kept_filtered=int((kp & ~m).sum()), n_handles=len(hd))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
