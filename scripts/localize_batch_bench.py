"""agh_localize_batch against agh_localize one capture after the other, on C2-style raw captures (700k points, 2000 drawn
samples, classifier on), batches of 1 / 4 / 8.  Medians over --reps calls, ms PER CAPTURE:
  batch_host      agh_localize_batch (host buffers: the captures are packed end to end and uploaded)
  batch_device    agh_localize_batch_device (torch CUDA tensors read in place)
  sequential      agh_localize on each capture of the batch, one after the other, on one context
  two_contexts    the same captures on two contexts taking turns: agh_localize_begin(k + 1) on the other context before
                  agh_localize_end(k) (the two chains' kernels side by side) -- what a caller could do before the batch
--mixed-origins: eight captures under FOUR origin pairs (captures 2j, 2j + 1 under pair j), ms per capture:
  mixed_batch_host    one agh_localize_batch with the per-cloud origin table (agh_set_cloud_cam_origins)
  mixed_four_contexts the same captures through four contexts, one per origin pair, agh_localize one after the other
  shared_batch_host   the batch without a table (what the table costs)
--staged: the same eight captures, pinned and pageable sources, ms per capture, all in one run:
  blocking_*_ms   agh_localize_batch from host buffers, call after call
  staged_*_ms     the stream agh_localize_batch_stage(k + 1) -> agh_localize_batch_end(k) -> agh_localize_batch_begin(k + 1) over two
                  sets of buffers taking turns (one iteration = one batch; the upload of the next batch runs under this one's
                  kernels); the iterations are timed back to back (median of their durations, and *_mean_ms = the loop's wall
                  clock over its iterations), the results are compared after the loop
  device_ms       agh_localize_batch_device (the captures already on the device: the floor of the staged stream)
  and writes the JSON line to --out as well.
One JSON line; the GPU and the way it was run go in with --note.  scripts/localize_batch_trace.sh takes the kernel trace."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from agile_grasp_amd import binding, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def mixed_origins(a):
    caps = [synthetic.make_raw_cloud(700_000, 21 + k) for k in range(8)]
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    base = np.asarray(caps[0].cam_origins, np.float64)
    pairs = [base + np.array([0.0, 0.15 * j, 0.05 * j]) for j in range(4)]  # four rigs side by side
    tab = np.stack([pairs[k // 2] for k in range(8)])
    ctxs = [binding.Context(p) for p in pairs]
    for c in ctxs:
        c.load_svm(z["w"], float(z["rho"]))
    kw = dict(classify=True, min_inliers=3, min_length=0.005)
    sl, ws, seeds = [c.size_left for c in caps], [c.workspace for c in caps], [5 + k for k in range(8)]
    batch = lambda: ctxs[0].localize_batch([c.xyz for c in caps], sl, ws, n_samples=2000, sample_seeds=seeds, **kw)
    shared = median_ms(batch, a.reps)
    ctxs[0].set_cloud_cam_origins(tab)
    mixed = median_ms(batch, a.reps)
    got = batch()
    ctxs[0].set_cloud_cam_origins(None)

    def four():
        return [ctxs[k // 2].localize(c.xyz, c.size_left, c.workspace, n_samples=2000, sample_seed=seeds[k], **kw)
                for k, c in enumerate(caps)]

    per = median_ms(four, a.reps)
    def equal(g, r):  # every field of every hand but the call's stamp, every handle field, the inlier lists and the counts
        return (g["n_voxels"] == r["n_voxels"] and g["n_hypotheses"] == r["n_hypotheses"] and len(g["hands"]) == len(r["hands"]) and
                all(np.array_equal(g["hands"][f], r["hands"][f]) for f in g["hands"].dtype.names if f != "epoch") and
                len(g["handles"]) == len(r["handles"]) and
                all(np.array_equal(g["handles"][f], r["handles"][f]) for f in g["handles"].dtype.names) and
                np.array_equal(g["inlier_idx"], r["inlier_idx"]) and np.array_equal(g["samples"], r["samples"]))

    same = all(equal(g, r) for g, r in zip(got, four()))
    print(json.dumps({"points": 700_000, "samples": 2000, "reps": a.reps, "note": a.note, "captures": 8, "origin_pairs": 4,
                      "mixed_batch_host_ms": round(mixed / 8, 4), "mixed_four_contexts_ms": round(per / 8, 4),
                      "shared_batch_host_ms": round(shared / 8, 4), "results_equal": bool(same)}))


def staged(a):
    import torch

    caps = [synthetic.make_raw_cloud(700_000, 21 + k) for k in range(8)]
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(caps[0].cam_origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    sl, ws, seeds = [c.size_left for c in caps], [c.workspace for c in caps], [5 + k for k in range(8)]
    kw = dict(n_samples=2000, sample_seeds=seeds, classify=True, min_inliers=3, min_length=0.005)
    out = {"points": 700_000, "samples": 2000, "captures": 8, "reps": a.reps, "note": a.note}

    def equal(got, ref):
        return all(g["n_voxels"] == r["n_voxels"] and g["n_hypotheses"] == r["n_hypotheses"] and
                   all(np.array_equal(g["hands"][f], r["hands"][f]) for f in g["hands"].dtype.names if f != "epoch") and
                   all(np.array_equal(g["handles"][f], r["handles"][f]) for f in g["handles"].dtype.names) and
                   np.array_equal(g["inlier_idx"], r["inlier_idx"]) and np.array_equal(g["samples"], r["samples"])
                   for g, r in zip(got, ref))

    same = True
    for kind in ("pinned", "pageable"):
        make = (lambda x: torch.from_numpy(np.array(x)).pin_memory().numpy()) if kind == "pinned" else (lambda x: np.array(x))
        sets = [[make(c.xyz) for c in caps] for _ in range(2)]  # two sets of buffers taking turns, as a directory walk has
        turn = [0]

        def blocking():
            turn[0] ^= 1
            return ctx.localize_batch(sets[turn[0]], sl, ws, **kw)

        out[f"blocking_{kind}_ms"] = round(median_ms(blocking, a.reps) / 8, 4)
        ref = blocking()
        # The stream is timed as a whole: the stamps are taken back to back, one per batch collected, so that no GPU work of a
        # queued chain runs under untimed host code; the results are kept and compared after the loop.
        ctx.localize_batch_begin(sets[0], sl, ws, **kw)
        stamps, kept, nxt = [time.perf_counter()], [], 1
        for i in range(3 + a.reps):
            up = ctx.localize_batch_stage(sets[nxt])
            kept.append(ctx.localize_batch_end())
            ctx.localize_batch_begin(up, sl, ws, **kw)
            stamps.append(time.perf_counter())
            nxt ^= 1
        kept.append(ctx.localize_batch_end())
        same = same and all(equal(got, ref) for got in kept)
        d = np.diff(np.array(stamps[3:])) * 1e3  # (a.reps consecutive iterations, the first three left out)
        out[f"staged_{kind}_ms"] = round(float(np.median(d)) / 8, 4)
        out[f"staged_{kind}_mean_ms"] = round(float(stamps[-1] - stamps[3]) * 1e3 / a.reps / 8, 4)
    dev = [torch.from_numpy(c.xyz).cuda() for c in caps]
    out["device_ms"] = round(median_ms(lambda: ctx.localize_batch(dev, sl, ws, **kw), a.reps) / 8, 4)
    out["results_equal"] = bool(same)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--note", default="")
    ap.add_argument("--batch-only", action="store_true", help="the batch calls alone (for a kernel trace)")
    ap.add_argument("--mixed-origins", action="store_true", help="eight captures under four origin pairs: table batch against four contexts")
    ap.add_argument("--staged", action="store_true", help="blocking, staged begin/stage/end and device batches of eight, in one run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_batch_staged.json"), help="--staged: where the line goes")
    a = ap.parse_args()
    if a.mixed_origins:
        return mixed_origins(a)
    if a.staged:
        return staged(a)
    import torch

    sizes = [int(b) for b in a.batches.split(",")]
    caps = [synthetic.make_raw_cloud(700_000, 21 + k) for k in range(max(sizes))]
    z = np.load(os.path.join(ROOT, "tests", "golden", "svm_weights.npz"))
    ctx = binding.Context(caps[0].cam_origins)
    ctx.load_svm(z["w"], float(z["rho"]))
    other = binding.Context(caps[0].cam_origins)
    other.load_svm(z["w"], float(z["rho"]))
    dev = [torch.from_numpy(c.xyz).cuda() for c in caps]
    kw = dict(classify=True, min_inliers=3, min_length=0.005)
    out = {"points": 700_000, "samples": 2000, "reps": a.reps, "note": a.note}
    for B in sizes:
        cs = caps[:B]
        sl, ws = [c.size_left for c in cs], [c.workspace for c in cs]
        seeds = [5 + k for k in range(B)]
        host = median_ms(lambda: ctx.localize_batch([c.xyz for c in cs], sl, ws, n_samples=2000, sample_seeds=seeds, **kw), a.reps)
        devb = median_ms(lambda: ctx.localize_batch(dev[:B], sl, ws, n_samples=2000, sample_seeds=seeds, **kw), a.reps)
        if a.batch_only:
            out[f"b{B}"] = {"batch_host_ms": round(host / B, 4), "batch_device_ms": round(devb / B, 4)}
            continue

        def seq():
            for k, c in enumerate(cs):
                ctx.localize(c.xyz, c.size_left, c.workspace, n_samples=2000, sample_seed=seeds[k], **kw)

        sq = median_ms(seq, a.reps)

        def turns():
            pair = (ctx, other)
            for k, c in enumerate(cs):
                pair[k % 2].localize_begin(c.xyz, c.size_left, c.workspace, n_samples=2000, sample_seed=seeds[k], **kw)
                if k > 0:
                    pair[(k - 1) % 2].localize_end()
            pair[(len(cs) - 1) % 2].localize_end()

        two = median_ms(turns, a.reps)
        out[f"b{B}"] = {"batch_host_ms": round(host / B, 4), "batch_device_ms": round(devb / B, 4),
                        "sequential_ms": round(sq / B, 4), "two_contexts_ms": round(two / B, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
