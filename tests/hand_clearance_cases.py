"""The hand clearance's contract (include/agh.h, agh_set_hand_clearance; DESIGN.md, "Hand clearance") as a numpy model, and the
scenes and regimes its tests run (numpy only).

  palm_points       rule 1: the palm o of every hypothesis, from its sample's point, bottom, binormal, approach and bite
  body_coords       rule 2: (xb, yb, zb) of every cloud point in every hand's frame, float64, left to right
  corridor_counts   rules 2-4: the points of the WHOLE cloud inside each hand's corridor, by brute force
  drop              rule 5: the decision per hypothesis, behind the hand filter's reasons (a hand they drop is not tested)
  counts            [n_tested, n_dropped, n_kept] as agh_get_hand_clearance_counts reports

A clearance is a dict with the fields of agh_hand_clearance_params (missing ones take DEFAULTS).  The scenes are
hand_filter_cases.box_scene's: a box on a table in one or two 160 x 120 views, whose table is what most corridors meet."""
import numpy as np

from tests import hand_filter_cases as HF

DEFAULTS = dict(near_offset=0.0, far_offset=0.12, half_width=0.05, half_height=0.04, max_points=0)
GEOMETRY = HF.GEOMETRY
# the regimes tests/test_hand_clearance_cases.py pins on box_scene(1) and box_scene(2)
BODY = dict(near_offset=0.0, far_offset=0.20, half_width=0.06, half_height=0.05)       # a larger gripper body
FINGERS = dict(near_offset=0.0, far_offset=0.10, half_width=0.045, half_height=0.02)  # the fingers' own cross-section
LARGEST = dict(near_offset=0.0, far_offset=0.5, half_width=0.25, half_height=0.25)    # the bounds of the record


def params(**fields) -> dict:
    bad = set(fields) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **fields)


def palm_points(hyps, sample_points, geom=GEOMETRY) -> np.ndarray:
    """(H, 3) float64: o = (s + h x binormal) + y0 x approach.  sample_points: (H, 3), the float32 point of each hypothesis'
    sample in the voxelised cloud."""
    s = np.asarray(sample_points, np.float32).astype(np.float64).reshape(-1, 3)
    bottom, binormal = hyps["bottom"].astype(np.float64), hyps["binormal"].astype(np.float64)
    approach = hyps["approach"].astype(np.float64)
    h = HF.dot3(bottom - s, binormal)
    table = HF.bite_table(geom)
    y0 = table[np.clip(hyps["depth_index"], 0, len(table) - 1)] - geom["hand_depth"]
    return (s + h[:, None] * binormal) + y0[:, None] * approach


def body_coords(hyps, palms, cloud):
    """(xb, yb, zb), each (H, N) float64: cloud point j in hand i's frame -- e = p - o, then (e0 v0 + e1 v1) + e2 v2"""
    p = np.asarray(cloud, np.float32).astype(np.float64).reshape(-1, 3)
    e = p[None, :, :] - np.asarray(palms, np.float64)[:, None, :]
    out = []
    for name in ("binormal", "approach", "axis"):
        v = hyps[name].astype(np.float64)[:, None, :]
        out.append((e[..., 0] * v[..., 0] + e[..., 1] * v[..., 1]) + e[..., 2] * v[..., 2])
    return out[0], out[1], out[2]


def in_corridor(xb, yb, zb, cp) -> np.ndarray:
    """rule 2: four closed comparisons; a NaN compares false"""
    with np.errstate(invalid="ignore"):
        return (-cp["far_offset"] <= yb) & (yb <= -cp["near_offset"]) & (np.abs(xb) <= cp["half_width"]) & (np.abs(zb) <= cp["half_height"])


def corridor_counts(hyps, sample_points, cloud, cp, geom=GEOMETRY, chunk=64) -> np.ndarray:
    """(H,) int64: the points of `cloud` (all of it: brute force) inside each hand's corridor"""
    cp = params(**cp)
    out = np.zeros(len(hyps), np.int64)
    palms = palm_points(hyps, sample_points, geom)
    for i in range(0, len(hyps), chunk):
        with np.errstate(invalid="ignore"):
            xb, yb, zb = body_coords(hyps[i:i + chunk], palms[i:i + chunk], cloud)
        out[i:i + chunk] = in_corridor(xb, yb, zb, cp).sum(1)
    return out


def drop(hyps, sample_points, cloud, cp, reason=None, geom=GEOMETRY) -> np.ndarray:
    """bool per hypothesis: dropped by the clearance.  reason: the hand filter's reasons (hand_filter_cases.drop_reasons), if one
    is set -- a hand it dropped is not tested and is not counted here."""
    cp = params(**cp)
    d = corridor_counts(hyps, sample_points, cloud, cp, geom) > cp["max_points"]
    if reason is not None:
        d &= np.asarray(reason) == 0
    return d


def counts(dropped, reason=None) -> list:
    """[n_tested, n_dropped, n_kept] as agh_get_hand_clearance_counts reports"""
    tested = len(dropped) if reason is None else int((np.asarray(reason) == 0).sum())
    return [tested, int(np.asarray(dropped).sum()), tested - int(np.asarray(dropped).sum())]


# ---- regime predicates ----

def bites(dropped, least=5) -> bool:
    """the regime is non-empty on both sides: at least `least` hands dropped and as many kept"""
    d = np.asarray(dropped)
    return int(d.sum()) >= least and int((~d).sum()) >= least


def mostly_clear(c, share=0.95) -> bool:
    """at least `share` of the hands have an empty corridor"""
    return len(c) > 0 and float((np.asarray(c) == 0).mean()) >= share


def pick_small_count(c, lo=1, hi=10):
    """a hand whose corridor holds lo .. hi points (the threshold tests): its index, or None"""
    k = np.flatnonzero((np.asarray(c) >= lo) & (np.asarray(c) <= hi))
    return int(k[0]) if len(k) else None


def two_scene(seed: int = 6) -> dict:
    """a second capture unlike box_scene(2): other intrinsics and samples, so that the two clouds of a batch differ"""
    return HF.box_scene(2, seed=seed, f=190.0)
