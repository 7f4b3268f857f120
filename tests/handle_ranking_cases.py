"""The handle ranking's contract (include/agh.h, agh_set_handle_ranking; DESIGN.md, "Handle ranking") as a numpy model, and the
constructed lists its tests run (numpy only).

  wave_sum     rule 2: W(v, n), the only sum whose order matters -- 64 strided partial sums from +0.0, then the xor butterfly
  terms        rule 3: the seven terms of every handle, float64, left to right
  scores       rules 3-5: SCORE records (score, terms, index, best_inlier) in list order
  order        rule 6: the indices of the handles returned, in rank order, and n_below
  rank         all of it: (handles in rank order, their score records, [n_found, n_below, n_returned])

A ranking is a dict with the fields of agh_handle_ranking_params (missing ones take DEFAULTS).  Hands are HYP records (only
`bottom` is read), handles HANDLE records; the dtypes below restate the binding's, so that the CPU tests need no library."""
import numpy as np

HANDLE_DTYPE = np.dtype([("axis", "<f8", 3), ("center", "<f8", 3), ("approach", "<f8", 3), ("binormal", "<f8", 3),
                         ("hands_center", "<f8", 3), ("width", "<f8"), ("n_inliers", "<i4"), ("first_inlier", "<i4")])
SCORE_DTYPE = np.dtype([("score", "<f8"), ("terms", "<f8", 7), ("index", "<i4"), ("best_inlier", "<i4")])
assert HANDLE_DTYPE.itemsize == 136 and SCORE_DTYPE.itemsize == 72

DEFAULTS = dict(w_support=1.0, w_margin=1.0, w_approach=0.0, w_position=0.0, w_distance=0.0, w_width=0.0, w_length=0.0,
                approach_dir=(0.0, 0.0, -1.0), position_dir=(0.0, 0.0, 1.0), ref_point=(0.0, 0.0, 0.0), preferred_width=0.0,
                min_score=-np.inf, support_cap=10, max_handles=0)
WEIGHTS = ("w_support", "w_margin", "w_approach", "w_position", "w_distance", "w_width", "w_length")
# margins only: the score IS the wave sum over n (the constructed lists are ranked with it)
MARGIN_ONLY = dict(w_support=0.0, w_margin=1.0)


def params(**fields) -> dict:
    bad = set(fields) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **fields)


def wave_sum(v) -> float:
    """W(v, n): p[l] = ((v[l] + v[l + 64]) + v[l + 128]) + ... from +0.0; p[l] = p[l] + p[l ^ o], o = 32 .. 1; p[0]"""
    v = np.asarray(v, np.float64)
    p = np.zeros(64, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, len(v), 64):
            part = v[k0:k0 + 64]
            p[:len(part)] = p[:len(part)] + part
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            p = p + p[lanes ^ o]
    return float(p[0])


def sequential_sum(v) -> float:
    """the plain left-to-right sum, for the tests that show W is another sum"""
    s = np.float64(0.0)
    for x in np.asarray(v, np.float64):
        s = s + x
    return float(s)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def best_inlier(g) -> int:
    """the first k in inlier order with the largest g_k; a NaN never wins; 0 if none wins"""
    best, best_k = 0.0, -1
    for k, x in enumerate(np.asarray(g, np.float64)):
        if x == x and (best_k < 0 or x > best):
            best, best_k = x, k
    return max(best_k, 0)


def scores(rp, hands, margins, handles, inlier_idx) -> np.ndarray:
    """the SCORE records of `handles` in list order.  margins: per hand, or None (zeros: no classifier)"""
    rp = params(**rp)
    out = np.zeros(len(handles), SCORE_DTYPE)
    bottom = np.asarray(hands["bottom"], np.float64).reshape(-1, 3)
    g_all = np.zeros(len(bottom), np.float64) if margins is None else np.asarray(margins, np.float64)
    idx = np.asarray(inlier_idx, np.int64)
    d, pd, ref = (np.asarray(rp[k], np.float64) for k in ("approach_dir", "position_dir", "ref_point"))
    w = [np.float64(rp[k]) for k in WEIGHTS]
    cap = int(rp["support_cap"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for h, hd in enumerate(handles):
            n, first = int(hd["n_inliers"]), int(hd["first_inlier"])
            members = idx[first:first + n]
            g = g_all[members]
            c, a, ax = hd["center"].astype(np.float64), hd["approach"].astype(np.float64), hd["axis"].astype(np.float64)
            b = bottom[members]
            x = (ax[0] * b[:, 0] + ax[1] * b[:, 1]) + ax[2] * b[:, 2]
            e = c - ref
            t = np.zeros(7, np.float64)
            t[0] = np.float64(min(n, cap)) / np.float64(cap)
            t[1] = np.float64(wave_sum(g)) / np.float64(n)
            t[2] = _dot3(a, d)
            t[3] = _dot3(c, pd)
            t[4] = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            t[5] = np.abs(np.float64(hd["width"]) - np.float64(rp["preferred_width"]))
            t[6] = np.fmax.reduce(x, initial=-np.inf) - np.fmin.reduce(x, initial=np.inf)
            s = w[0] * t[0] + w[1] * t[1]
            for k in range(2, 7):
                s = s + w[k] * t[k]
            out[h] = (s, t, h, best_inlier(g))
    return out


def order(sc, rp):
    """(the indices returned, in rank order; n_below): left out iff !(score >= min_score); score descending, NaN behind every
    number, ties (==, so +0 and -0 tie) by ascending index; the first max_handles"""
    rp = params(**rp)
    s = np.asarray(sc["score"], np.float64)
    with np.errstate(invalid="ignore"):
        stays = (s >= rp["min_score"]) | (rp["min_score"] == -np.inf)  # (-inf: no bound at all, a NaN score stays)
    kept = [int(i) for i in np.flatnonzero(stays)]

    def key(i):
        x = s[i]
        return (1, 0.0, i) if x != x else (0, -x if x != 0.0 else 0.0, i)  # (-x: descending; -(+-0) folded onto +0)

    kept.sort(key=key)
    if rp["max_handles"] > 0:
        kept = kept[:rp["max_handles"]]
    return np.asarray(kept, np.int64), int((~stays).sum())


def rank(rp, hands, margins, handles, inlier_idx):
    """(handles in rank order, their SCORE records, [n_found, n_below, n_returned])"""
    sc = scores(rp, hands, margins, handles, inlier_idx)
    keep, n_below = order(sc, rp)
    return handles[keep].copy(), sc[keep].copy(), [len(handles), n_below, len(keep)]


def same_bytes(a, b) -> bool:
    """two record arrays, byte for byte (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_scores(a, b) -> bool:
    """two arrays of SCORE records: index and best_inlier equal, every double equal bit for bit -- the sign of zero included -- or
    NaN in both (an arithmetic NaN's sign and payload are the processor's, not the contract's)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a["index"], b["index"]) or not np.array_equal(a["best_inlier"], b["best_inlier"]):
        return False
    for f in ("score", "terms"):
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if not ((x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))).all():
            return False
    return True


# ---- constructed lists: hands, margins, handles, inlier_idx ----

def hyp_dtype():
    from agile_grasp_amd import binding

    return binding.HYP_DTYPE


def make_list(sizes, margins, seed=1, dtype=None, shuffle=True):
    """a list whose handle h has sizes[h] inliers: sum(sizes) hands with random unit frames and bottoms, the given margins (one per
    hand, in hand order), the inlier lists a random permutation of the hands cut into spans"""
    rng = np.random.default_rng(seed)
    H = int(np.sum(sizes))
    hands = np.zeros(H, dtype if dtype is not None else hyp_dtype())
    hands["bottom"] = rng.uniform(-0.3, 0.3, (H, 3))
    idx = (rng.permutation(H) if shuffle else np.arange(H)).astype(np.int32)
    handles = np.zeros(len(sizes), HANDLE_DTYPE)
    first = 0
    for h, n in enumerate(sizes):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        handles[h]["axis"], handles[h]["approach"], handles[h]["binormal"] = q[:, 0], q[:, 1], q[:, 2]
        handles[h]["center"] = rng.uniform(-0.3, 0.3, 3)
        handles[h]["hands_center"] = rng.uniform(-0.3, 0.3, 3)
        handles[h]["width"] = rng.uniform(0.01, 0.08)
        handles[h]["n_inliers"], handles[h]["first_inlier"] = n, first
        first += n
    g = np.asarray(margins, np.float64)
    assert g.shape == (H,)
    return hands, g, handles, idx


def singles(values, seed=1, dtype=None):
    """a list of len(values) handles of one inlier each; under MARGIN_ONLY handle h's score is values[h] exactly (hand h is handle
    h's: W of one value is the value, over 1.0)"""
    return make_list([1] * len(values), values, seed, dtype, shuffle=False)


def cancelling_margins(n, seed=3):
    """n margins of wildly different magnitudes: their wave sum and their sequential sum round differently"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 9, n)


# Signed zeros: a margin cannot carry one (W starts from +0.0), the products can.  Every weight is -0.0 but the width's, -1.0, and
# signed_zero_list's handles have every term positive but t_approach = -+1 and t_width: a handle of the preferred width scores the
# sum of seven zeros, -0.0 if all are (t_approach = 1) and +0.0 if one is not (t_approach = -1); the others score below zero.
SIGNED_ZERO = dict(w_support=-0.0, w_margin=-0.0, w_approach=-0.0, w_position=-0.0, w_distance=-0.0, w_width=-1.0, w_length=-0.0,
                   preferred_width=0.05)


def signed_zero_list(values, seed=5, dtype=None):
    """one single-inlier handle per value: -0.0 and +0.0 give exactly that score under SIGNED_ZERO, any other value v a score near
    -|v|"""
    values = np.asarray(values, np.float64)
    hands, g, handles, idx = singles(np.ones(len(values)), seed, dtype)
    handles["approach"] = (0.0, 0.0, -1.0)
    handles["approach"][(values == 0.0) & ~np.signbit(values), 2] = 1.0
    handles["center"][:, 2] = np.abs(handles["center"][:, 2]) + 0.1
    handles["width"] = 0.05 + np.abs(values)
    return hands, g, handles, idx


def swapped_pair(n, dtype=None):
    """two handles of n inliers (n a multiple of 64) over the same margins, the second with every inlier k at k ^ 32: their wave
    sums are equal bit for bit, their sequential sums are not (the seed is chosen so that handle 1's is the larger)"""
    assert n % 64 == 0
    for seed in range(3, 40):
        g = cancelling_margins(n, seed)
        swapped = g[np.arange(n) ^ 32]
        if sequential_sum(g) < sequential_sum(swapped):
            break
    return make_list([n, n], np.concatenate([g, swapped]), seed=2, dtype=dtype, shuffle=False)


SPECIAL_SCORES = np.array([0.5, np.nan, -np.inf, 0.0, np.inf, -0.0, 0.5, -1.0, np.nan, np.inf, 0.0, -np.inf, 3.0, -0.0])
