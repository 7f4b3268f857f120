"""Inputs at exact counts: clouds whose neighbourhoods, hand crops and handle-search rows sit on the boundaries where the
kernels change template instantiation, tile, LDS class or launch (tests/test_capacity_clouds.py checks every case against
the oracle and numpy on the CPU; tests/test_gpu_capacity_edges.py runs them on the GPU).

Plain numpy, no GPU.  Every point is placed at least MARGIN inside or outside each sphere and slab that decides a count,
so float32 rounding cannot move a point across.
"""
from __future__ import annotations

import numpy as np

MARGIN = 1e-4
SPACING = 0.25  # between the samples of one cloud: more than r_hands + r_taubin (0.08 + 0.03), so regions never overlap
ORIGIN = np.array([0.7, -0.5, -0.5])  # in front of synthetic.camera_origins(), which look along +x
HAND_DEFAULTS = dict(nn_radius_taubin=0.03, nn_radius_hands=0.08, hand_height=0.02)


def cams():
    from agile_grasp_amd import synthetic

    return synthetic.camera_origins()


def flann_d2(xyz, q):
    """FLANN's float32 squared distance, in its order of operations (the kernels' d2)."""
    d = np.asarray(xyz, np.float32) - np.asarray(q, np.float32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def in_ball(xyz, q, r):
    return flann_d2(xyz, q) < np.float32(r * r)


def _site(k):
    """Centre of the k-th sample region: a 6-wide grid in the y-z plane (the patches face the cameras along -x)."""
    return ORIGIN + SPACING * np.array([0.0, k % 6, k // 6])


def _surface(rng, centre, n, rmax, noise=3e-4):
    """n points of a noisy curved patch through `centre` (normal -x), spread over the disk of radius rmax."""
    rad = rmax * np.sqrt(rng.random(n))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    u, v = rad * np.cos(phi), rad * np.sin(phi)
    w = 2.0 * u * u - 1.2 * v * v + rng.normal(0.0, noise, n)
    return centre + np.stack([w, u, v], 1)


def _ball_points(rng, centre, n_in, r, n_out):
    """The sample (first row), n_in - 1 further points at least MARGIN inside the ball of radius r around it and n_out
    points at least MARGIN outside it (up to 1.5 r): float32 rows."""
    q = np.asarray(centre, np.float32)
    inside, outside = [], []
    need_in, need_out = n_in - 1, n_out
    while need_in > 0 or need_out > 0:
        cand = _surface(rng, centre, 4 * (need_in + need_out) + 64, 1.5 * r).astype(np.float32)
        d = np.sqrt(flann_d2(cand, q).astype(np.float64))
        a = cand[(d < r - MARGIN) & (d > 0)][:max(need_in, 0)]
        b = cand[d > r + MARGIN][:max(need_out, 0)]
        inside.append(a)
        outside.append(b)
        need_in -= len(a)
        need_out -= len(b)
    return np.concatenate([q[None]] + inside + outside)


def ball_cloud(targets, r=0.03, seed=0, filler=0, total=None):
    """One cloud with one sample per target N whose FLANN ball of radius r holds exactly N points (the sample included).
    `filler` ordinary points (a sparse patch of their own, far from every sample) may be added, or as many as make the
    cloud `total` points long.  Returns (xyz float32, cam int32, samples int32)."""
    rng = np.random.default_rng(seed)
    parts, samples, n = [], [], 0
    for k, t in enumerate(targets):
        pts = _ball_points(rng, _site(k), int(t), r, int(min(max(t // 2, 20), 2000)))
        samples.append(n)
        parts.append(pts)
        n += len(pts)
    if total is not None:
        filler = total - n
        assert filler >= 0, (total, n)
    if filler:
        parts.append(_surface(rng, _site(len(targets)), filler, 0.1, noise=2e-3).astype(np.float32))
    xyz = np.concatenate(parts).astype(np.float32)
    cam = (rng.random(len(xyz)) < 0.5).astype(np.int32)
    return xyz, cam, np.array(samples, np.int32)


def crop_count(xyz, sample_xyz, axis, r_hands, hand_height):
    """Points of the hand crop as k_hand_sweep counts them (hand_search.cpp:141-158, rotating_hand.cpp:26,37-51): inside
    the FLANN ball of r_hands and |tz| < hand_height, tz = the fp64 dot of the frame's axis with the float32 difference."""
    d = np.asarray(xyz, np.float32) - np.asarray(sample_xyz, np.float32)
    inball = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < np.float32(r_hands * r_hands)
    c = d.astype(np.float64)
    tz = (axis[0] * c[:, 0] + axis[1] * c[:, 1]) + axis[2] * c[:, 2]
    return int((inball & (tz > -1.0 * hand_height) & (tz < hand_height)).sum())


def _params(geom, **kw):
    import os

    from oracle import oracle_py as O

    return O.default_params(cams(), num_threads=min(os.cpu_count() or 1, 16), **{**geom, **kw})


def crop_cloud(targets, geom=None, seed=0, pad_samples=0, base=400):
    """One cloud with one sample per target T whose hand crop holds exactly T points.  Each sample sits on a small curved
    patch (every point within 0.018 m, so its Taubin ball -- and its frame -- is the patch); the crop is then topped up
    with points in the shell 1.2 r_taubin < d < 0.9 r_hands and the slab |axis . (p - s)| < hand_height / 2, in a
    sector behind the surface (inside the hand's closing region of the middle orientations).  Those points change the crop
    and not the frame.  `pad_samples` ordinary samples of a filler patch follow.  Returns (xyz, cam, samples, frames):
    the frames are the oracle's for the crop samples."""
    from oracle import oracle_py as O

    g = {**HAND_DEFAULTS, **(geom or {})}
    rt, rh, hh = g["nn_radius_taubin"], g["nn_radius_hands"], g["hand_height"]
    rng = np.random.default_rng(seed)
    patches, samples, n = [], [], 0
    for k in range(len(targets)):
        c = _site(k)
        pts = np.concatenate([c[None], _surface(rng, c, base - 1, 0.017)]).astype(np.float32)
        samples.append(n)
        patches.append(pts)
        n += len(pts)
    xyz = np.concatenate(patches)
    cam = (rng.random(len(xyz)) < 0.5).astype(np.int32)
    s = np.array(samples, np.int32)
    fr = O.fit_frames(_params(g), xyz, cam, s, rt)
    extra = []
    for k, t in enumerate(targets):
        q = xyz[s[k]]
        ax, nm = fr["axis"][k], fr["normal"][k]
        inward = np.array([1.0, 0.0, 0.0])  # away from the cameras
        inward = inward - np.dot(inward, ax) * ax
        inward /= np.linalg.norm(inward)
        side = np.cross(ax, inward)
        have = crop_count(patches[k], q, ax, rh, hh)
        need = int(t) - have
        assert need >= 0, (t, have)
        got = []
        while need > 0:
            m = 2 * need + 64
            rad = rng.uniform(1.2 * rt + 2 * MARGIN, 0.9 * rh - 2 * MARGIN, m)
            phi = rng.uniform(-0.6, 0.6, m)
            a = rng.uniform(-(hh / 2 - 2 * MARGIN), hh / 2 - 2 * MARGIN, m)
            p = (q.astype(np.float64) + rad[:, None] * (np.cos(phi)[:, None] * inward + np.sin(phi)[:, None] * side)
                 + a[:, None] * ax).astype(np.float32)
            dd = p - q
            dist = np.sqrt(((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).astype(np.float64))
            cc = dd.astype(np.float64)
            tz = (ax[0] * cc[:, 0] + ax[1] * cc[:, 1]) + ax[2] * cc[:, 2]
            ok = (dist > 1.2 * rt + MARGIN) & (dist < 0.9 * rh - MARGIN) & (np.abs(tz) < hh / 2 - MARGIN)
            p = p[ok][:need]
            got.append(p)
            need -= len(p)
        extra.append(np.concatenate(got) if got else np.zeros((0, 3), np.float32))
    xyz = np.concatenate([xyz] + extra)
    cam = np.concatenate([cam, (rng.random(len(xyz) - len(cam)) < 0.5).astype(np.int32)])
    if pad_samples:
        f0 = len(xyz)
        fill = _surface(rng, _site(len(targets)), pad_samples, 0.1, noise=2e-3).astype(np.float32)
        xyz = np.concatenate([xyz, fill])
        cam = np.concatenate([cam, (rng.random(pad_samples) < 0.5).astype(np.int32)])
        s = np.concatenate([s, np.arange(f0, f0 + pad_samples, dtype=np.int32)])
    return xyz.astype(np.float32), cam.astype(np.int32), s.astype(np.int32), fr


# ---- hands for the handle search -------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _hand(dtype, axis, appr, bottom, width):
    r = np.zeros(1, dtype)[0]
    r["axis"], r["approach"], r["bottom"] = axis, appr, bottom
    r["surface"] = bottom - 0.03 * appr
    r["binormal"] = np.cross(appr, axis)
    r["width"] = width
    r["valid"] = 1
    return r


BIG_AXIS = _unit(np.array([0.2, 0.9, 0.1]))
BIG_APPROACH = _unit(np.cross(BIG_AXIS, np.array([0.0, 0.0, 1.0])))


def big_members(hands):
    """Mask of the hands of handle_hands' big handle (every other hand's approach opposes it)."""
    return hands["approach"] @ BIG_APPROACH > 0.9


def handle_hands(H, big=0, seed=0, per=14):
    """H hypothesis records: straight handles of `per` hands each along random lines (the idea of test_handles._crafted)
    and, with big > 0, one handle of `big` hands that are all inliers of each other (common axis and approach up to small
    noise, bottoms within 1 mm of one 0.1 m line) -- the seed of that handle that comes first
    has exactly `big` inliers.  The rest is clutter whose approach opposes the big handle's, so it never joins it."""
    from oracle import oracle_py as orc

    dt = orc.HYP_DTYPE
    rng = np.random.default_rng(seed)
    recs = []
    big_axis, big_appr = BIG_AXIS, BIG_APPROACH
    big_origin = np.array([0.0, -0.6, 0.0])
    for k in range(big):
        t = 0.1 * k / max(big, 1)
        recs.append(_hand(dt, _unit(big_axis + rng.normal(scale=0.01, size=3)) * (1 if rng.random() < 0.8 else -1),
                          _unit(big_appr + rng.normal(scale=0.01, size=3)),
                          big_origin + t * big_axis + rng.normal(scale=3e-4, size=3), rng.uniform(0.01, 0.08)))
    rest = H - big
    n_handles = rest // (2 * per)
    for h in range(n_handles):
        axis = _unit(rng.normal(size=3))
        appr = _unit(np.cross(axis, rng.normal(size=3)))
        if np.dot(appr, big_appr) > 0:
            appr = -appr
        origin = rng.uniform(-0.4, 0.4, 3)
        t = np.sort(rng.uniform(0.0, 0.12, per))
        if h % 2 == 1:
            t[per // 2:] += 0.03  # a gap for shortenHandle
        for k in range(per):
            a = _unit(appr + rng.normal(scale=0.03, size=3))
            recs.append(_hand(dt, _unit(axis + rng.normal(scale=0.02, size=3)) * (1 if rng.random() < 0.8 else -1), a,
                              origin + t[k] * axis + rng.normal(scale=0.001, size=3), rng.uniform(0.01, 0.08)))
    while len(recs) < H:
        a = _unit(rng.normal(size=3))
        if np.dot(a, big_appr) > 0:
            a = -a
        b = rng.uniform(-0.4, 0.4, 3)
        recs.append(_hand(dt, _unit(rng.normal(size=3)), a, b, rng.uniform(0.01, 0.08)))
    hands = np.array(recs, dt)
    return hands[rng.permutation(len(hands))]


def seed_inliers(hands, i):
    """Potential inliers of seed i before any hand is retired (handle_search.cpp:19-28) -- of ALL hands, the ones with
    width = -1 included: what k_handle_pairs writes into rowcnt."""
    ia, ip, inn = hands["axis"][i], hands["bottom"][i], hands["approach"][i]
    d = hands["bottom"] - ip
    P = np.eye(3) - np.outer(ia, ia)
    v = d @ P.T
    dist = np.sqrt((v * v).sum(1))
    aa = np.clip(hands["axis"] @ ia, -1, 1)
    nn = np.clip(hands["approach"] @ inn, -1, 1)
    ang = np.arccos(aa)
    return int(((dist < 0.01) & (np.minimum(ang, np.pi - ang) < 0.34) & (np.arccos(nn) < 0.34)).sum())


def along_seed(hands, i, members):
    """dist_along_line of `members` from seed i (handle_search.cpp:34), in the oracle's order of operations."""
    ia = hands["axis"][i]
    d = hands["bottom"][members] - hands["bottom"][i]
    return (ia[0] * d[:, 0] + ia[1] * d[:, 1]) + ia[2] * d[:, 2]


def big_row_sorted(hands):
    """The big row as its first seed (the member with the lowest index) sorts it: (seed, members in (distance, index) order,
    their distances) -- std::sort's order on (dist_along_line, j), the order the walk cuts."""
    members = np.flatnonzero(big_members(hands))
    seed = int(members[0])
    dist = along_seed(hands, seed, members)
    order = np.lexsort((members, dist))
    return seed, members[order], dist[order]


def handle_row_hands(H, big, seed=0, gap_after=None, ties=0, dead=0):
    """handle_hands(H, big, seed) with the big row reshaped (no option: the same arrays, bit for bit).  Positions are those of
    big_row_sorted, i.e. of the list the first seed of the row sorts.
      gap_after = k  the hands after sorted position k move 3 cm on along the seed's axis (bottom and surface): the gap
                     between positions k and k + 1 is more than the 2 cm of shortenHandle, which keeps the k hands before it
      ties = m       m pairs of neighbours of the sorted list share one `bottom` exactly: their distance along ANY seed's axis
                     is equal and the index decides.  The pairs are the sorted positions (63, 64), (61, 62), (65, 66),
                     (59, 60), ...: the first straddles the two slots of the sorted list
      dead = d       d hands of the row (spread evenly over it, its first seed left out) get width = -1: retired before the search
                     begins, and still counted in rowcnt (k_handle_pairs does not look at the width)"""
    hands = handle_hands(H, big, seed)
    if gap_after is None and not ties and not dead:
        return hands
    first, members, dist = big_row_sorted(hands)
    ax = hands["axis"][first]
    if gap_after is not None:
        assert 0 < gap_after < big - 1, (gap_after, big)
        moved = members[gap_after + 1:]
        hands["bottom"][moved] += 0.03 * ax
        hands["surface"][moved] += 0.03 * ax
    for t in range(ties):
        p = 63 + (-1 if t % 2 else 1) * 2 * ((t + 1) // 2)
        assert 0 < p and p + 1 < big, (p, big)
        a, b = members[p], members[p + 1]
        hands["surface"][b] += hands["bottom"][a] - hands["bottom"][b]
        hands["bottom"][b] = hands["bottom"][a]
    if dead:
        rest = members[members != first]  # (the row's first seed stays alive: the positions are its list's)
        pos = np.unique(np.round(np.linspace(0, big - 2, dead)).astype(int))
        assert len(pos) == dead, (dead, big)
        hands["width"][rest[pos]] = -1.0
    return hands


# ---- the cases (shared by the CPU check and the GPU tests; the threshold table ties each one to its source constant) ----
TAUBIN_DET = (1, 2, 9, 10, 63, 64, 65, 128, 129, 256, 257, 1151, 1152, 1153, 4095, 4096, 4097, 6143, 6144, 6145)
RAND50_EDGE = (49, 50, 51, 1152, 1153)  # early in the list, ordinary samples follow
ALLPOINTS = (128, 129, 256, 257, 1152, 1153)  # r = nn_radius_normals = 0.01
ALLPOINTS_SIZES = (16384, 16385)  # kNormalsChunk and one point beyond: a last chunk of one point
TILES = {"default": 2176, "wg4": 1408, "probe4": 2176, "normals": 1728, "train": 1280, "normals_probe3": 1728, "train_probe3": 1280}
# test_other_hand_geometries_bit_exact's general-probe geometry (the kLutProbe instantiations): three thresholds in its fullest
# look-up cell, not four (tests/hand_geometries.py: three_a)
PROBE4 = dict(finger_width=0.01, hand_outer_diameter=0.1)
PROBE4_KINDS = ("probe4", "normals_probe3", "train_probe3")
SAMPLE_COUNTS = (1, 7, 9, 127, 128, 4095, 4096, 4097, 65536, 65537)
MIRROR_COUNTS = (65536, 65537)  # hypotheses: the pinned host mirror's room and one beyond
HANDLE_COUNTS = (640, 641, 1024, 1025, 4096, 4097, 8192)
HANDLE_SEEDS = ((600, 64), (600, 65), (1500, 64), (1500, 65), (3000, 2048), (3000, 2049))  # (H, inliers of one seed)
# rows around kMaxRow (k_handle_batch declines beyond) in the LDS variant (H <= 640) and the general one: (H, big)
HANDLE_ROWS = tuple((H, big) for H in (600, 1500) for big in (127, 128, 129))


def _row_shapes():
    """(H, big, options of handle_row_hands): rows of 128 (the longest k_handle_batch takes) and of 100 hands, in two slots per
    lane.  A gap at the last lanes of the first slot, across the slots, at the first lane of the second, before the row's last
    hand (big - 2: the clamped read at position 127 for big = 128) and at position 100 of the full row; ties across the slots;
    and rows with more than 64 potential members of which fewer than 64 are alive."""
    out = []
    for H in (600, 1500):
        for big in (128, 100):
            gaps = (62, 63, 64, big - 2) + ((100,) if big == 128 else ())
            out += [(H, big, dict(gap_after=g)) for g in gaps]
            out.append((H, big, dict(ties=4)))
            out.append((H, big, dict(dead=big - 58 if big == 128 else big - 60)))
    return tuple(out)


HANDLE_ROW_SHAPES = _row_shapes()


def row_shape_id(case):
    H, big, opt = case
    return f"{H}-{big}-" + "-".join(f"{k}{v}" for k, v in opt.items())


def row_shape_hands(case):
    H, big, opt = case
    return handle_row_hands(H, big, seed=H + big, **opt)


def tile_targets(T):
    return (T - 1, T, T + 1, 2 * T, 2 * T + 1)


def rand50_cloud(seed=5):
    """RAND50_EDGE, then 24 ordinary samples (60-400 neighbours): a wrong draw offset shifts every later sample."""
    rng = np.random.default_rng(seed)
    return ball_cloud(list(RAND50_EDGE) + list(rng.integers(60, 400, 24)), 0.03, seed=seed, filler=300)


def tile_cloud(kind):
    """The crop cases of one sweep tile: (xyz, cam, samples, geometry, frames)."""
    T = TILES[kind]
    geom = PROBE4 if kind in PROBE4_KINDS else {}
    xyz, cam, s, fr = crop_cloud(tile_targets(T), geom, seed=len(kind), pad_samples=4100 if kind == "wg4" else 0)
    return xyz, cam, s, geom, fr
