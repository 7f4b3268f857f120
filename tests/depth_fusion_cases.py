"""agh_fuse_depth's contract (include/agh.h, "DEPTH FUSION", rules 1 to 7) as a numpy model -- integer arithmetic for uint16,
np.float32 operations in the stated order for float32 -- with a seeded burst generator over tests/hand_filter_cases.box_scene
(noise, drop-outs, weak pixels, edge flips and flying edge pixels), random bursts for the launch boundaries, and one constructed
image in which every pixel is a case."""
import numpy as np

from tests import depth_captures as D
from tests import hand_filter_cases as HF

DEFAULTS = dict(min_valid=2, max_spread_abs=0.005, max_spread_rel=0.005)
EMPTY, UNSUPPORTED, INCONSISTENT, FUSED = 0, 1, 2, 3
COUNT_FIELDS = ("n_pixels", "n_empty", "n_unsupported", "n_inconsistent", "n_fused", "n_filled")
NO_READING = np.uint32(0xFFFFFFFF)


def params(**fields) -> dict:
    assert all(k in DEFAULTS for k in fields), fields
    return dict(DEFAULTS, **fields)


def valid_mask(stack: np.ndarray) -> np.ndarray:
    """rule 1 on a (T, H, W) stack"""
    if stack.dtype == np.uint16:
        return stack != 0
    with np.errstate(invalid="ignore"):
        return (stack > 0) & (stack < np.inf)


def fuse(frames, depth_scale: float = D.SCALE, **fields) -> dict:
    """`frames`: the burst's (H, W) arrays, all uint16 or all float32, in frame order.  Returns image (what the slot holds), cls
    (the class per pixel), counts (COUNT_FIELDS order), and the intermediate m, k, member (T, H, W), tol, zm for the tests."""
    fp = params(**fields)
    stack = np.stack([np.asarray(f) for f in frames])
    T = stack.shape[0]
    assert 1 <= T <= 16 and stack.dtype in (np.uint16, np.float32)
    u16 = stack.dtype == np.uint16
    sa, sr, scale = np.float32(fp["max_spread_abs"]), np.float32(fp["max_spread_rel"]), np.float32(depth_scale)
    ok = valid_mask(stack)
    m = ok.sum(0)
    keys = np.where(ok, stack.astype(np.uint32) if u16 else np.ascontiguousarray(stack).view(np.uint32), NO_READING)
    order = np.sort(keys, axis=0)  # (positive floats order as their bits do)
    med = np.take_along_axis(order, (np.maximum(m, 1) - 1)[None] // 2, axis=0)[0]
    with np.errstate(all="ignore"):
        z = stack.astype(np.float32) * scale if u16 else stack
        zm = med.astype(np.float32) * scale if u16 else med.view(np.float32)
        tol = sa + (sr * zm)
        member = ok & (np.abs(z - zm[None]) <= tol[None])
        k = member.sum(0)
        cls = np.where(m == 0, EMPTY, np.where(m < fp["min_valid"], UNSUPPORTED, np.where(k < fp["min_valid"], INCONSISTENT, FUSED)))
        if u16:
            total = np.where(member, stack, 0).astype(np.uint32).sum(0, dtype=np.uint32)
            kk = np.maximum(k, 1).astype(np.uint32)
            image = np.where(cls == FUSED, (total + kk // 2) // kk, 0).astype(np.uint16)
        else:
            s = np.zeros(stack.shape[1:], np.float32)
            seen = np.zeros(stack.shape[1:], bool)
            for t in range(T):  # frame order: the first member, then s = s + z
                s = np.where(member[t], np.where(seen, s + stack[t], stack[t]), s).astype(np.float32)
                seen |= member[t]
            image = np.where(cls == FUSED, s / np.maximum(k, 1).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    filled = (cls == FUSED) & ~ok[-1]
    counts = [int(m.size)] + [int((cls == c).sum()) for c in (EMPTY, UNSUPPORTED, INCONSISTENT, FUSED)] + [int(filled.sum())]
    return dict(image=image, cls=cls, counts=counts, m=m, k=k, member=member, tol=tol, zm=zm, filled=filled)


def same_image(a: np.ndarray, b: np.ndarray) -> bool:
    """bytes, not values: a float32 image's NaNs compare"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))
    return bool(np.array_equal(a, b))


# ---- a burst of a fixed camera over the box scene ----
def burst(image: dict, n_frames: int = 8, seed: int = 1, noise: float = 2.0, drop: float = 0.10, weak: float = 0.005,
          weak_drop: float = 0.8, flip: float = 0.15, flying: float = 0.10, edge_jump: int = 20) -> dict:
    """`image`: one clean uint16 view of box_scene.  Per frame: Gaussian noise of `noise` raw units on every reading; independent
    drop-outs with probability `drop`, and `weak_drop` on the `weak` share of pixels with a weak return; along depth edges (a
    4-neighbour more than edge_jump units away) a reading flips to that neighbour's surface with probability `flip`, and on the
    `flying` share of edge pixels every reading lies somewhere between the two surfaces.  Returns frames (image dicts with the
    clean one's intrinsics and pose), clean, and flipped (H, W): the pixels some frame took off their own surface."""
    clean = np.array(image["data"])
    assert clean.dtype == np.uint16
    rng = np.random.default_rng(seed)
    h, w = clean.shape
    c = clean.astype(np.int64)
    other = c.copy()
    edge = np.zeros((h, w), bool)
    for dv, du in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        nb = np.roll(c, (dv, du), (0, 1))
        inside = np.ones((h, w), bool)
        if dv:
            inside[0 if dv > 0 else -1, :] = False
        if du:
            inside[:, 0 if du > 0 else -1] = False
        jump = inside & (c > 0) & (nb > 0) & (np.abs(nb - c) > edge_jump) & ~edge
        other[jump] = nb[jump]
        edge |= jump
    weak_px = rng.random((h, w)) < weak
    flying_px = edge & (rng.random((h, w)) < flying)
    frames, flipped = [], np.zeros((h, w), bool)
    for _ in range(n_frames):
        z = c + np.rint(rng.normal(0.0, noise, (h, w))).astype(np.int64)
        flips = edge & ~flying_px & (rng.random((h, w)) < flip)
        z[flips] = (other + np.rint(rng.normal(0.0, noise, (h, w))).astype(np.int64))[flips]
        mix = rng.random((h, w))
        z[flying_px] = np.rint(c + mix * (other - c))[flying_px].astype(np.int64)
        flipped |= flips | flying_px
        gone = (c == 0) | (rng.random((h, w)) < np.where(weak_px, weak_drop, drop))
        data = np.where(gone, 0, np.clip(z, 1, 65535)).astype(np.uint16)
        frames.append(dict(image, data=data))
    return dict(frames=frames, clean=clean, flipped=flipped)


_BURSTS = {}


def box_bursts(n_frames: int = 8, w: int = HF.W, h: int = HF.H, f: float = HF.F) -> list:
    """the bursts of box_scene(2)'s two views, cached and read-only"""
    key = (n_frames, w, h, f)
    if key not in _BURSTS:
        sc = HF.box_scene(2, w=w, h=h, f=f)
        _BURSTS[key] = [burst(im, n_frames, seed=11 + cam) for cam, im in enumerate(sc["images"])]
        for b in _BURSTS[key]:
            for fr in b["frames"]:
                fr["data"].setflags(write=False)
    return _BURSTS[key]


# ---- random bursts at the launch's boundaries ----
SIZES = ((1, 1), (63, 1), (64, 1), (65, 3), (130, 2), (257, 5))
FRAME_COUNTS = (1, 2, 3, 4, 5, 8, 15, 16)


def random_burst(w: int, h: int, n_frames: int, fmt, seed: int, pad: int = 0) -> list:
    """about 20 % invalid readings, noise inside the default spread, a tenth of the readings 5 cm behind; frame t's rows are
    pad + t elements longer than the image when pad is set"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.4, 1.5, (h, w))
    frames = []
    for t in range(n_frames):
        z = base + rng.normal(0.0, 0.002, (h, w)) + np.where(rng.random((h, w)) < 0.1, 0.05, 0.0)
        d = np.rint(z / D.SCALE).astype(np.uint16) if fmt == D.U16 else z.astype(np.float32)
        d[rng.random((h, w)) < 0.2] = 0
        frames.append(dict(data=D.padded(d, pad + t) if pad else d, pose=D.scene_pose(0), depth_scale=D.SCALE, **D.intrinsics(w, h, 100.0)))
    return frames


# ---- one image, every pixel a case ----
def constructed(fmt):
    """(frames, params, cases): 8 frames of a one-row image.  cases: name -> (pixel, expected class, expected value or None).
    min_valid 3 and spreads that are exact in binary, so that "at the tolerance" is a fact and not a rounding: uint16 with
    depth_scale 2^-10 and a spread of two raw units, float32 with a spread of 0.25."""
    T, MV = 8, 3
    u16 = fmt == D.U16
    cols = []
    cases = {}

    def add(name, readings, cls, value=None):
        assert len(readings) == T
        cases[name] = (len(cols), cls, value)
        cols.append(readings)

    if u16:
        scale = 1.0 / 1024
        fp = dict(min_valid=MV, max_spread_abs=2.0 / 1024, max_spread_rel=0.0)
        a, far = 1000, 1500
        add("no frame valid", [0] * T, EMPTY, 0)
        add("min_valid - 1 valid", [a, a] + [0] * 6, UNSUPPORTED, 0)
        add("exactly min_valid valid", [a, a, a + 1] + [0] * 5, FUSED, a)
        add("consensus one short", [a, far, far + 1, far + 40, far + 80] + [0] * 3, INCONSISTENT, 0)  # (median far + 1: two members)
        add("two equal clusters", [a, far, a, far, a, far, a, far], FUSED, a)  # (lower median: the nearer surface)
        add("members 1 and 2", [1, 2, 1, 2] + [0] * 4, FUSED, 2)  # ((6 + 2) / 4 = 2: half rounds up; median 1, both within the spread)
        add("all 65535", [65535] * T, FUSED, 65535)
        add("raw 1", [1] * T, FUSED, 1)
        add("last frame invalid", [a] * 7 + [0], FUSED, a)
        add("last frame valid", [0] + [a] * 7, FUSED, a)
        add("at tolerance", [a, a, a, a + 2, a + 2] + [0] * 3, FUSED, a + 1)  # ((5a + 4 + 2) / 5)
        add("beyond tolerance", [a, a, a, a + 3, a + 3] + [0] * 3, FUSED, a)
    else:
        scale = D.SCALE
        fp = dict(min_valid=MV, max_spread_abs=0.25, max_spread_rel=0.0)
        f = np.float32
        a, far = f(1.0), f(2.0)
        nan, inf, den = f(np.nan), f(np.inf), f(1e-40)
        beyond = np.nextafter(f(1.25), f(2.0))
        add("no frame valid", [nan, inf, f(-1.0), f(0.0), f(-0.0), -inf, nan, f(0.0)], EMPTY)
        add("min_valid - 1 valid", [a, a, nan, inf, f(-1.0), f(0.0), f(-0.0), nan], UNSUPPORTED)
        add("exactly min_valid valid", [a, nan, a, inf, a, f(-1.0), f(0.0), f(-0.0)], FUSED, a)
        add("consensus one short", [a, far, f(2.25), f(2.75), f(3.5), nan, nan, nan], INCONSISTENT)  # (median 2.25: two members)
        add("two equal clusters", [a, far, a, far, a, far, a, far], FUSED, a)
        add("denormals", [den] * 4 + [nan] * 4, FUSED, den)
        add("last frame invalid", [a] * 7 + [nan], FUSED, a)
        add("last frame valid", [nan] + [a] * 7, FUSED, a)
        add("at tolerance", [a, a, a, f(1.25), f(1.25), nan, nan, nan], FUSED, f(1.1))
        add("beyond tolerance", [a, a, a, beyond, beyond, nan, nan, nan], FUSED, a)
    data = np.array(cols, fmt).T.reshape(T, 1, len(cols))
    frames = [dict(data=np.ascontiguousarray(data[t]), pose=D.scene_pose(0), depth_scale=scale, **D.intrinsics(len(cols), 1, 100.0))
              for t in range(T)]
    return frames, fp, cases


def zero_spread(fmt):
    """(frames, params): spreads 0, min_valid 1 -- the consensus is the readings equal to the median, the result the median"""
    if fmt == D.U16:
        cols = [[5, 1, 9, 7, 3], [4, 4, 8, 4, 0], [0, 0, 6, 0, 2]]
    else:
        cols = [[5.0, 1.25, 9.0, 7.0, 3.0], [4.0, 4.0, 8.0, 4.0, np.nan], [np.nan, np.inf, 6.0, 0.0, 2.0]]
    data = np.array(cols, fmt).T.reshape(5, 1, 3)
    frames = [dict(data=np.ascontiguousarray(data[t]), pose=D.scene_pose(0), depth_scale=D.SCALE, **D.intrinsics(3, 1, 100.0)) for t in range(5)]
    return frames, dict(min_valid=1, max_spread_abs=0.0, max_spread_rel=0.0), np.array([[5, 4, 2]], fmt)


def order_of_the_sum():
    """(frames, params, value): float32 members whose sum depends on the order -- 1e8f first swallows every 1.0f that follows
    (1e8f + 1.0f == 1e8f), while 1.0f seven times and then 1e8f gives 1e8f + 8 -- with a spread that takes them all in"""
    f = np.float32
    cols = [[f(1e8)] + [f(1.0)] * 7, [f(1.0)] * 7 + [f(1e8)]]
    data = np.array(cols, f).T.reshape(8, 1, 2)
    frames = [dict(data=np.ascontiguousarray(data[t]), pose=D.scene_pose(0), depth_scale=D.SCALE, **D.intrinsics(2, 1, 100.0)) for t in range(8)]
    first = f(1e8) / f(8.0)
    s = f(7.0) + f(1e8)
    return frames, dict(min_valid=1, max_spread_abs=1e9, max_spread_rel=0.0), np.array([[first, s / f(8.0)]], f)
