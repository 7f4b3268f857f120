"""The depth filter of include/agh.h (agh_set_depth_filter) as a float32 numpy model, and the captures its tests run (numpy only).

  params            the filter's record as a dict (the defaults of agh_default_depth_filter_params, then the given fields)
  filter_image      one image through the four steps of the contract: keep mask, counts, the in-range set, the support
  filter_points     a capture: what agh_deproject writes with the filter set, and the counts per view
  cases             name -> dict(images, fp, check): check(case) asserts, ON THE MODEL, that the case exercises what its name says
  injected_main     depth_captures.main_case() with flying pixels pulled 15 cm towards the camera

Every case is a condition on the inputs; the library is compared with the model elsewhere (tests/test_gpu_depth_filter.py).
"""
import numpy as np

from tests import depth_captures as DC

U16, F32 = DC.U16, DC.F32
COUNT_NAMES = ("n_valid", "n_out_of_range", "n_unsupported", "n_kept")
TILE_W, TILE_H = 64, 16  # k_deproject_filtered's tile: the seams the cases aim at


def params(**fields) -> dict:
    fp = dict(radius=1, min_support=3, max_jump_abs=0.01, max_jump_rel=0.01, z_min=0.0, z_max=float("inf"))
    for k in fields:
        assert k in fp, k
    fp.update(fields)
    return fp


def rounded(fp):
    """ja, jr, zlo, zhi: the four doubles rounded once to float32"""
    with np.errstate(over="ignore"):
        return F32(fp["max_jump_abs"]), F32(fp["max_jump_rel"]), F32(fp["z_min"]), F32(fp["z_max"])


def filter_image(im, fp) -> dict:
    """Steps 1 to 4 for one image: z and valid (k_deproject's), inr, tol, support (int, counted on the in-range set; 0 where the
    centre is not in range), keep, counts (COUNT_NAMES order)."""
    d = im["data"]
    h, w = d.shape
    r = int(fp["radius"])
    ja, jr, zlo, zhi = rounded(fp)
    with np.errstate(all="ignore"):
        if d.dtype == U16:
            z = d.astype(F32) * F32(im.get("depth_scale", DC.SCALE))
            valid = d != 0
        else:
            z = np.array(d, F32)
            valid = (z > 0) & (z < np.inf)
        inr = valid & (z >= zlo) & (z <= zhi)
        tol = ja + (jr * z)
        assert z.dtype == F32 and tol.dtype == F32
        zn = np.full((h + 2 * r, w + 2 * r), np.nan, F32)  # pixels outside the image never support
        zn[r:r + h, r:r + w] = np.where(inr, z, F32(np.nan))
        support = np.zeros((h, w), np.int32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy or dx:
                    q = zn[r + dy:r + dy + h, r + dx:r + dx + w]
                    diff = np.abs(q - z)
                    assert diff.dtype == F32
                    support += diff <= tol
    support[~inr] = 0
    keep = inr & (support >= int(fp["min_support"]))
    counts = np.array([valid.sum(), (valid & ~inr).sum(), (inr & ~keep).sum(), keep.sum()], np.int64)
    return dict(z=z, valid=valid, inr=inr, tol=tol, support=support, keep=keep, counts=counts)


def filter_points(images, fp):
    """(points, counts): deproject_ref's points with every pixel the filter does not keep set to NaN, (sum W x H, 3) float32, and
    the (n_images, 4) counts."""
    pts = DC.deproject_ref(images)
    res = [filter_image(im, fp) for im in images]
    keep = np.concatenate([m["keep"].reshape(-1) for m in res])
    pts[~keep] = np.nan
    return pts, np.stack([m["counts"] for m in res])


def _image(data, cam=0, pad=0):
    h, w = data.shape
    return dict(data=DC.padded(data, pad) if pad else np.ascontiguousarray(data), pose=DC.scene_pose(cam), depth_scale=DC.SCALE,
                **DC.intrinsics(w, h, 0.8 * max(w, h) + 3.0))


def surface_image(rng, w, h, fmt, cam=0, pad=0):
    """A slanted surface with noise of about the tolerance, a fifth of the pixels without a reading and a few far outliers: kept,
    unsupported and invalid pixels side by side."""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    z = 0.8 + 0.002 * u + 0.003 * v + rng.uniform(-0.012, 0.012, (h, w))
    z[rng.random((h, w)) < 0.05] += 0.4
    d = np.rint(z / DC.SCALE).astype(U16) if fmt == U16 else z.astype(F32)
    d[rng.random((h, w)) < 0.2] = 0
    return _image(d, cam, pad)


SIZES = ((1, 1), (63, 3), (65, 2), (257, 1), (64, 16), (65, 17), (128, 33))


def settings(radius):
    """min_support at 1, at 3 and at (2 r + 1)^2 - 1"""
    return [(radius, ms) for ms in (1, 3, (2 * radius + 1) ** 2 - 1)]


def _check_mixed(case):
    # (what the surface images are for: both outcomes, and both reasons for a rejection where the range is narrowed)
    tot = sum(filter_image(im, case["fp"])["counts"] for im in case["images"])
    npix = sum(im["data"].size for im in case["images"])
    assert tot[0] == tot[1] + tot[2] + tot[3]
    if npix >= 64:
        assert tot[0] < npix and tot[2] > 0, tot
        if case["fp"]["min_support"] <= 3 and min(im["data"].shape[0] for im in case["images"]) >= 3:
            assert tot[3] > 0, tot
        if case["fp"]["z_min"] > 0:
            assert tot[1] > 0, tot


def _size_cases(cases):
    rng = np.random.default_rng(2024)
    combos = settings(1) + settings(2)
    k = 0
    for w, h in SIZES:
        for fmt, name in ((U16, "u16"), (F32, "f32")):
            # the two largest sizes take every setting, the others one each in turn
            for r, ms in (combos if (w, h) in ((65, 17), (128, 33)) else [combos[k % len(combos)]]):
                fp = params(radius=r, min_support=ms, z_min=0.85 if k % 2 else 0.0, z_max=1.3 if k % 3 == 0 else float("inf"))
                cases[f"{name}_{w}x{h}_r{r}_s{ms}"] = dict(images=[surface_image(rng, w, h, fmt, cam=k % 2)], fp=fp, check=_check_mixed)
                k += 1
    # padded rows, and a U16 row stride that is an odd number of elements (every other row off a 4-byte boundary)
    cases["u16_odd_stride"] = dict(images=[surface_image(rng, 63, 18, U16, pad=2), surface_image(rng, 64, 5, U16, cam=1, pad=1)],
                                   fp=params(), check=_check_mixed)
    cases["f32_padded"] = dict(images=[surface_image(rng, 64, 17, F32, pad=1), surface_image(rng, 30, 7, F32, cam=1, pad=3)],
                               fp=params(radius=2, min_support=5), check=_check_mixed)
    assert cases["u16_odd_stride"]["images"][0]["data"].strides[0] == 65 * 2


def _seam_case(radius, fmt):
    """Pixels in columns 63 / 64 and rows 15 / 16 whose ONLY supporters lie in the neighbouring tile: min_support of them (kept),
    or one fewer (rejected).  The background has no reading."""
    w, h, ms = 2 * TILE_W + 2, 2 * TILE_H + 2, 3
    d = np.zeros((h, w), F32)
    marks = []  # (y, x, expected keep, the supporters)

    def place(y, x, cand, n):
        d[y, x] = 1.0
        sup = cand[:n]
        for (yy, xx) in sup:
            d[yy, xx] = 1.004
        marks.append((y, x, n >= ms, sup))

    for j, n in enumerate((ms, ms - 1)):
        # the vertical seam 63 | 64 (and 127 | 128): the centre left of it, the supporters right of it, and the other way round
        for seam in (TILE_W, 2 * TILE_W):
            y = 4 + 8 * j + (seam // TILE_W - 1) * TILE_H
            place(y, seam - 1, [(y + dy, seam + k) for k in range(radius) for dy in (0, -1, 1)], n)
            y += 4
            place(y, seam, [(y + dy, seam - 1 - k) for k in range(radius) for dy in (0, -1, 1)], n)
        # the horizontal seam 15 | 16 (and 31 | 32)
        for seam in (TILE_H, 2 * TILE_H):
            x = 8 + 16 * j + (seam // TILE_H - 1) * TILE_W
            place(seam - 1, x, [(seam + k, x + dx) for k in range(radius) for dx in (0, -1, 1)], n)
            x += 8
            place(seam, x, [(seam - 1 - k, x + dx) for k in range(radius) for dx in (0, -1, 1)], n)
    data = np.rint(d / DC.SCALE).astype(U16) if fmt == U16 else d

    def check(case):
        m = filter_image(case["images"][0], case["fp"])
        assert len(marks) == 16
        for y, x, kept, sup in marks:
            assert m["keep"][y, x] == kept and m["support"][y, x] == len(sup), (y, x)
            # every supporter lies in another tile than the centre
            assert all((yy // TILE_H, xx // TILE_W) != (y // TILE_H, x // TILE_W) for yy, xx in sup), (y, x)
        assert sum(1 for mk in marks if mk[2]) == 8

    return dict(images=[_image(data)], fp=params(radius=radius, min_support=ms), check=check)


def _border_case(ms):
    """A constant image of 65 x 17: a corner has 3 neighbours, a border pixel 5, an inner one 8 (radius 1)."""
    d = np.full((17, 65), 0.9, F32)

    def check(case):
        keep = filter_image(case["images"][0], case["fp"])["keep"]
        sup = filter_image(case["images"][0], case["fp"])["support"]
        corners = [(0, 0), (0, 64), (16, 0), (16, 64)]
        assert all(sup[c] == 3 for c in corners) and all(keep[c] == (3 >= ms) for c in corners)
        border = np.ones_like(keep)
        border[1:-1, 1:-1] = False
        for c in corners:
            border[c] = False
        assert (sup[border] == 5).all() and (keep[border] == (5 >= ms)).all()
        assert (sup[1:-1, 1:-1] == 8).all() and keep[1:-1, 1:-1].all()

    return dict(images=[_image(d, cam=1)], fp=params(min_support=ms), check=check)


def _two_image_case():
    """Image 0's last row and image 1's first row hold depths that would support one another if the images were one: each is one
    short of min_support inside its own image."""
    a = np.zeros((6, 40), F32)
    a[5, 0:3] = 1.0        # (5, 1) has 2 supporters in its own image
    b = np.zeros((5, 33), U16)
    b[0, 0:3] = 1000       # (0, 1) likewise; image 0's row above it would add three
    rng = np.random.default_rng(5)
    a[0:3, 8:] = surface_image(rng, 32, 3, F32)["data"]
    b[2:, 3:] = surface_image(rng, 30, 3, U16)["data"]

    def check(case):
        m0, m1 = (filter_image(im, case["fp"]) for im in case["images"])
        assert m0["inr"][5, 0:3].all() and m1["inr"][0, 0:3].all()
        assert m0["support"][5, 1] == 2 and m1["support"][0, 1] == 2 and case["fp"]["min_support"] == 3
        assert not m0["keep"][5].any() and not m1["keep"][0].any()
        # "mutually supporting": the depths are within each other's tolerance
        assert abs(m0["z"][5, 1] - m1["z"][0, 1]) <= min(m0["tol"][5, 1], m1["tol"][0, 1])
        assert m0["keep"].any() and m1["keep"].any()

    return dict(images=[_image(a), _image(b, cam=1, pad=1)], fp=params(), check=check)


SPECIALS = [np.nan, np.inf, -np.inf, -0.7, -0.0, 0.0, 1e-40, float(np.float32(1e-45))]


def _special_case(w, h):
    """NaN, +-inf, negatives, -0.0 and denormals as centre and as neighbour of a constant surface; a run of denormals that support
    one another."""
    d = np.full((h, w), 0.9, F32)
    spots = []
    k = 0
    for y in range(1, h, 3):
        for x in range(1, w, 2):
            if k < len(SPECIALS):
                d[y, x] = SPECIALS[k]
                spots.append((y, x))
                k += 1
    assert k == len(SPECIALS)
    d[h - 1, 0:4] = [1e-40, float(np.float32(1e-45)), 1e-39, 1e-40]
    d[h - 2, 0:4] = [1e-39, 1e-40, 1e-40, 0.0]

    def check(case):
        m = filter_image(case["images"][0], case["fp"])
        for (y, x), s in zip(spots, SPECIALS):
            denormal = 0 < s < 1e-38
            assert m["valid"][y, x] == denormal and m["keep"][y, x] == False  # noqa: E712  (a lone denormal has no support)
            # as a neighbour: the surface pixel beside it is in range, and does not count it
            assert m["inr"][y, x - 1] and m["support"][y, x - 1] < 8
        assert m["keep"][h - 1, 1] and m["support"][h - 1, 1] == 5  # denormals among denormals: the border's five neighbours
        assert m["keep"].sum() > 0 and m["counts"][2] > 0

    return dict(images=[_image(d, cam=1)], fp=params(min_support=4), check=check)


def _boundary_neighbour(zp, tol):
    """the largest float32 z_q >= z_p with fabsf(z_q - z_p) <= tol, in float32"""
    zq = F32(zp + tol)
    while F32(zq - zp) > tol:
        zq = np.nextafter(zq, F32(0))
    while F32(np.nextafter(zq, F32(np.inf)) - zp) <= tol:
        zq = np.nextafter(zq, F32(np.inf))
    return zq


def _tie_case(ja, jr, zp):
    """A neighbour at exactly tol counts; one ulp beyond does not.  Two centres with min_support 3: three neighbours at the
    boundary (kept); two at it and one an ulp beyond (rejected)."""
    zp = F32(zp)
    tol = F32(ja) + (F32(jr) * zp)
    zq = _boundary_neighbour(zp, tol)
    beyond = np.nextafter(zq, F32(np.inf))
    d = np.zeros((3, 9), F32)
    d[1, 1] = d[1, 6] = zp
    d[0, 0:3] = zq
    d[0, 5:7] = zq
    d[0, 7] = beyond

    def check(case):
        m = filter_image(case["images"][0], case["fp"])
        assert m["tol"][1, 1] == tol and F32(zq - zp) <= tol and not (F32(beyond - zp) <= tol)
        if jr == 0:
            assert (zp, zq, tol) == (F32(1.0), F32(1.25), F32(0.25))
        assert m["support"][1, 1] == 3 and m["keep"][1, 1]
        assert m["support"][1, 6] == 2 and not m["keep"][1, 6] and m["inr"][0, 7]

    return dict(images=[_image(d)], fp=params(max_jump_abs=ja, max_jump_rel=jr), check=check)


def _range_case(z_min, z_max):
    """z exactly at z_min and at z_max (rounded to float32) is in range; one ulp outside is not.  The tolerance is wide, so that
    support never decides."""
    zlo, zhi = F32(z_min), F32(z_max)
    d = np.full((4, 12), F32(0.5) * (zlo + zhi), F32)
    d[1, 1], d[1, 4] = zlo, np.nextafter(zlo, F32(0))
    d[2, 7], d[2, 10] = zhi, np.nextafter(zhi, F32(np.inf))

    def check(case):
        m = filter_image(case["images"][0], case["fp"])
        assert m["keep"][1, 1] and m["keep"][2, 7]
        assert m["valid"][1, 4] and not m["inr"][1, 4] and m["valid"][2, 10] and not m["inr"][2, 10]
        assert m["counts"][1] == 2 and m["counts"][2] == 0

    return dict(images=[_image(d, cam=1)], fp=params(min_support=1, max_jump_abs=10.0, z_min=z_min, z_max=z_max), check=check)


_CASES = {}


def cases() -> dict:
    if not _CASES:
        c = {}
        _size_cases(c)
        for r in (1, 2):
            c[f"seams_f32_r{r}"] = _seam_case(r, F32)
            c[f"seams_u16_r{r}"] = _seam_case(r, U16)
        for ms in (3, 4, 5, 6):
            c[f"borders_s{ms}"] = _border_case(ms)
        c["two_images"] = _two_image_case()
        c["f32_special_values"] = _special_case(16, 6)
        c["f32_special_unaligned"] = _special_case(7, 12)
        c["tie_abs"] = _tie_case(0.25, 0.0, 1.0)
        c["tie_rel"] = _tie_case(0.01, 0.01, 0.8)
        c["range_exact"] = _range_case(0.5, 2.0)
        c["range_rounded"] = _range_case(0.3, 1.1)  # (neither is a float32: the host's rounding decides)
        for case in c.values():
            for im in case["images"]:
                im["data"].setflags(write=False)
        _CASES.update(c)
    return _CASES


def batch_captures():
    """Unequal captures of one and two images for agh_deproject_batch: (list of captures, fp)."""
    c = cases()
    names = ("u16_65x17_r1_s3", "two_images", "f32_128x33_r1_s3", "u16_odd_stride", "seams_f32_r1")
    return [c[n]["images"] for n in names], params()


_INJECTED = {}


def injected_main():
    """main_case() with a copy of each image in which every sixth pixel in both directions that the filter keeps and whose raw
    value exceeds 400 is pulled 150 units (15 cm) towards the camera: (images, masks of the injected pixels, workspace, origins,
    fp)."""
    if not _INJECTED:
        images, ws, origins = DC.main_case()
        fp = params()
        out, masks = [], []
        for k, im in enumerate(images):
            d = np.array(im["data"])
            keep = filter_image(im, fp)["keep"]
            grid = np.zeros(d.shape, bool)
            grid[::6, ::6] = True
            inj = grid & keep & (d > 400)
            d[inj] -= 150
            new = dict(im, data=DC.padded(d, 4 + 3 * k))
            new["data"].setflags(write=False)
            out.append(new)
            masks.append(inj)
        _INJECTED["v"] = (out, masks, ws, origins, fp)
    return _INJECTED["v"]
