"""Depth-image captures for the agh_localize_depth* tests, and numpy models of what the library does with them (numpy only).

An image is a dict as agile_grasp_amd.binding.depth_image_records takes it: `data` ((H, W) uint16 or float32, rows possibly
padded), fx, fy, cx, cy, `pose` (3 x 4, camera optical frame -> cloud frame) and depth_scale.

  deproject_ref     the arithmetic contract of include/agh.h in np.float32
  render_depth      a camera's view of a synthetic.make_raw_cloud scene as a depth image
  voxel_model       the per-camera unique voxels of the deprojected cloud, camera id = image index
  main_case / edge_cases   the captures the tests run
"""
import numpy as np

from agile_grasp_amd import synthetic

U16, F32 = np.uint16, np.float32
SCALE = 0.001
# 320 x 240 at a focal length of 260 px: 2.7 mm per pixel at 0.7 m, about the 3 mm voxel
MAIN_W, MAIN_H, MAIN_F = 320, 240, 260.0


def scene_pose(cam: int) -> np.ndarray:
    """synthetic.camera_poses()[cam] taken into the (tilted) scene frame: 3 x 4 [R|t], camera frame -> scene frame."""
    tf = synthetic.camera_poses()[cam]
    rot = synthetic._tilt() @ tf[:3, :3]
    t = synthetic.to_scene_frame(tf[:3, 3][None, :])[0]
    return np.concatenate([rot, t[:, None]], axis=1)


def intrinsics(w: int, h: int, f: float = MAIN_F) -> dict:
    return dict(fx=f, fy=f * 1.01, cx=(w - 1) / 2 + 0.3, cy=(h - 1) / 2 - 0.2)


def padded(a: np.ndarray, pad: int) -> np.ndarray:
    """The same pixels in rows `pad` elements longer (the padding holds a value no test expects to see)."""
    wide = np.full((a.shape[0], a.shape[1] + pad), 7 if a.dtype == U16 else 7.0, a.dtype)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]]


def render_depth(xyz: np.ndarray, cam: int, w: int, h: int, fmt=U16, f: float = MAIN_F, pad: int = 0) -> dict:
    """Splat the scene-frame points `xyz` into camera `cam`'s nearest-depth buffer, quantised to the format (uint16 units of
    SCALE metres, or float32 metres); pixels no point falls into stay 0 (no reading)."""
    pose = scene_pose(cam)
    k = intrinsics(w, h, f)
    p = xyz[np.isfinite(xyz).all(1)].astype(np.float64)
    pc = (p - pose[:, 3]) @ pose[:, :3]  # R^T (p - t)
    pc = pc[pc[:, 2] > 0.05]
    u = np.rint(k["fx"] * pc[:, 0] / pc[:, 2] + k["cx"]).astype(np.int64)
    v = np.rint(k["fy"] * pc[:, 1] / pc[:, 2] + k["cy"]).astype(np.int64)
    ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    z = np.full(h * w, np.inf)
    np.minimum.at(z, v[ok] * w + u[ok], pc[ok, 2])
    z = z.reshape(h, w)
    hit = np.isfinite(z)
    if fmt == U16:
        data = np.where(hit, np.clip(np.rint(np.where(hit, z, 0.0) / SCALE), 1, 65535), 0).astype(U16)
    else:
        data = np.where(hit, z, 0.0).astype(F32)
    return dict(data=padded(data, pad) if pad else np.ascontiguousarray(data), pose=pose, depth_scale=SCALE, **k)


def deproject_ref(images) -> np.ndarray:
    """The contract of include/agh.h, all float32, left to right: (sum W x H, 3), image 0 first, pixels row-major."""
    out = []
    for im in images:
        d = im["data"]
        h, w = d.shape
        kx, ky = F32(1.0 / im["fx"]), F32(1.0 / im["fy"])
        cx, cy = F32(im["cx"]), F32(im["cy"])
        p = np.asarray(im["pose"], np.float64).reshape(12).astype(F32)
        with np.errstate(all="ignore"):
            if d.dtype == U16:
                z = d.astype(F32) * F32(im.get("depth_scale", SCALE))
                ok = d != 0
            else:
                z = np.array(d, F32)
                ok = (z > 0) & (z < np.inf)
            u = np.arange(w, dtype=F32)[None, :]
            v = np.arange(h, dtype=F32)[:, None]
            x = ((u - cx) * z) * kx
            y = ((v - cy) * z) * ky
            rows = [((p[4 * r] * x + p[4 * r + 1] * y) + p[4 * r + 2] * z) + p[4 * r + 3] for r in range(3)]
        pts = np.stack(rows, axis=-1)
        assert pts.dtype == F32
        pts[~ok] = np.nan
        out.append(pts.reshape(-1, 3))
    return np.concatenate(out)


def deproject_f64(images) -> np.ndarray:
    """The same formulas in float64, rounded once at the end: what "bit for bit" is NOT."""
    out = []
    for im in images:
        d = im["data"]
        h, w = d.shape
        p = np.asarray(im["pose"], np.float64).reshape(12)
        z = d.astype(np.float64) * (np.float64(F32(im.get("depth_scale", SCALE))) if d.dtype == U16 else 1.0)
        ok = (d != 0) if d.dtype == U16 else ((z > 0) & (z < np.inf))
        u = np.arange(w, dtype=np.float64)[None, :]
        v = np.arange(h, dtype=np.float64)[:, None]
        with np.errstate(all="ignore"):
            x = (u - im["cx"]) * z / im["fx"]
            y = (v - im["cy"]) * z / im["fy"]
            pts = np.stack([p[4 * r] * x + p[4 * r + 1] * y + p[4 * r + 2] * z + p[4 * r + 3] for r in range(3)], axis=-1)
        pts[~ok] = np.nan
        out.append(pts.reshape(-1, 3).astype(F32))
    return np.concatenate(out)


def image_index(images) -> np.ndarray:
    """camera id per deprojected point: its image's index"""
    return np.concatenate([np.full(im["data"].size, k, np.int32) for k, im in enumerate(images)])


def voxel_model(points: np.ndarray, cams: np.ndarray, workspace, cell: float = 0.003):
    """The voxelised cloud of the points with camera ids `cams` (localization.cpp:216-355 as tests/test_cpp_adapter.py restates
    it): workspace box (false for NaN), then per camera the unique voxels in lexicographic order, camera 0 block first."""
    ws = np.asarray(workspace, np.float64)
    p = np.asarray(points, F32)
    with np.errstate(invalid="ignore"):
        inb = ((p[:, 0] >= ws[0]) & (p[:, 0] <= ws[1]) & (p[:, 1] >= ws[2]) & (p[:, 1] <= ws[3]) & (p[:, 2] >= ws[4])
               & (p[:, 2] <= ws[5]))
    out, out_cam = [], []
    for c in (0, 1):
        q = p[inb & (cams == c)]
        if len(q) == 0:
            continue
        mn = q.min(0).astype(np.float64)
        vox = np.unique(np.floor((q.astype(np.float64) - mn) / cell).astype(np.int64), axis=0)
        out.append((vox.astype(np.float64) * cell + 1.0 * mn).astype(F32))
        out_cam.append(np.full(len(vox), c, np.int32))
    return np.concatenate(out), np.concatenate(out_cam)


def rank_labels(points: np.ndarray, size_left: int) -> np.ndarray:
    """What dense = 0 would label the points: camera = (rank among the finite points >= size_left), the reference's ids after
    pcl::removeNaNFromPointCloud without re-indexing.  -1 for the removed points."""
    ok = np.isfinite(points).all(1)
    lab = np.full(len(points), -1, np.int32)
    lab[ok] = (np.arange(int(ok.sum())) >= size_left).astype(np.int32)
    return lab


_MAIN = {}


def main_case(w: int = MAIN_W, h: int = MAIN_H, f: float = MAIN_F, seed: int = 31, n_points: int = 600_000):
    """Two U16 views of a raw-cloud scene with padded rows: (images, workspace, camera origins).  Cached, read-only."""
    key = (w, h, f, seed, n_points)
    if key not in _MAIN:
        raw = synthetic.make_raw_cloud(n_points, seed, nan_frac=0.0, n_objects=6)
        views = (raw.xyz[:raw.size_left], raw.xyz[raw.size_left:])
        images = [render_depth(views[k], k, w, h, U16, f, pad=4 + 3 * k) for k in range(2)]
        for im in images:
            im["data"].setflags(write=False)
        origins = np.stack([im["pose"][:, 3] for im in images])
        _MAIN[key] = (images, raw.workspace.copy(), origins)
    return _MAIN[key]


def _random_image(rng, w, h, fmt, cam=0, pad=0, zero_frac=0.2):
    z = rng.uniform(0.4, 1.5, (h, w))
    if fmt == U16:
        d = np.rint(z / SCALE).astype(U16)
    else:
        d = z.astype(F32)
    d[rng.random((h, w)) < zero_frac] = 0
    return dict(data=padded(d, pad) if pad else d, pose=scene_pose(cam), depth_scale=SCALE, **intrinsics(w, h, 0.8 * max(w, h) + 3.0))


def edge_cases() -> dict:
    """name -> images: the sizes and layouts at which k_deproject takes another path."""
    rng = np.random.default_rng(77)
    cases = {}
    for w, h in ((1, 1), (63, 3), (65, 2), (257, 1)):  # widths that are no multiple of the lane's run of 4
        cases[f"u16_{w}x{h}"] = [_random_image(rng, w, h, U16)]
        cases[f"f32_{w}x{h}"] = [_random_image(rng, w, h, F32, cam=1)]
    # a U16 row stride that is an odd multiple of 2 bytes (65 elements): every other row starts off a 4-byte boundary
    cases["u16_odd_stride"] = [_random_image(rng, 63, 6, U16, pad=2), _random_image(rng, 64, 5, U16, cam=1, pad=1)]
    cases["f32_padded"] = [_random_image(rng, 64, 5, F32, pad=1), _random_image(rng, 30, 7, F32, cam=1, pad=3)]
    # totals of 1023, 1024 and 1025 pixels; image 1's points start at 511, 512 and 513
    for name, (w0, h0) in (("total_1023", (73, 7)), ("total_1024", (64, 8)), ("total_1025", (27, 19))):
        cases[name] = [_random_image(rng, w0, h0, U16), _random_image(rng, 64, 8, F32, cam=1)]
    special = _random_image(rng, 16, 4, F32, zero_frac=0.0)
    special["data"][0, :8] = [0.0, -0.7, np.nan, np.inf, 1e-40, -np.inf, -0.0, np.float32(1e-45)]
    special["data"][2, 5:9] = [np.inf, 0.9, np.nan, 1e-39]
    cases["f32_special_values"] = [special]
    # the same values where the runs take the element loads: 7-pixel rows (28 bytes: rows 1 to 3 off a 16-byte boundary, a tail
    # run of 3 in every row)
    odd = _random_image(rng, 7, 4, F32, cam=1, zero_frac=0.0)
    odd["data"][1, :] = [0.0, -0.7, np.nan, np.inf, 1e-40, -np.inf, np.float32(1e-45)]
    odd["data"][2, 4:] = [np.nan, 1e-39, np.inf]
    cases["f32_special_unaligned"] = [odd]
    cases["u16_extremes"] = [dict(_random_image(rng, 9, 2, U16), depth_scale=0.00025)]
    cases["u16_extremes"][0]["data"][0, :3] = [65535, 1, 0]
    cases["one_image"] = [main_case()[0][0]]
    cases["main"] = list(main_case()[0])
    return cases
