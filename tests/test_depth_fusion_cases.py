"""The regimes tests/test_gpu_depth_fusion.py relies on, proved on the CPU with the numpy model of tests/depth_fusion_cases.py:
the generated bursts of the box scene's two views reach every class and close the newest frame's holes, and every pixel of the
constructed image lands in the class it was built for.  A regime found empty fails."""
import numpy as np
import pytest

from tests import depth_captures as D
from tests import depth_fusion_cases as FU


@pytest.mark.parametrize("view", [0, 1])
def test_generated_burst_reaches_every_regime(view):
    b = FU.box_bursts()[view]
    assert len(b["frames"]) == 8
    r = FU.fuse([f["data"] for f in b["frames"]], min_valid=3)
    n_pixels, n_empty, n_unsupported, n_inconsistent, n_fused, n_filled = r["counts"]
    print("view", view, dict(zip(FU.COUNT_FIELDS, r["counts"])))
    assert n_pixels == n_empty + n_unsupported + n_inconsistent + n_fused
    assert n_unsupported > 0 and n_inconsistent > 0 and n_filled > 0 and n_fused > 0
    clean, frame0, fused = b["clean"], b["frames"][0]["data"], r["image"]
    seen = clean > 0
    share0, share = ((frame0 == 0) & seen).sum() / seen.sum(), ((fused == 0) & seen).sum() / seen.sum()
    print("invalid among the clean image's valid pixels: frame 0", share0, "fused", share)
    assert share <= share0 / 10
    steady = seen & ~b["flipped"]

    def rms(img):
        on = steady & (img > 0)
        return float(np.sqrt(((img[on].astype(np.float64) - clean[on]) ** 2).mean()))

    print("rms over never-flipped pixels: frame 0", rms(frame0), "fused", rms(fused))
    assert rms(fused) < rms(frame0)


@pytest.mark.parametrize("fmt", [D.U16, D.F32], ids=["u16", "f32"])
def test_constructed_pixels_yield_their_classes(fmt):
    frames, fp, cases = FU.constructed(fmt)
    r = FU.fuse([f["data"] for f in frames], frames[0]["depth_scale"], **fp)
    for name in ("no frame valid", "min_valid - 1 valid", "exactly min_valid valid", "consensus one short", "two equal clusters",
                 "last frame invalid", "at tolerance", "beyond tolerance"):
        assert name in cases
    for name, (px, cls, value) in cases.items():
        assert r["cls"][0, px] == cls, (name, r["cls"][0, px])
        if value is not None:
            assert r["image"][0, px] == value, (name, r["image"][0, px])
    px = cases["min_valid - 1 valid"][0]
    assert r["m"][0, px] == fp["min_valid"] - 1 and r["m"][0, cases["exactly min_valid valid"][0]] == fp["min_valid"]
    px = cases["consensus one short"][0]
    assert r["m"][0, px] >= fp["min_valid"] and r["k"][0, px] == fp["min_valid"] - 1
    assert r["filled"][0, cases["last frame invalid"][0]] and not r["filled"][0, cases["last frame valid"][0]]
    # the reading at the tolerance is in the consensus, the next one beyond it is out
    at, beyond = cases["at tolerance"][0], cases["beyond tolerance"][0]
    data = np.stack([f["data"] for f in frames])[:, 0, :]
    scale = np.float32(frames[0]["depth_scale"])
    z = (lambda v: v.astype(np.float32) * scale) if fmt == D.U16 else (lambda v: v)
    assert np.abs(z(data[3, at]) - r["zm"][0, at]) == r["tol"][0, at] and r["member"][3, 0, at] and r["k"][0, at] == 5
    step = data[3, at] + 1 if fmt == D.U16 else np.nextafter(data[3, at], np.float32(np.inf))
    assert data[3, beyond] == step and not r["member"][3, 0, beyond] and r["k"][0, beyond] == 3
    assert r["member"][0, 0, beyond]  # (the median is always a member)


@pytest.mark.parametrize("fmt", [D.U16, D.F32], ids=["u16", "f32"])
def test_zero_spread_gives_the_median(fmt):
    frames, fp, value = FU.zero_spread(fmt)
    r = FU.fuse([f["data"] for f in frames], **fp)
    assert FU.same_image(r["image"], value) and (r["cls"] == FU.FUSED).all()


def test_float_sum_depends_on_the_order():
    frames, fp, value = FU.order_of_the_sum()
    r = FU.fuse([f["data"] for f in frames], **fp)
    assert FU.same_image(r["image"], value) and value[0, 0] != value[0, 1] and (r["k"] == 8).all()


def test_special_float_readings_are_invalid_and_a_denormal_is_valid():
    f = np.float32
    stack = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-40, 1.0], f).reshape(8, 1, 1)
    assert FU.valid_mask(stack)[:, 0, 0].tolist() == [False] * 6 + [True, True]
    frames, fp, cases = FU.constructed(D.F32)
    assert "denormals" in cases and 0 < frames[0]["data"][0, cases["denormals"][0]] < np.finfo(f).tiny
