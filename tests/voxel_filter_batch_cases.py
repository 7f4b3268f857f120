"""Batches of captures for the agh_set_voxel_filter tests of the masked, labelled and clustered batch chains (numpy only), and
their models COMPOSED from what exists: voxel_filter_cases.filter_model / filtered_cloud / filtered_eligible, cluster_cases.
cluster_model and plane_fit_cases.fit_model on the filtered cloud.  No model of the filter or of a stage is stated here.

A batch is a list of (name, case) pairs.  All cases have 1 cm voxels and dense = True, and one filter holds for a whole batch: the
setting is the context's.

  lattice_batch    eight lattice captures of voxel_filter_cases.cases() at radius 2, min_neighbors 2, among them an empty and a
                   wholly pruned one; every case carries `mask`, `labels` (two objects) and `model` (filter_model's dict)
  bridged_batch    four captures of plane_fit_cases at radius 1, min_neighbors 3: two blocks on a floor joined by a bridge one
                   voxel thick, which the filter takes away -- one object unfiltered, two filtered
  outgrowing_case  a lattice capture with more bitmap words than a slot sized by lattice_batch holds
  raw_rows         per raw point the row of its voxel in the UNFILTERED cloud (-1: not kept)
  leaky_eligible   the list a mark kernel would give that lets the points of pruned voxels through: each marks the row its pruned
                   voxel's index falls on among the survivors -- the next surviving one
  masked_model / labeled_model / cluster_models    what the GPU tests hold a batch against
"""
import functools

import numpy as np

from tests import cluster_cases as CC
from tests import mask_batch_cases as MB
from tests import mask_cases as M
from tests import plane_fit_batch_cases as PB
from tests import plane_fit_cases as PF
from tests import voxel_filter_cases as VF

F32 = np.float32
LATTICE_FILTER = dict(radius=2, min_neighbors=2)
BRIDGED_FILTER = dict(radius=1, min_neighbors=3)
LATTICE_ORDER = ("last_word", "seams", "empty", "cam1_seams", "one_voxel", "camera0_inside_camera1", "dense_block",
                 "cam1_block_neighbours")
LEAK_CASES = ("seams", "cam1_seams", "camera0_inside_camera1")  # (tests/test_voxel_filter_batch_cases.py: a leak shows in them)
BRIDGE = [(5, 4, 2), (6, 4, 2), (7, 4, 2), (8, 4, 2), (8, 5, 2), (8, 6, 2)]
STRAYS = [(0, 11, 4), (11, 0, 3), (6, 1, 4)]
BRIDGED_ORDER = ("bridged", "floor_blocks_small", "bridged_lifted", "both_cameras")


def raw_rows(points, cams, workspace, cell) -> np.ndarray:
    """mask_cases._voxels, per raw point: the row of its voxel in the unfiltered voxelised cloud, camera 0's block first"""
    rows, base = np.full(len(points), -1, np.int64), 0
    for sel, ijk in M._voxels(points, cams, workspace, cell):
        if len(sel) == 0:
            continue
        uniq, inv = np.unique(ijk, axis=0, return_inverse=True)
        rows[sel] = base + inv.reshape(-1)
        base += len(uniq)
    return rows


def pruned_points(rows, keep) -> np.ndarray:
    """per raw point: kept by the preprocessing, and its voxel pruned by the filter"""
    out = np.zeros(len(rows), bool)
    out[rows >= 0] = ~keep[rows[rows >= 0]]
    return out


def leaky_eligible(rows, keep, mask) -> np.ndarray:
    """The indices, in the FILTERED cloud, that the masked points mark when a point of a pruned voxel is not stopped: its voxel's
    index among the survivors is the number of surviving rows before it, which is the next surviving row's (none beyond the last)."""
    before = np.cumsum(keep) - keep  # surviving rows ahead of row r
    sel = (rows >= 0) & (np.asarray(mask).reshape(-1) != 0)
    idx = before[rows[sel]]
    return np.unique(idx[idx < keep.sum()]).astype(np.int32)


def _mask(rows, keep) -> np.ndarray:
    """every raw point whose voxel the model prunes, and every fourth raw point"""
    m = pruned_points(rows, keep)
    m[::4] = True
    return m.astype(np.uint8)


def _labels(rows, keep, cam) -> np.ndarray:
    """Two objects by raw index parity; every point of a pruned voxel gets the object that the next surviving row of its camera
    does not receive from the points of surviving voxels, wherever that row exists and receives one object only."""
    labels = (1 + np.arange(len(rows)) % 2).astype(np.uint8)
    pruned = pruned_points(rows, keep)
    alive = (rows >= 0) & ~pruned
    got = np.zeros((len(keep), 2), bool)  # per unfiltered row: the objects its surviving points give it
    got[rows[alive], labels[alive] - 1] = True
    surviving = np.flatnonzero(keep)
    for i in np.flatnonzero(pruned):
        q = np.searchsorted(surviving, rows[i])
        if q == len(surviving) or cam[surviving[q]] != cam[rows[i]]:
            continue
        objs = got[surviving[q]]
        if objs.sum() == 1:
            labels[i] = 2 if objs[0] else 1
    return labels


def _annotate(base: dict, fp: dict) -> dict:
    """the capture fields of `base` with the filter `fp`, its model, and the mask and labels made from the model"""
    c = {f: base[f] for f in ("points", "size_left", "dense", "workspace", "cell")}
    c.update(fp)
    cams = VF.case_cams(c)
    m = VF.filter_model(c["points"], cams, c["workspace"], c["cell"], **fp)
    rows = raw_rows(c["points"], cams, c["workspace"], c["cell"])
    c.update(cams=cams, model=m, rows=rows, mask=_mask(rows, m["keep"]), labels=_labels(rows, m["keep"], m["cam"]), n_objects=2)
    for f in ("mask", "labels"):
        c[f].setflags(write=False)
    return c


def _lattice_case(name: str) -> dict:
    base = VF.cases()["one_voxel" if name == "empty" else name]
    if name == "empty":
        base = dict(base, points=np.zeros((0, 3), F32), size_left=0)
    return _annotate(base, LATTICE_FILTER)


OUTGROWING_DIM = (130, 64, 110)  # 915 200 bits, 28 600 words: more than the 24 576 of a slot sized by cam1_block_neighbours


@functools.lru_cache(maxsize=None)
def outgrowing_case() -> dict:
    """A capture whose lattice outgrows the slots every lattice_batch capture fits: three runs of three voxels, one at the
    lattice's far end (the far pin beside it), which survive radius 2, min_neighbors 2, and strays (the corner pin among them)
    that do not."""
    runs = [(10 + i, 10, 10) for i in range(3)] + [(60, 30 + i, 33) for i in range(3)] + [(128, 62, 107 + i) for i in range(3)]
    strays = [(5, 50, 60), (100, 3, 7), (64, 32, 5), (127, 0, 109)]
    return _annotate(VF._case(VF._with_pins(runs + strays, OUTGROWING_DIM), check=None, **LATTICE_FILTER), LATTICE_FILTER)


@functools.lru_cache(maxsize=None)
def _lattice_cases() -> dict:
    return {name: _lattice_case(name) for name in LATTICE_ORDER}


def lattice_batch(reverse: bool = False) -> list:
    batch = [(name, _lattice_cases()[name]) for name in LATTICE_ORDER]
    return batch[::-1] if reverse else batch


def filtered_cloud(c: dict):
    return VF.filtered_cloud(c["points"], c["cams"], c["workspace"], c["cell"], c["model"]["keep"])


def masked_model(c: dict, mask=None, filtered: bool = True):
    """(E, cloud) of a capture under the filter, as tests/test_gpu_localize_batch_masked.py's _check_model takes them -- or,
    filtered = False, of the same capture and mask on a context without one"""
    mask = c["mask"] if mask is None else mask
    if not filtered:
        return (M.eligible_model(c["points"], c["cams"], mask, c["workspace"], c["cell"]),
                VF.unfiltered_cloud(c["points"], c["cams"], c["workspace"], c["cell"]))
    return (VF.filtered_eligible(c["points"], c["cams"], mask, c["workspace"], c["cell"], c["model"]["keep"]), filtered_cloud(c))


def labeled_model(c: dict, filtered: bool = True):
    """([E_0, E_1], cloud)"""
    parts = [masked_model(c, c["labels"] == j + 1, filtered) for j in range(c["n_objects"])]
    return [p[0] for p in parts], parts[0][1]


def masked_samples_of(name: str, m: int) -> int:
    return MB.n_samples(name, m)


def labeled_samples_of(name: str, ms) -> int:
    """S per object, around the longest list as mask_batch_cases.n_samples is around M"""
    return MB.n_samples(name, max(ms))


def seed(k: int) -> int:
    return MB.seed(k)


def args(batch) -> dict:
    """the arrays a masked or labelled binding call takes for a lattice batch"""
    return dict(captures=[c["points"] for _, c in batch], sizes_left=[c["size_left"] for _, c in batch],
                workspaces=[c["workspace"] for _, c in batch])


# ---- the bridged batch ----

def _lifted(ijk):
    return [(i, j, k + PB.LIFT) for i, j, k in ijk]


@functools.lru_cache(maxsize=None)
def _bridged_cases() -> dict:
    bridged = PF.SMALL + BRIDGE + STRAYS
    lift_plane = (0.0, 0.0, 1.0, -(CC.ORIGIN[2] + PB.LIFT * CC.CELL))  # the given plane of the lifted capture: its own floor
    cases = PF.cases()
    out = {"bridged": PF._case(bridged), "floor_blocks_small": cases["floor_blocks_small"],
           "bridged_lifted": PF._case(_lifted(bridged), plane=lift_plane), "both_cameras": cases["both_cameras"]}
    for c in out.values():
        c["points"].setflags(write=False)
    return out


def bridged_batch(reverse: bool = False) -> list:
    batch = [(name, _bridged_cases()[name]) for name in BRIDGED_ORDER]
    return batch[::-1] if reverse else batch


def bridged_filter_model(c: dict, fp=BRIDGED_FILTER) -> dict:
    cams = M.camera_ids(c["points"], c["size_left"], c["dense"])
    return VF.filter_model(c["points"], cams, c["workspace"], c["cell"], **fp)


def bridged_cloud(c: dict, fp=BRIDGED_FILTER):
    """the capture's voxelised cloud under the filter `fp` (None: unfiltered)"""
    cams = M.camera_ids(c["points"], c["size_left"], c["dense"])
    if fp is None:
        return VF.unfiltered_cloud(c["points"], cams, c["workspace"], c["cell"])
    return VF.filtered_cloud(c["points"], cams, c["workspace"], c["cell"], bridged_filter_model(c, fp)["keep"])


def cluster_models(batch, fp=BRIDGED_FILTER, fitted: bool = False) -> list:
    """per capture dict(cloud, fit, cluster), the way plane_fit_batch_cases.models makes them, on the cloud under the filter `fp`:
    `cluster` above the case's given plane, or -- fitted -- above the plane fit_model finds (None without one)"""
    table = PB.origin_table(batch)
    out = []
    for k, (_n, c) in enumerate(batch):
        xyz, cams = bridged_cloud(c, fp)
        if not fitted:
            out.append(dict(cloud=(xyz, cams), fit=None, cluster=CC.cluster_model(xyz, c["cp"])))
            continue
        fit = PF.fit_model(xyz, c["fp"], table[k][0])
        cluster = CC.cluster_model(xyz, dict(c["cp"], plane=tuple(fit["plane"]))) if fit["found"] else None
        out.append(dict(cloud=(xyz, cams), fit=fit, cluster=cluster))
    return out
