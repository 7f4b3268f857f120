"""Batches of captures for the agh_localize_batch_clustered_fit* tests (numpy only), built from the single-capture cases of
tests/plane_fit_cases.py.  No second model: a capture's fit is plane_fit_cases.fit_model on its own voxelised cloud, its objects
cluster_cases.cluster_model with the model's plane.

A batch is a list of (name, case) pairs, a case as tests/plane_fit_cases.py makes it (`points`, `size_left`, `dense`, `workspace`,
`cell`, `cp`, `fp`, `origins`, `table`); cell_size is equal across a batch, and a batch holds at most 64 lists.  Each batch is
named after the regime tests/test_plane_fit_batch_cases.py proves it is in.

  small_batch      every case of plane_fit_cases.cases() in its order, max_objects lowered to 2: 22 captures, 44 lists
  seed_pair        floor_blocks_small twice: identical coordinates, seeds 1 and 2
  lifted_pair      floor_blocks_small as it is, and lifted by five lattice levels (5 cm)
  origin_batch     floor_blocks_small three times; the origin table's row for capture 1 puts camera 0 below the floor
  origin_table     the n_captures-row agh_set_cloud_cam_origins table of a batch: a case's own one-row table, else its origins
  models           per capture: dict(cloud=(xyz, cams), fit=fit_model(...), cluster=cluster_model(...) or None without a plane)
  args             the arrays a binding call takes for a batch
"""
import functools

import numpy as np

from tests import cluster_cases as CC
from tests import plane_fit_cases as PF

SMALL_MAX_OBJECTS = 2
LIFT = 5  # lattice levels of 1 cm


def _with(c: dict, fp=None, cp=None, **fields) -> dict:
    return dict(c, fp=dict(c["fp"], **(fp or {})), cp=dict(c["cp"], **(cp or {})), **fields)


@functools.lru_cache(maxsize=None)
def _cases() -> dict:
    return PF.cases()


def small_batch() -> list:
    return [(n, _with(c, cp=dict(max_objects=SMALL_MAX_OBJECTS))) for n, c in _cases().items()]


def seed_pair() -> list:
    c = _cases()["floor_blocks_small"]
    return [("seed_1", _with(c, fp=dict(seed=1))), ("seed_2", _with(c, fp=dict(seed=2)))]


def lifted_pair() -> list:
    lifted = [(i, j, k + LIFT) for i, j, k in PF.SMALL]
    return [("as_it_is", _cases()["floor_blocks_small"]), ("lifted", PF._case(lifted))]


def origin_batch() -> list:
    c = _cases()["floor_blocks_small"]
    below = np.array([[0.3, 0.3, 0.0], [0.3, 0.3, 0.0]])
    return [("above_0", c), ("below", _with(c, table=below)), ("above_2", c)]


def origin_table(batch) -> np.ndarray:
    """(n_captures, 2, 3): row k is capture k's rig"""
    return np.stack([np.asarray(c["table"] if c["table"] is not None else c["origins"], np.float64) for _, c in batch])


def models(batch, table=None) -> list:
    """per capture, with camera 0's origin of row k of `table` (origin_table(batch) when None)"""
    table = origin_table(batch) if table is None else table
    out = []
    for k, (_n, c) in enumerate(batch):
        xyz, cams = PF.voxel_cloud(c)
        fit = PF.fit_model(xyz, c["fp"], table[k][0])
        cluster = CC.cluster_model(xyz, dict(c["cp"], plane=tuple(fit["plane"]))) if fit["found"] else None
        out.append(dict(cloud=(xyz, cams), fit=fit, cluster=cluster))
    return out


def args(batch) -> dict:
    """captures, sizes_left, workspaces, dense and the fp and cp fields of a batch, as lists in capture order"""
    assert len({c["cell"] for _, c in batch}) == 1
    assert sum(c["cp"]["max_objects"] for _, c in batch) <= 64
    return dict(captures=[c["points"] for _, c in batch], sizes_left=[c["size_left"] for _, c in batch],
                workspaces=[c["workspace"] for _, c in batch], dense=[c["dense"] for _, c in batch], cp=[c["cp"] for _, c in batch],
                fp=[c["fp"] for _, c in batch], cell=batch[0][1]["cell"])
