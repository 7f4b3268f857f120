"""Batches of captures for the agh_localize_batch_clustered* tests (numpy only), built from the single-capture cases of
tests/cluster_cases.py and tests/cluster_grid_cases.py.

A batch is a list of (name, case) pairs, a case as tests/cluster_cases.py makes it (`points`, `size_left`, `dense`, `workspace`,
`cell`, `cp`); cell_size must be equal across a batch, and a batch holds at most 64 lists (cp["max_objects"] per capture).  Each
batch is named after the regime tests/test_cluster_batch_cases.py proves it is in.

  small_batch      the twelve cases of cluster_cases.cases() in their order, seventy_components lowered to `seventy_lists` lists:
                   22 makes exactly 64 lists, 23 makes 65
  grid_batch       four captures of 1 cm voxels whose search grids have cells of 0.04 / 0.02 / 0.08 / 0.02 m: reach 2 / 3 / 1 / 1
  table_batch      table_scene(5), (6), (7) with K = 4, 3, 5 and S = 60, 45, 60: the chain-equality batch
  first_lists      capture k's first list among the batch's (the exclusive prefix sum of max_objects)
  args             the arrays a binding call takes for a batch
"""
import functools

import numpy as np

from tests import cluster_cases as CC
from tests import cluster_grid_cases as G
from tests import label_batch_cases as LB

SMALL_ORDER = ("threshold_neighbours", "threshold_neighbours_above", "strict_heights", "strict_heights_inside", "snake",
               "both_cameras", "size_ties", "seventy_components", "no_foreground", "all_one_component", "fewer_objects_than_K",
               "non_finite")
SMALL_MAX_OBJECTS = (4, 4, 4, 4, 4, 4, 3, 64, 4, 2, 5, 4)
GRID_ORDER = ("doubled_cells_0.04_tol0.05", "snake_tol0.05", "doubled_cells_0.08_tol0.011", "size_ties")
GRID_CELLS = (0.04, 0.02, 0.08, 0.02)
GRID_REACH = (2, 3, 1, 1)
TABLE_SEEDS, TABLE_K, TABLE_S = (5, 6, 7), (4, 3, 5), (60, 45, 60)


def _with_cp(c: dict, **fields) -> dict:
    return dict(c, cp=dict(c["cp"], **fields))


@functools.lru_cache(maxsize=None)
def _small_cases() -> dict:
    return CC.cases()


def small_batch(seventy_lists: int = 22) -> list:
    cases = _small_cases()
    assert tuple(cases) == SMALL_ORDER
    return [(n, _with_cp(c, max_objects=seventy_lists) if n == "seventy_components" else c) for n, c in cases.items()]


def small_samples(batch) -> list:
    """S_k of the twelve-case batch: 7, and 40 for the snake"""
    return [40 if n == "snake" else 7 for n, _ in batch]


def grid_batch() -> list:
    small, grid = _small_cases(), G.cases()
    return [(GRID_ORDER[0], grid[GRID_ORDER[0]]), (GRID_ORDER[1], _with_cp(small["snake"], tolerance=0.05)),
            (GRID_ORDER[2], grid[GRID_ORDER[2]]), (GRID_ORDER[3], small["size_ties"])]


@functools.lru_cache(maxsize=None)
def table_scenes() -> tuple:
    """per capture of the chain-equality batch: dict(xyz, size_left, ws, ws_cut, origins, cp, S), read-only"""
    out = []
    for seed, K, S in zip(TABLE_SEEDS, TABLE_K, TABLE_S):
        xyz, size_left, ws, origins, cp = CC.table_scene(seed)
        xyz.setflags(write=False)
        ws_cut = ws.copy()
        ws_cut[1] = 0.75 + 25 * 0.003 + 0.004  # the +x face through the second cube
        out.append(dict(xyz=xyz, size_left=size_left, ws=ws, ws_cut=ws_cut, origins=origins, cp=dict(cp, max_objects=K), S=S))
    return tuple(out)


def first_lists(batch) -> np.ndarray:
    return LB.first_lists([(n, dict(n_objects=c["cp"]["max_objects"])) for n, c in batch])


def args(batch) -> dict:
    """captures, sizes_left, workspaces, dense and the cp fields of a batch, as lists in capture order"""
    assert len({c["cell"] for _, c in batch}) == 1
    return dict(captures=[c["points"] for _, c in batch], sizes_left=[c["size_left"] for _, c in batch],
                workspaces=[c["workspace"] for _, c in batch], dense=[c["dense"] for _, c in batch], cp=[c["cp"] for _, c in batch],
                cell=batch[0][1]["cell"])
