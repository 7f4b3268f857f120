"""Inputs for the summation loop of k_taubin_moments: neighbourhoods whose sizes sit on the edges of its 56-neighbour chunks
(tests/test_moments_chunk_clouds.py checks the counts on the CPU; tests/test_gpu_moments_chunks.py runs them on the GPU).

The loop forms chunk c + 1 into one term tile while it adds chunk c out of the other, so a case is named by its number of
chunks, by whether the last chunk is full, and by the tile (chunk index modulo 2) the last chunk lands in.
"""
from __future__ import annotations

from tests import capacity_clouds as cc

CHUNK = 56  # kChunk (taubin.hip)

# 1152 class, r = 0.03: one, two and three chunks minus one row / exact / plus one row (last chunk in tile 0, 1, 0, 1);
# twenty full chunks; 1151 (a last chunk of 31) and the class's cap (a last chunk of 32, the 21st: tile 0)
CHUNK_EDGES = (1, 55, 56, 57, 111, 112, 113, 167, 168, 169, 1120, 1151, 1152)
CHUNK_EDGES_POINTS = 6964
# 4096 class: the first size beyond 1152, 21 chunks minus one row / exact / plus one row, 4095 and the cap
BIG_EDGES = (1153, 1175, 1176, 1177, 4095, 4096)
# all-points pass, r = 0.01, 256 class: one chunk minus one row / exact / plus one row
SMALL_EDGES = (55, 56, 57)


def chunk_edge_cloud():
    return cc.ball_cloud(CHUNK_EDGES, 0.03, seed=3, filler=300)


def big_edge_cloud():
    return cc.ball_cloud(BIG_EDGES, 0.03, seed=4, filler=300)


def small_edge_cloud():
    return cc.ball_cloud(SMALL_EDGES, 0.01, seed=5, filler=200)


def ball_counts(xyz, samples, r):
    return [int(cc.in_ball(xyz, xyz[i], r).sum()) for i in samples]
