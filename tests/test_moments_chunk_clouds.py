"""The clouds of tests/test_gpu_moments_chunks.py are in the regime they name: every sample's FLANN ball holds exactly the
stated number of points (numpy, no GPU)."""
import numpy as np

from tests import moments_chunk_clouds as mc


def test_chunk_edge_cloud_counts():
    xyz, cam, s = mc.chunk_edge_cloud()
    assert len(xyz) == mc.CHUNK_EDGES_POINTS and len(cam) == len(xyz)
    assert mc.ball_counts(xyz, s, 0.03) == list(mc.CHUNK_EDGES)
    # what the cases stand for: last chunks one row short, full and of one row, in both tiles; many full chunks; the cap
    rem = [n % mc.CHUNK for n in mc.CHUNK_EDGES]
    assert {mc.CHUNK - 1, 0, 1} <= set(rem)
    last_tile = {((n - 1) // mc.CHUNK) % 2 for n in mc.CHUNK_EDGES}
    assert last_tile == {0, 1}
    assert max(mc.CHUNK_EDGES) == 1152 and 20 * mc.CHUNK in mc.CHUNK_EDGES


def test_big_edge_cloud_counts():
    xyz, _, s = mc.big_edge_cloud()
    assert mc.ball_counts(xyz, s, 0.03) == list(mc.BIG_EDGES)
    assert min(mc.BIG_EDGES) == 1153 and max(mc.BIG_EDGES) == 4096
    assert {n - 21 * mc.CHUNK for n in mc.BIG_EDGES} >= {-1, 0, 1}


def test_small_edge_cloud_counts():
    xyz, _, s = mc.small_edge_cloud()
    assert mc.ball_counts(xyz, s, 0.01) == list(mc.SMALL_EDGES)
    assert max(mc.SMALL_EDGES) <= 256
    # no other point of the cloud has a larger ball than the 256 class holds (the whole pass stays in that class)
    counts = [int(c) for c in mc.ball_counts(xyz, np.arange(len(xyz)), 0.01)]
    assert max(counts) <= 256
