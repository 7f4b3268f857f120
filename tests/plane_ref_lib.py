"""ctypes front of tests/cpp/plane_ref.cpp, the host restatement of PCL 1.7's plane segmentation that agh_remove_plane is
held to ("Table-plane removal").  The library is compiled once per process with g++ -ffp-contract=off."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plane_ref.cpp")
_LIB = None


def build_cmd(out: str) -> list[str]:
    return ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", SRC, "-o", out]


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="plane_ref_"), "libplane_ref.so")
        subprocess.check_call(build_cmd(out))
        _LIB = C.CDLL(out)
        _LIB.pr_rnd.restype = None
    return _LIB


def rnd(seed: int, n: int) -> np.ndarray:
    out = np.zeros(n, np.uint32)
    lib().pr_rnd(C.c_uint32(seed), C.c_int64(n), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def segment(xyz, max_iterations: int = 100, threshold: float = 0.01, probability: float = 0.99, seed: int = 12345,
            optimize: bool = True) -> dict:
    """SACSegmentation::segment + ExtractIndices(negative) on a packed float32 cloud."""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    n = xyz.shape[0]
    cap = max_iterations + 1
    planes = np.zeros((cap, 4), np.float32)
    samples = np.zeros((cap, 3), np.int32)
    counts = np.zeros(cap, np.int64)
    mask = np.zeros(max(n, 1), np.uint8)
    coef = np.zeros(4, np.float32)
    n_cand, best, it = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    found = lib().pr_segment(
        xyz.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(n), C.c_int32(max_iterations), C.c_double(threshold),
        C.c_double(probability), C.c_uint32(seed), C.c_int32(int(optimize)), planes.ctypes.data_as(C.POINTER(C.c_float)),
        samples.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32(cap),
        C.byref(n_cand), C.byref(best), C.byref(it), coef.ctypes.data_as(C.POINTER(C.c_float)),
        mask.ctypes.data_as(C.POINTER(C.c_uint8)))
    k = n_cand.value
    m = mask[:n].astype(bool)
    return {"found": bool(found), "planes": planes[:k], "samples": samples[:k], "counts": counts[:k], "best": best.value,
            "iterations": it.value, "coefficients": coef, "mask": m, "inliers": np.nonzero(m)[0].astype(np.int32)}


def replay_py(counts, n_points: int, max_iterations: int = 100, probability: float = 0.99):
    """RandomSampleConsensus::computeModel's loop, transcribed plainly (candidate i = the i-th model scored)."""
    import math

    best, n_best, k, it = -1, -(2 ** 31 - 1), 1.0, 0
    eps = np.finfo(np.float64).eps
    log_probability = math.log(1.0 - probability)
    one_over_indices = 1.0 / n_points if n_points else math.inf
    i = 0
    while it < k and i < len(counts):
        if counts[i] > n_best:
            n_best, best = int(counts[i]), i
            w = n_best * one_over_indices
            p = min(1.0 - eps, max(eps, 1.0 - math.pow(w, 3.0)))
            k = log_probability / math.log(p)
        it += 1
        i += 1
        if it > max_iterations:
            break
    return best, it
