"""ctypes binding of libagile_grasp_hip.so (the C ABI of include/agh.h) for tests and bench.py.

The product is the shared library; this module only marshals numpy / torch buffers into it.  There is no CPU
fallback: if the library or a gfx950 device is missing, loading or ``Context()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

NORMALS_DETERMINISTIC = 0
NORMALS_RAND50 = 1


class AghParams(C.Structure):
    _fields_ = [
        ("finger_width", C.c_double),
        ("hand_outer_diameter", C.c_double),
        ("hand_depth", C.c_double),
        ("hand_height", C.c_double),
        ("init_bite", C.c_double),
        ("nn_radius_taubin", C.c_double),
        ("nn_radius_hands", C.c_double),
        ("nn_radius_normals", C.c_double),
        ("cam_origin", (C.c_double * 3) * 2),
        ("normals_mode", C.c_int32),
        ("rand_seed", C.c_uint32),
        ("device", C.c_int32),
        ("profile", C.c_int32),
    ]


class AghTiming(C.Structure):
    _fields_ = [("ms", C.c_float * 16), ("name", C.c_char_p * 16), ("n", C.c_int32), ("total_ms", C.c_float)]


HYP_DTYPE = np.dtype(
    [
        ("axis", "<f8", 3),
        ("approach", "<f8", 3),
        ("binormal", "<f8", 3),
        ("bottom", "<f8", 3),
        ("surface", "<f8", 3),
        ("width", "<f8"),
        ("sample", "<i4"),
        ("orientation", "<i4"),
        ("cam_source", "<i4"),
        ("n_in_box", "<i4"),
        ("half_antipodal", "u1"),
        ("full_antipodal", "u1"),
        ("svm_keep", "u1"),
        ("valid", "u1"),
        ("finger_index", "<i4"),
        ("depth_index", "<i4"),
        ("epoch", "<i4"),
    ]
)
FRAME_DTYPE = np.dtype(
    [
        ("sample", "<f8", 3),
        ("normal", "<f8", 3),
        ("axis", "<f8", 3),
        ("binormal", "<f8", 3),
        ("params", "<f8", 10),
        ("eigenvalue", "<f8"),
        ("n_nb", "<i4"),
        ("majority_cam", "<i4"),
        ("max_index", "<i4"),
        ("valid", "<i4"),
    ]
)
HANDLE_DTYPE = np.dtype([("axis", "<f8", 3), ("center", "<f8", 3), ("approach", "<f8", 3), ("binormal", "<f8", 3),
                         ("hands_center", "<f8", 3), ("width", "<f8"), ("n_inliers", "<i4"), ("first_inlier", "<i4")])
assert HYP_DTYPE.itemsize == 160 and FRAME_DTYPE.itemsize == 200 and HANDLE_DTYPE.itemsize == 136

EXPORTS = [
    "agh_default_params", "agh_create", "agh_destroy", "agh_last_error", "agh_set_cloud", "agh_set_cloud_device", "agh_set_cloud_batch", "agh_set_cloud_batch_device",
    "agh_preprocess", "agh_preprocess_device", "agh_localize", "agh_localize_device", "agh_localize_begin", "agh_localize_stage", "agh_localize_end", "agh_localize_batch", "agh_localize_batch_device", "agh_localize_batch_begin", "agh_localize_batch_begin_device",
    "agh_localize_batch_stage", "agh_localize_batch_end", "agh_get_cloud", "agh_find_handles", "agh_find_hands", "agh_find_hands_device", "agh_load_svm", "agh_load_svm_file", "agh_classify",
    "agh_classify_device", "agh_get_frames", "agh_get_neighbor_counts", "agh_get_images", "agh_get_hog",
    "agh_get_normals", "agh_get_timing", "agh_get_timing_counts", "agh_get_grid_stats", "agh_get_grid_desc", "agh_set_profile", "agh_synchronize", "agh_selftest_math",
    "agh_set_training_images", "agh_get_training_images", "agh_hog_images", "agh_train_svm", "agh_save_svm_file",
    "agh_load_svm_model", "agh_get_learning_points", "agh_get_epoch", "agh_get_packed_images", "agh_classify_images", "agh_comm_rccl_origin",
    "agh_save_svm_file_ex", "agh_comm_unique_id", "agh_comm_init", "agh_comm_init_local", "agh_comm_destroy", "agh_comm_rank", "agh_comm_last_count", "agh_comm_last_exchange", "agh_comm_set_segment_records", "agh_comm_inject_fault",
    "agh_shard_slice", "agh_find_hands_sharded_device", "agh_find_hands_sharded", "agh_classify_sharded_device",
    "agh_classify_sharded", "agh_default_plane_params", "agh_remove_plane", "agh_get_plane_inliers",
    "agh_get_plane_candidates", "agh_plane_replay", "agh_set_cloud_cam_origins", "agh_get_cloud_cam_origins",
    "agh_deproject", "agh_localize_depth", "agh_localize_depth_device", "agh_localize_depth_begin", "agh_localize_depth_stage",
    "agh_deproject_batch", "agh_localize_depth_batch", "agh_localize_depth_batch_device", "agh_localize_depth_batch_begin",
    "agh_localize_depth_batch_begin_device",
    "agh_localize_masked", "agh_localize_masked_device", "agh_localize_masked_begin", "agh_localize_depth_masked",
    "agh_localize_depth_masked_device", "agh_localize_depth_masked_begin", "agh_get_sample_mask_count",
    "agh_localize_labeled", "agh_localize_labeled_device", "agh_localize_depth_labeled", "agh_localize_depth_labeled_device",
    "agh_get_label_counts",
    "agh_default_cluster_params", "agh_localize_clustered", "agh_localize_clustered_device", "agh_localize_depth_clustered",
    "agh_localize_depth_clustered_device", "agh_get_cluster_info", "agh_get_cluster_labels",
    "agh_default_plane_fit_params", "agh_localize_clustered_fit", "agh_localize_clustered_fit_device",
    "agh_localize_depth_clustered_fit", "agh_localize_depth_clustered_fit_device", "agh_get_plane_fit",
    "agh_get_plane_fit_candidates",
    "agh_localize_batch_masked", "agh_localize_batch_masked_device", "agh_localize_batch_masked_begin",
    "agh_localize_batch_masked_begin_device", "agh_localize_depth_batch_masked", "agh_localize_depth_batch_masked_device",
    "agh_localize_depth_batch_masked_begin", "agh_localize_depth_batch_masked_begin_device", "agh_get_batch_mask_counts",
    "agh_localize_batch_labeled", "agh_localize_batch_labeled_device", "agh_localize_batch_labeled_begin",
    "agh_localize_batch_labeled_begin_device", "agh_localize_depth_batch_labeled", "agh_localize_depth_batch_labeled_device",
    "agh_localize_depth_batch_labeled_begin", "agh_localize_depth_batch_labeled_begin_device", "agh_get_batch_label_counts",
    "agh_localize_batch_clustered", "agh_localize_batch_clustered_device", "agh_localize_batch_clustered_begin",
    "agh_localize_batch_clustered_begin_device", "agh_localize_depth_batch_clustered", "agh_localize_depth_batch_clustered_device",
    "agh_localize_depth_batch_clustered_begin", "agh_localize_depth_batch_clustered_begin_device", "agh_get_batch_cluster_info",
    "agh_get_batch_cluster_labels",
    "agh_localize_batch_clustered_fit", "agh_localize_batch_clustered_fit_device", "agh_localize_batch_clustered_fit_begin",
    "agh_localize_batch_clustered_fit_begin_device", "agh_localize_depth_batch_clustered_fit",
    "agh_localize_depth_batch_clustered_fit_device", "agh_localize_depth_batch_clustered_fit_begin",
    "agh_localize_depth_batch_clustered_fit_begin_device", "agh_get_batch_plane_fit", "agh_get_batch_plane_fit_candidates",
    "agh_default_depth_filter_params", "agh_set_depth_filter", "agh_get_depth_filter", "agh_get_depth_filter_counts",
    "agh_default_depth_fusion_params", "agh_fuse_depth", "agh_fuse_depth_device", "agh_get_depth_fusion_counts", "agh_get_fused_depth",
    "agh_default_voxel_filter_params", "agh_set_voxel_filter", "agh_get_voxel_filter", "agh_get_voxel_filter_counts",
    "agh_default_hand_filter_params", "agh_set_hand_filter", "agh_get_hand_filter", "agh_get_hand_filter_counts",
    "agh_default_hand_clearance_params", "agh_set_hand_clearance", "agh_get_hand_clearance", "agh_get_hand_clearance_counts",
    "agh_default_handle_ranking_params", "agh_set_handle_ranking", "agh_get_handle_ranking", "agh_get_handle_scores",
    "agh_get_handle_ranking_counts", "agh_get_hand_margins", "agh_rank_handles",
]


def comm_unique_id() -> bytes:
    """ncclGetUniqueId: call on one rank, hand the 128 bytes to the others."""
    buf = (C.c_uint8 * 128)()
    rc = load_library().agh_comm_unique_id(buf)
    if rc != 0:
        raise AghError(rc, "agh_comm_unique_id failed (is RCCL installed?)")
    return bytes(buf)


def comm_init_local(contexts) -> None:
    """The contexts (one host thread each) become the ranks of an in-process communicator: the sharded schedule with
    device copies instead of RCCL, for validation on a single GPU."""
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    rc = load_library().agh_comm_init_local(arr, C.c_int32(len(contexts)))
    if rc != 0:
        raise AghError(rc, "agh_comm_init_local failed")


def shard_slice(n: int, rank: int, n_ranks: int):
    lo, hi = C.c_int64(0), C.c_int64(0)
    load_library().agh_shard_slice(C.c_int64(n), C.c_int32(rank), C.c_int32(n_ranks), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def comm_rccl_origin() -> str:
    """Which RCCL image the library bound (binds it if that has not happened yet)."""
    lib = load_library()
    lib.agh_comm_rccl_origin.restype = C.c_char_p
    return lib.agh_comm_rccl_origin().decode()


def pack_images(images: np.ndarray) -> np.ndarray:
    """(n, 8000) uint8 images (0 / 255) -> (n, 250) uint32 words, bit (b & 31) of word (b >> 5) = pixel b."""
    im = np.ascontiguousarray(images, np.uint8).reshape(-1, 8000) != 0
    return np.packbits(im, axis=1, bitorder="little").view("<u4").reshape(-1, 250).copy()


def unpack_images(words: np.ndarray) -> np.ndarray:
    w = np.ascontiguousarray(words, "<u4").reshape(-1, 250)
    return (np.unpackbits(w.view(np.uint8), axis=1, bitorder="little") * np.uint8(255)).reshape(-1, 8000)


SVM_LINEAR = 0
SVM_POLY2 = 1


def save_svm_file(path: str, w: np.ndarray, rho: float, kernel: int = SVM_LINEAR, alpha: np.ndarray | None = None) -> None:
    """CvSVM::save (needs no device): the compacted linear vector (w: 3528 floats) or, with `alpha`, the support
    vectors (w: n_sv x 3528) of a model with the given kernel."""
    sv = np.ascontiguousarray(w, np.float32).reshape(-1, 3528)
    al = np.ones(1, np.float64) if alpha is None else np.ascontiguousarray(alpha, np.float64)
    assert al.shape[0] == sv.shape[0]
    rc = load_library().agh_save_svm_file(path.encode(), C.c_int32(kernel), _p(sv, C.c_float), C.c_int32(sv.shape[0]),
                                          C.c_int32(3528), _p(al, C.c_double), C.c_double(rho))
    if rc != 0:
        raise AghError(rc, f"cannot write {path}")


class AghLocalizeParams(C.Structure):
    _fields_ = [("size_left", C.c_int64), ("dense", C.c_int32), ("classify", C.c_int32), ("workspace", C.c_double * 6),
                ("cell_size", C.c_double), ("sample_idx", C.POINTER(C.c_int32)), ("n_samples", C.c_int64),
                ("sample_seed", C.c_uint64), ("min_inliers", C.c_int32), ("filters_boundaries", C.c_int32),
                ("min_length", C.c_double)]


class AghLocalizeResult(C.Structure):
    _fields_ = [("n_voxels", C.c_int64), ("n_hypotheses", C.c_int64), ("n_hands", C.c_int64), ("n_handles", C.c_int64),
                ("n_inlier_idx", C.c_int64)]


class AghLocalizeBatchResult(C.Structure):
    _fields_ = [("r", AghLocalizeResult), ("first_handle", C.c_int64), ("first_inlier_idx", C.c_int64), ("first_hand", C.c_int64),
                ("first_sample", C.c_int64)]


class AghClusterParams(C.Structure):
    _fields_ = [("plane", C.c_double * 4), ("min_height", C.c_double), ("max_height", C.c_double), ("tolerance", C.c_double),
                ("min_voxels", C.c_int32), ("max_objects", C.c_int32)]


class AghClusterInfo(C.Structure):
    _fields_ = [("n_foreground", C.c_int64), ("n_components", C.c_int64), ("n_objects", C.c_int64)]


def cluster_params(**fields) -> AghClusterParams:
    """agh_default_cluster_params, then the given fields (plane: four numbers)."""
    cp = AghClusterParams()
    load_library().agh_default_cluster_params(C.byref(cp))
    for k, v in fields.items():
        if k == "plane":
            v = (C.c_double * 4)(*[float(x) for x in v])
        elif not hasattr(cp, k):
            raise TypeError(f"agh_cluster_params has no field {k}")
        setattr(cp, k, v)
    return cp


class AghPlaneFitParams(C.Structure):
    _fields_ = [("n_candidates", C.c_int32), ("refine", C.c_int32), ("min_inliers", C.c_int32), ("reserved", C.c_int32),
                ("distance_threshold", C.c_double), ("seed", C.c_uint64)]


class AghPlaneFitResult(C.Structure):
    _fields_ = [("plane", C.c_double * 4), ("n_voxels", C.c_int64), ("n_inliers", C.c_int64), ("n_refit", C.c_int64),
                ("best_candidate", C.c_int32), ("found", C.c_int32), ("refined", C.c_int32), ("reserved", C.c_int32)]


def plane_fit_params(**fields) -> AghPlaneFitParams:
    """agh_default_plane_fit_params, then the given fields."""
    fp = AghPlaneFitParams()
    load_library().agh_default_plane_fit_params(C.byref(fp))
    for k, v in fields.items():
        if not hasattr(fp, k):
            raise TypeError(f"agh_plane_fit_params has no field {k}")
        setattr(fp, k, v)
    return fp


DEPTH_U16, DEPTH_F32 = 0, 1


class AghDepthImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("row_stride_bytes", C.c_int64),
                ("format", C.c_int32), ("depth_scale", C.c_float), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("pose", C.c_double * 12)]


class AghDepthFilterParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("min_support", C.c_int32), ("max_jump_abs", C.c_double), ("max_jump_rel", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double)]


class AghDepthFilterCounts(C.Structure):
    _fields_ = [("n_valid", C.c_int64), ("n_out_of_range", C.c_int64), ("n_unsupported", C.c_int64), ("n_kept", C.c_int64)]


class AghDepthFusionParams(C.Structure):
    _fields_ = [("min_valid", C.c_int32), ("reserved", C.c_int32), ("max_spread_abs", C.c_double), ("max_spread_rel", C.c_double)]


class AghDepthFusionCounts(C.Structure):
    _fields_ = [("n_pixels", C.c_int64), ("n_empty", C.c_int64), ("n_unsupported", C.c_int64), ("n_inconsistent", C.c_int64),
                ("n_fused", C.c_int64), ("n_filled", C.c_int64)]


class AghVoxelFilterParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("min_neighbors", C.c_int32)]


class AghVoxelFilterCounts(C.Structure):
    _fields_ = [("n_occupied", C.c_int64 * 2), ("n_pruned", C.c_int64 * 2), ("n_kept", C.c_int64 * 2)]


class AghHandFilterParams(C.Structure):
    _fields_ = [("approach_on", C.c_int32), ("width_on", C.c_int32), ("view_on", C.c_int32), ("probes_per_finger", C.c_int32),
                ("approach_dir", C.c_double * 3), ("min_approach_cos", C.c_double), ("min_width", C.c_double),
                ("max_width", C.c_double), ("depth_margin", C.c_double), ("max_unobserved", C.c_int32), ("reserved", C.c_int32)]


class AghHandFilterCounts(C.Structure):
    _fields_ = [("n_hypotheses", C.c_int64), ("n_dropped_approach", C.c_int64), ("n_dropped_width", C.c_int64),
                ("n_dropped_unobserved", C.c_int64), ("n_kept", C.c_int64)]


class AghHandClearanceParams(C.Structure):
    _fields_ = [("near_offset", C.c_double), ("far_offset", C.c_double), ("half_width", C.c_double), ("half_height", C.c_double),
                ("max_points", C.c_int32), ("reserved", C.c_int32)]


class AghHandClearanceCounts(C.Structure):
    _fields_ = [("n_tested", C.c_int64), ("n_dropped", C.c_int64), ("n_kept", C.c_int64)]


class AghHandleRankingParams(C.Structure):
    _fields_ = [("w_support", C.c_double), ("w_margin", C.c_double), ("w_approach", C.c_double), ("w_position", C.c_double),
                ("w_distance", C.c_double), ("w_width", C.c_double), ("w_length", C.c_double), ("approach_dir", C.c_double * 3),
                ("position_dir", C.c_double * 3), ("ref_point", C.c_double * 3), ("preferred_width", C.c_double),
                ("min_score", C.c_double), ("support_cap", C.c_int32), ("max_handles", C.c_int32)]


class AghHandleScore(C.Structure):
    _fields_ = [("score", C.c_double), ("terms", C.c_double * 7), ("index", C.c_int32), ("best_inlier", C.c_int32)]


class AghHandleRankingCounts(C.Structure):
    _fields_ = [("n_found", C.c_int64), ("n_below", C.c_int64), ("n_returned", C.c_int64)]


SCORE_DTYPE = np.dtype([("score", "<f8"), ("terms", "<f8", 7), ("index", "<i4"), ("best_inlier", "<i4")])
assert SCORE_DTYPE.itemsize == 72 == C.sizeof(AghHandleScore)


def handle_ranking_params(**fields) -> AghHandleRankingParams:
    """agh_default_handle_ranking_params, then the given fields (the three vectors: any sequence of three floats)."""
    rp = AghHandleRankingParams()
    load_library().agh_default_handle_ranking_params(C.byref(rp))
    for k, v in fields.items():
        if not hasattr(rp, k):
            raise TypeError(f"agh_handle_ranking_params has no field {k}")
        if k in ("approach_dir", "position_dir", "ref_point"):
            v = (C.c_double * 3)(*[float(x) for x in v])
        setattr(rp, k, v)
    return rp


def hand_clearance_params(**fields) -> AghHandClearanceParams:
    """agh_default_hand_clearance_params, then the given fields."""
    cp = AghHandClearanceParams()
    load_library().agh_default_hand_clearance_params(C.byref(cp))
    for k, v in fields.items():
        if not hasattr(cp, k):
            raise TypeError(f"agh_hand_clearance_params has no field {k}")
        setattr(cp, k, v)
    return cp


def hand_filter_params(**fields) -> AghHandFilterParams:
    """agh_default_hand_filter_params, then the given fields (approach_dir: any sequence of three floats)."""
    fp = AghHandFilterParams()
    load_library().agh_default_hand_filter_params(C.byref(fp))
    for k, v in fields.items():
        if not hasattr(fp, k):
            raise TypeError(f"agh_hand_filter_params has no field {k}")
        setattr(fp, k, (C.c_double * 3)(*[float(x) for x in v]) if k == "approach_dir" else v)
    return fp


def voxel_filter_params(**fields) -> AghVoxelFilterParams:
    """agh_default_voxel_filter_params, then the given fields."""
    fp = AghVoxelFilterParams()
    load_library().agh_default_voxel_filter_params(C.byref(fp))
    for k, v in fields.items():
        if not hasattr(fp, k):
            raise TypeError(f"agh_voxel_filter_params has no field {k}")
        setattr(fp, k, v)
    return fp


def depth_filter_params(**fields) -> AghDepthFilterParams:
    """agh_default_depth_filter_params, then the given fields."""
    fp = AghDepthFilterParams()
    load_library().agh_default_depth_filter_params(C.byref(fp))
    for k, v in fields.items():
        if not hasattr(fp, k):
            raise TypeError(f"agh_depth_filter_params has no field {k}")
        setattr(fp, k, v)
    return fp


def depth_fusion_params(**fields) -> AghDepthFusionParams:
    """agh_default_depth_fusion_params, then the given fields."""
    fp = AghDepthFusionParams()
    load_library().agh_default_depth_fusion_params(C.byref(fp))
    for k, v in fields.items():
        if not hasattr(fp, k):
            raise TypeError(f"agh_depth_fusion_params has no field {k}")
        setattr(fp, k, v)
    return fp


class DeviceImage:
    """A fused depth image in a slot buffer of its context (Context.fuse_depth): the few tensor methods depth_image_records asks
    of a torch CUDA tensor, so that the handle goes wherever such a tensor goes.  Valid until its slot is fused again or the
    context is closed."""
    is_cuda = True

    def __init__(self, rec: "AghDepthImage"):
        self._ptr, self.shape = int(rec.data), (int(rec.height), int(rec.width))
        self._es = 2 if rec.format == DEPTH_U16 else 4
        self._row = int(rec.row_stride_bytes) // self._es

    def dim(self):
        return 2

    def stride(self, k: int):
        return (self._row, 1)[k]

    def element_size(self):
        return self._es

    def data_ptr(self):
        return self._ptr


def depth_image_records(images):
    """The agh_depth_image records of a capture.  `images`: one or two dicts with `data` (an (H, W) uint16 or float32 array whose
    rows may be padded -- a column slice of a wider array -- or a torch CUDA tensor for the _device call), fx, fy, cx, cy, `pose`
    (3 x 4, camera optical frame -> cloud frame) and, for uint16, depth_scale (default 0.001).  Returns (records, what keeps the
    pixel buffers alive, on_device)."""
    recs = (AghDepthImage * len(images))()
    keep = []
    on_device = any(hasattr(im["data"], "is_cuda") and im["data"].is_cuda for im in images)
    for r, im in zip(recs, images):
        d = im["data"]
        if on_device:
            assert d.is_cuda and d.dim() == 2 and d.stride(1) == 1
            es = d.element_size()
            r.data, r.height, r.width, r.row_stride_bytes = d.data_ptr(), int(d.shape[0]), int(d.shape[1]), int(d.stride(0)) * es
            is_u16 = es == 2
        else:
            assert isinstance(d, np.ndarray) and d.ndim == 2 and d.dtype in (np.uint16, np.float32), "uint16 or float32 (H, W)"
            assert d.strides[1] == d.itemsize and d.strides[0] >= d.shape[1] * d.itemsize, "rows must be contiguous"
            r.data, r.height, r.width, r.row_stride_bytes = d.ctypes.data, d.shape[0], d.shape[1], d.strides[0]
            is_u16 = d.dtype == np.uint16
        keep.append(d)
        r.format = DEPTH_U16 if is_u16 else DEPTH_F32
        r.depth_scale = float(im.get("depth_scale", 0.001))
        r.fx, r.fy, r.cx, r.cy = float(im["fx"]), float(im["fy"]), float(im["cx"]), float(im["cy"])
        pose = np.asarray(im["pose"], np.float64).reshape(-1)
        assert pose.size == 12
        for q in range(12):
            r.pose[q] = float(pose[q])
    return recs, keep, on_device


def draw_samples(n_points: int, n_samples: int, seed: int) -> np.ndarray:
    """The sample list agh_localize draws on the device for sample_idx = NULL (include/agh.h): one index per stratum."""
    M = (1 << 64) - 1

    def splitmix64(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    out = np.empty(n_samples, np.int32)
    for k in range(n_samples):
        if n_points >= n_samples:
            lo, hi = (k * n_points) // n_samples, ((k + 1) * n_points) // n_samples
            out[k] = lo + splitmix64((seed ^ (k * 0x9E3779B97F4A7C15)) & M) % (hi - lo)
        else:
            out[k] = k if k < n_points else -(1 << 31)
    return out


def masked_samples(eligible, n_samples: int, seed: int) -> np.ndarray:
    """The sample list agh_localize_masked draws (include/agh.h): draw_samples' strata over the ascending list `eligible` of the
    eligible voxel indices; with fewer eligible voxels than samples the list itself, then INT32_MIN."""
    E = np.ascontiguousarray(eligible, np.int32)
    pos = draw_samples(E.shape[0], n_samples, seed)
    out = np.full(n_samples, -(1 << 31), np.int32)
    ok = pos >= 0
    out[ok] = E[pos[ok]]
    return out


class AghSampleMask(C.Structure):
    _fields_ = [("data", C.c_void_p), ("row_stride_bytes", C.c_int64)]


def sample_mask_records(masks, on_device: bool):
    """The agh_sample_mask records of a depth capture's masks: per image an (H, W) uint8 array whose rows may be padded (a torch
    CUDA tensor for the _device call), or None: no pixel of that image is eligible.  Returns (records, what keeps them alive)."""
    recs = (AghSampleMask * max(len(masks), 1))()
    keep = []
    for r, m in zip(recs, masks):
        if m is None:
            r.data, r.row_stride_bytes = None, 0
        elif on_device:
            assert m.is_cuda and m.dim() == 2 and m.stride(1) == 1 and m.element_size() == 1
            r.data, r.row_stride_bytes = m.data_ptr(), int(m.stride(0))
        else:
            assert isinstance(m, np.ndarray) and m.ndim == 2 and m.dtype in (np.uint8, np.bool_) and m.strides[1] == 1
            r.data, r.row_stride_bytes = m.ctypes.data, m.strides[0]
        keep.append(m)
    return recs, keep


def labeled_samples(eligible_lists, n_samples: int, seed: int) -> np.ndarray:
    """The sample list agh_localize_labeled draws (include/agh.h): masked_samples of every object's ascending list of eligible
    voxel indices with the one seed, object after object (n_objects x n_samples entries)."""
    if not len(eligible_lists) or n_samples == 0:
        return np.zeros(0, np.int32)
    return np.concatenate([masked_samples(E, n_samples, seed) for E in eligible_lists])


def batch_labeled_samples(eligible_lists, n_samples, seeds) -> np.ndarray:
    """The sample list agh_localize_batch_labeled draws (include/agh.h): labeled_samples of every capture, capture after
    capture.  eligible_lists[k]: capture k's per-object ascending lists of eligible CAPTURE-LOCAL voxel indices; n_samples and
    seeds: an int for all captures, or one per capture."""
    Ck = len(eligible_lists)
    per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * Ck
    parts = [labeled_samples(E, int(S), int(seed)) for E, S, seed in zip(eligible_lists, per(n_samples), per(seeds))]
    return np.concatenate(parts) if parts else np.zeros(0, np.int32)


class AghLabelImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("row_stride_bytes", C.c_int64)]


def label_image_records(labels, on_device: bool):
    """The agh_label_image records of a depth capture's label images: as sample_mask_records, the bytes being labels (0: no
    object, j + 1: object j), or None: no pixel of that image belongs to an object."""
    recs = (AghLabelImage * max(len(labels), 1))()
    keep = []
    for r, m in zip(recs, labels):
        if m is None:
            r.data, r.row_stride_bytes = None, 0
        elif on_device:
            assert m.is_cuda and m.dim() == 2 and m.stride(1) == 1 and m.element_size() == 1
            r.data, r.row_stride_bytes = m.data_ptr(), int(m.stride(0))
        else:
            assert isinstance(m, np.ndarray) and m.ndim == 2 and m.dtype == np.uint8 and m.strides[1] == 1
            r.data, r.row_stride_bytes = m.ctypes.data, m.strides[0]
        keep.append(m)
    return recs, keep


class AghPlaneParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("optimize", C.c_int32), ("distance_threshold", C.c_double),
                ("probability", C.c_double), ("seed", C.c_uint32), ("cam_ids_by_position", C.c_int32)]


class AghPlaneResult(C.Structure):
    _fields_ = [("coefficients", C.c_float * 4), ("n_inliers", C.c_int64), ("n_remaining", C.c_int64),
                ("iterations", C.c_int32), ("found", C.c_int32)]


def plane_replay(counts, n_points: int, max_iterations: int = 100, probability: float = 0.99):
    """RandomSampleConsensus::computeModel's termination over candidate inlier counts (agh_plane_replay, host only):
    returns (chosen candidate or -1, iterations)."""
    lib = load_library()
    cnt = np.ascontiguousarray(counts, np.int64)
    best, it = C.c_int32(0), C.c_int32(0)
    lib.agh_plane_replay(_p(cnt, C.c_int64), C.c_int64(cnt.size), C.c_int64(n_points), C.c_int32(max_iterations),
                         C.c_double(probability), C.byref(best), C.byref(it))
    return best.value, it.value


AGH_ERR_INVALID_ARGUMENT, AGH_ERR_HIP, AGH_ERR_CAPACITY, AGH_ERR_NO_CLOUD, AGH_ERR_NO_SVM, AGH_ERR_STATE = -1, -3, -4, -5, -6, -8
AGH_ERR_RETRY = -9  # the context adapted its configuration to the input (include/agh.h): repeat the call


class AghError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"agh error {code}: {msg}")
        self.code = code


def library_path() -> str:
    return os.path.join(_HERE, "lib", "libagile_grasp_hip.so")


def load_library():
    """dlopen the HIP library.  torch is imported first when available so that both share one HIP runtime."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                "agile_grasp_amd has no CPU implementation.")
        if os.environ.get("AGH_NO_TORCH") != "1":
            try:
                import torch  # noqa: F401  (loads torch's libamdhip64 first; ours then binds to the same runtime)
            except Exception:
                pass
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        lib.agh_last_error.restype = C.c_char_p
        lib.agh_last_error.argtypes = [C.c_void_p]
        lib.agh_selftest_math.restype = C.c_int64
        lib.agh_destroy.restype = None
        lib.agh_default_params.restype = None
        lib.agh_shard_slice.restype = None
        lib.agh_plane_replay.restype = None
        lib.agh_default_plane_params.restype = None
        lib.agh_default_cluster_params.restype = None
        lib.agh_default_plane_fit_params.restype = None
        lib.agh_default_depth_filter_params.restype = None
        lib.agh_default_depth_fusion_params.restype = None
        lib.agh_default_voxel_filter_params.restype = None
        lib.agh_default_hand_filter_params.restype = None
        lib.agh_default_hand_clearance_params.restype = None
        lib.agh_default_handle_ranking_params.restype = None
        _LIB = lib
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


_NO_FIT = object()  # localize_clustered's fp when the call is no fitted one (None there passes a NULL record)


class Context:
    """One agh_ctx: HandSearch + Learning::classify state for one cloud on one GPU."""

    def __init__(self, cam_origins, normals_mode: int = NORMALS_DETERMINISTIC, device: int = 0, profile: bool = False,
                 rand_seed: int = 1, **geometry):
        self.lib = load_library()
        p = AghParams()
        self.lib.agh_default_params(C.byref(p))
        for c in range(2):
            for r in range(3):
                p.cam_origin[c][r] = float(cam_origins[c][r])
        p.normals_mode, p.device, p.profile, p.rand_seed = normals_mode, device, int(profile), rand_seed
        for k, v in geometry.items():
            setattr(p, k, v)
        self.params = p
        self._h = C.c_void_p()
        rc = self.lib.agh_create(C.byref(p), C.byref(self._h))
        if rc != 0:
            raise AghError(rc, self.lib.agh_last_error(None).decode())
        self._keep = []  # device tensors that must outlive the context's use of them
        self._fuse_keep = {}  # slot -> the device frames of its last fuse_depth

    def close(self):
        if self._h:
            self.lib.agh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc < 0:
            raise AghError(rc, self.lib.agh_last_error(self._h).decode())
        return rc

    # ---- host-buffer API ----
    def set_cloud(self, xyz: np.ndarray, cam: np.ndarray | None):
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        stride = xyz.shape[1] * 4  # (numpy reports arbitrary strides for empty arrays)
        camp = None
        if cam is not None:
            cam = np.ascontiguousarray(cam, np.int32)
            camp = _p(cam, C.c_int32)
        self._check(self.lib.agh_set_cloud(self._h, _p(xyz, C.c_float), C.c_int64(stride), camp,
                                           C.c_int64(xyz.shape[0])))
        self.n = xyz.shape[0]

    def set_cloud_batch(self, clouds, cams):
        """A batch of clouds in one context: `clouds` / `cams` are lists of (n_k, 3) float32 / (n_k,) int32 arrays.  Returns
        the offsets; point and sample indices of later calls are positions in the concatenation."""
        xyz = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32)[:, :3] for c in clouds]), np.float32)
        cam = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32) for c in cams]), np.int32)
        off = np.zeros(len(clouds) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in clouds])
        self._check(self.lib.agh_set_cloud_batch(self._h, _p(xyz, C.c_float), C.c_int64(12), _p(cam, C.c_int32),
                                                 _p(off, C.c_int64), C.c_int32(len(clouds))))
        self.n = xyz.shape[0]
        return off

    def set_cloud_cam_origins(self, cam_origins):
        """agh_set_cloud_cam_origins: an (n_clouds, 2, 3) array of camera origins, row k for cloud k of the batch in place of
        the context's own; None clears the table.  Sticky until cleared or replaced."""
        if cam_origins is None:
            self._check(self.lib.agh_set_cloud_cam_origins(self._h, None, C.c_int32(0)))
            return
        tab = np.ascontiguousarray(cam_origins, np.float64)
        assert tab.ndim == 3 and tab.shape[1:] == (2, 3)
        self._check(self.lib.agh_set_cloud_cam_origins(self._h, _p(tab, C.c_double), C.c_int32(tab.shape[0])))

    def get_cloud_cam_origins(self):
        """The table set_cloud_cam_origins holds, (n_clouds, 2, 3) float64, or None."""
        tab = np.zeros((64, 2, 3), np.float64)
        k = self._check(self.lib.agh_get_cloud_cam_origins(self._h, _p(tab, C.c_double), C.c_int32(64)))
        return tab[:k].copy() if k > 0 else None

    def set_depth_filter(self, fp=None, **fields):
        """agh_set_depth_filter: every later deprojection of this context (deproject*, localize_depth*) rejects flying pixels,
        speckles and out-of-range readings.  `fp`: a depth_filter_params() record, or None for the defaults; the keyword fields
        (radius, min_support, max_jump_abs, max_jump_rel, z_min, z_max) are set on top.  Sticky until clear_depth_filter()."""
        rec = depth_filter_params()
        if fp is not None:
            C.memmove(C.byref(rec), C.byref(fp), C.sizeof(AghDepthFilterParams))
        for k, v in fields.items():
            if not hasattr(rec, k):
                raise TypeError(f"agh_depth_filter_params has no field {k}")
            setattr(rec, k, v)
        self._check(self.lib.agh_set_depth_filter(self._h, C.byref(rec)))

    def clear_depth_filter(self):
        self._check(self.lib.agh_set_depth_filter(self._h, None))

    def depth_filter(self):
        """The agh_depth_filter_params record held, or None."""
        rec = AghDepthFilterParams()
        return rec if self._check(self.lib.agh_get_depth_filter(self._h, C.byref(rec))) == 1 else None

    def depth_filter_counts(self) -> np.ndarray:
        """agh_get_depth_filter_counts: an (n_views, 4) int64 array, a row per view of the last deprojection in launch order --
        n_valid, n_out_of_range, n_unsupported, n_kept -- or an empty one if that deprojection ran without a filter."""
        recs = (AghDepthFilterCounts * 128)()
        k = self._check(self.lib.agh_get_depth_filter_counts(self._h, recs, C.c_int32(128)))
        return np.array([[r.n_valid, r.n_out_of_range, r.n_unsupported, r.n_kept] for r in recs[:k]], np.int64).reshape(k, 4)

    def fuse_depth(self, frames, slot: int = 0, **params):
        """agh_fuse_depth (torch CUDA tensors: agh_fuse_depth_device): the burst `frames` of ONE camera -- 1 to 16 image dicts
        as depth_image_records takes them, equal in everything but the pixels and the row stride -- fused into slot `slot`
        (0 .. 127) of this context; `params`: min_valid, max_spread_abs, max_spread_rel on top of the defaults.  Returns frame
        0's dict with `data` a DeviceImage: it goes into every localize_depth* form as a CUDA tensor does, with no
        synchronisation in between."""
        recs, keep, on_device = depth_image_records(frames)
        fp = depth_fusion_params(**params)
        out = AghDepthImage()
        fn = self.lib.agh_fuse_depth_device if on_device else self.lib.agh_fuse_depth
        self._check(fn(self._h, recs, C.c_int32(len(recs)), C.byref(fp), C.c_int32(slot), C.byref(out)))
        if on_device:  # (read until the next synchronisation: kept until the slot is fused again)
            self._fuse_keep[slot] = keep
        fused = dict(frames[0])
        fused["data"] = DeviceImage(out)
        if out.format == DEPTH_U16:
            fused["depth_scale"] = float(out.depth_scale)
        return fused

    def depth_fusion_counts(self, slot: int = 0):
        """agh_get_depth_fusion_counts: the slot's AghDepthFusionCounts record, or None if the slot was never fused."""
        rec = AghDepthFusionCounts()
        return rec if self._check(self.lib.agh_get_depth_fusion_counts(self._h, C.c_int32(slot), C.byref(rec))) == 1 else None

    def fused_depth(self, slot: int = 0):
        """agh_get_fused_depth: the slot's fused image, an (H, W) uint16 or float32 array, or None if the slot was never fused."""
        rec = AghDepthImage()
        rc = self.lib.agh_get_fused_depth(self._h, C.c_int32(slot), None, C.c_int64(0), C.byref(rec))  # (the record: the image's size)
        if rc != AGH_ERR_CAPACITY:
            self._check(rc)
            return None
        out = np.empty((rec.height, rec.width), np.uint16 if rec.format == DEPTH_U16 else np.float32)
        got = self._check(self.lib.agh_get_fused_depth(self._h, C.c_int32(slot), out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes), None))
        assert got == out.nbytes
        return out

    def set_voxel_filter(self, fp=None, **fields):
        """agh_set_voxel_filter: every later voxelisation of this context (preprocess*, every localize* form) prunes the voxels
        with fewer than min_neighbors occupied voxels of their own camera within `radius` voxels.  `fp`: a voxel_filter_params()
        record, or None for the defaults; the keyword fields (radius, min_neighbors) are set on top.  Sticky until
        clear_voxel_filter()."""
        rec = voxel_filter_params()
        if fp is not None:
            C.memmove(C.byref(rec), C.byref(fp), C.sizeof(AghVoxelFilterParams))
        for k, v in fields.items():
            if not hasattr(rec, k):
                raise TypeError(f"agh_voxel_filter_params has no field {k}")
            setattr(rec, k, v)
        self._check(self.lib.agh_set_voxel_filter(self._h, C.byref(rec)))

    def clear_voxel_filter(self):
        self._check(self.lib.agh_set_voxel_filter(self._h, None))

    def voxel_filter(self):
        """The agh_voxel_filter_params record held, or None."""
        rec = AghVoxelFilterParams()
        return rec if self._check(self.lib.agh_get_voxel_filter(self._h, C.byref(rec))) == 1 else None

    def voxel_filter_counts(self) -> np.ndarray:
        """agh_get_voxel_filter_counts: an (n_captures, 6) int64 array, a row per capture of the last voxelisation -- n_occupied,
        n_pruned, n_kept, each for camera 0 and camera 1 -- or an empty one if that voxelisation ran without a filter."""
        recs = (AghVoxelFilterCounts * 64)()
        k = self._check(self.lib.agh_get_voxel_filter_counts(self._h, recs, C.c_int32(64)))
        return np.array([list(r.n_occupied) + list(r.n_pruned) + list(r.n_kept) for r in recs[:k]], np.int64).reshape(k, 6)

    def set_hand_filter(self, fp=None, **fields):
        """agh_set_hand_filter: every later localize* chain of this context drops, between the search and the classifier, the
        hands outside an approach cone (approach_on, approach_dir, min_approach_cos), outside the gripper's stroke (width_on,
        min_width, max_width) or with fingers in space no depth image saw (view_on, probes_per_finger, depth_margin,
        max_unobserved; the depth forms only).  `fp`: a hand_filter_params() record, or None for the defaults (every criterion
        off); the keyword fields are set on top.  Sticky until clear_hand_filter()."""
        rec = hand_filter_params(**fields)
        if fp is not None:
            C.memmove(C.byref(rec), C.byref(fp), C.sizeof(AghHandFilterParams))
            for k, v in fields.items():
                setattr(rec, k, (C.c_double * 3)(*[float(x) for x in v]) if k == "approach_dir" else v)
        self._check(self.lib.agh_set_hand_filter(self._h, C.byref(rec)))

    def clear_hand_filter(self):
        self._check(self.lib.agh_set_hand_filter(self._h, None))

    def get_hand_filter(self):
        """The agh_hand_filter_params record held, or None."""
        rec = AghHandFilterParams()
        return rec if self._check(self.lib.agh_get_hand_filter(self._h, C.byref(rec))) == 1 else None

    def hand_filter_counts(self) -> np.ndarray:
        """agh_get_hand_filter_counts: an (n_lists, 5) int64 array, a row per list of the last chain in the order of its results
        -- n_hypotheses, n_dropped_approach, n_dropped_width, n_dropped_unobserved, n_kept -- or an empty one if that chain ran
        without a filter."""
        recs = (AghHandFilterCounts * 64)()
        k = self._check(self.lib.agh_get_hand_filter_counts(self._h, recs, C.c_int32(64)))
        return np.array([[r.n_hypotheses, r.n_dropped_approach, r.n_dropped_width, r.n_dropped_unobserved, r.n_kept]
                         for r in recs[:k]], np.int64).reshape(k, 5)

    def set_hand_clearance(self, cp=None, **fields):
        """agh_set_hand_clearance: every later localize* chain of this context drops, between the search and the classifier and
        behind the hand filter, the hands whose approach corridor -- the oriented box near_offset .. far_offset behind the palm,
        +- half_width along the binormal, +- half_height along the axis -- holds more than max_points points of the capture's own
        voxelised cloud.  `cp`: a hand_clearance_params() record, or None for the defaults (0, 0.12, 0.05, 0.04, 0); the keyword
        fields are set on top.  Sticky until clear_hand_clearance()."""
        rec = hand_clearance_params(**fields)
        if cp is not None:
            C.memmove(C.byref(rec), C.byref(cp), C.sizeof(AghHandClearanceParams))
            for k, v in fields.items():
                setattr(rec, k, v)
        self._check(self.lib.agh_set_hand_clearance(self._h, C.byref(rec)))

    def clear_hand_clearance(self):
        self._check(self.lib.agh_set_hand_clearance(self._h, None))

    def get_hand_clearance(self):
        """The agh_hand_clearance_params record held, or None."""
        rec = AghHandClearanceParams()
        return rec if self._check(self.lib.agh_get_hand_clearance(self._h, C.byref(rec))) == 1 else None

    def hand_clearance_counts(self) -> np.ndarray:
        """agh_get_hand_clearance_counts: an (n_lists, 3) int64 array, a row per list of the last chain in the order of its results
        -- n_tested, n_dropped, n_kept -- or an empty one if that chain ran without a clearance."""
        recs = (AghHandClearanceCounts * 64)()
        k = self._check(self.lib.agh_get_hand_clearance_counts(self._h, recs, C.c_int32(64)))
        return np.array([[r.n_tested, r.n_dropped, r.n_kept] for r in recs[:k]], np.int64).reshape(k, 3)

    def set_handle_ranking(self, rp=None, **fields):
        """agh_set_handle_ranking: every later localize* chain of this context returns each list's handles in rank order -- score
        descending, NaN last, ties by the position in the unranked list, the handles below min_score left out, at most max_handles
        of them.  `rp`: a handle_ranking_params() record, or None for the defaults (support and margin, weight 1 each); the keyword
        fields are set on top.  Sticky until clear_handle_ranking()."""
        rec = handle_ranking_params(**fields)
        if rp is not None:
            given = rec
            rec = AghHandleRankingParams()
            C.memmove(C.byref(rec), C.byref(rp), C.sizeof(AghHandleRankingParams))
            for k in fields:
                setattr(rec, k, getattr(given, k))
        self._check(self.lib.agh_set_handle_ranking(self._h, C.byref(rec)))

    def clear_handle_ranking(self):
        self._check(self.lib.agh_set_handle_ranking(self._h, None))

    def get_handle_ranking(self):
        """The agh_handle_ranking_params record held, or None."""
        rec = AghHandleRankingParams()
        return rec if self._check(self.lib.agh_get_handle_ranking(self._h, C.byref(rec))) == 1 else None

    def handle_scores(self, cap: int = 8192 * 64) -> np.ndarray:
        """agh_get_handle_scores: the score records of the last chain's handles (SCORE_DTYPE), laid out as its handles_out."""
        out = np.zeros(max(cap, 1), SCORE_DTYPE)
        n = self._check(self.lib.agh_get_handle_scores(self._h, out.ctypes.data_as(C.c_void_p), C.c_int64(cap)))
        return out[:n].copy()

    def handle_ranking_counts(self) -> np.ndarray:
        """agh_get_handle_ranking_counts: an (n_lists, 3) int64 array, a row per list of the last chain -- n_found, n_below,
        n_returned."""
        recs = (AghHandleRankingCounts * 64)()
        k = self._check(self.lib.agh_get_handle_ranking_counts(self._h, recs, C.c_int32(64)))
        return np.array([[r.n_found, r.n_below, r.n_returned] for r in recs[:k]], np.int64).reshape(k, 3)

    def hand_margins(self, cap: int = 8192 * 64) -> np.ndarray:
        """agh_get_hand_margins: minus the classifier's decision sum of every hand of the last chain, laid out as its hands_out."""
        out = np.zeros(max(cap, 1), np.float64)
        n = self._check(self.lib.agh_get_hand_margins(self._h, _p(out, C.c_double), C.c_int64(cap)))
        return out[:n].copy()

    def rank_handles(self, rp, hands, margins, handles, inlier_idx, cap=None):
        """agh_rank_handles: the ranking `rp` (a handle_ranking_params() record) on one list in host buffers, by the chains' kernel.
        Returns (handles in rank order, their SCORE_DTYPE records, [n_found, n_below, n_returned])."""
        hands = np.ascontiguousarray(hands, HYP_DTYPE)
        handles = np.ascontiguousarray(handles, HANDLE_DTYPE)
        idx = np.ascontiguousarray(inlier_idx, np.int32)
        if margins is not None:
            margins = np.ascontiguousarray(margins, np.float64)
            assert margins.shape[0] == hands.shape[0]
        cap = handles.shape[0] if cap is None else cap
        out, sc = np.zeros(max(cap, 1), HANDLE_DTYPE), np.zeros(max(cap, 1), SCORE_DTYPE)
        counts = AghHandleRankingCounts()
        rc = self.lib.agh_rank_handles(self._h, C.byref(rp) if rp is not None else None, hands.ctypes.data_as(C.c_void_p),
                                       C.c_int64(hands.shape[0]), _p(margins, C.c_double) if margins is not None else None,
                                       handles.ctypes.data_as(C.c_void_p), C.c_int64(handles.shape[0]), _p(idx, C.c_int32),
                                       C.c_int64(idx.shape[0]), out.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                                       C.c_int64(cap), C.byref(counts))
        self.last_rank_counts = [counts.n_found, counts.n_below, counts.n_returned]
        self._check(rc)
        n = counts.n_returned
        return out[:n].copy(), sc[:n].copy(), list(self.last_rank_counts)

    def set_cloud_batch_torch(self, xyz_t, cam_t, offsets, stream=None):
        assert xyz_t.is_cuda and xyz_t.is_contiguous()
        off = np.ascontiguousarray(offsets, np.int64)
        self._keep = [xyz_t, cam_t]
        self.n = xyz_t.shape[0]
        self._check(self.lib.agh_set_cloud_batch_device(
            self._h, C.c_void_p(xyz_t.data_ptr()), C.c_int64(xyz_t.stride(0) * 4),
            C.c_void_p(cam_t.data_ptr()) if cam_t is not None else None, _p(off, C.c_int64), C.c_int32(off.shape[0] - 1),
            C.c_void_p(stream) if stream else None))

    def preprocess(self, xyz: np.ndarray, size_left: int, workspace, cell_size: float = 0.003, dense: bool = False) -> int:
        """NaN removal + workspace box + per-camera voxelisation on the GPU; the result becomes the context's cloud."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        ws = np.ascontiguousarray(workspace, np.float64)
        assert ws.size == 6
        nv = C.c_int64(0)
        self._check(self.lib.agh_preprocess(self._h, _p(xyz, C.c_float), C.c_int64(xyz.shape[1] * 4),
                                            C.c_int64(xyz.shape[0]), C.c_int64(size_left), C.c_int(1 if dense else 0),
                                            _p(ws, C.c_double), C.c_double(cell_size), C.byref(nv)))
        self.n = nv.value
        return nv.value

    def preprocess_torch(self, xyz_t, size_left: int, workspace, cell_size: float = 0.003, dense: bool = False,
                         stream=None) -> int:
        assert xyz_t.is_cuda and xyz_t.is_contiguous()
        ws = np.ascontiguousarray(workspace, np.float64)
        nv = C.c_int64(0)
        self._keep = [xyz_t]
        self._check(self.lib.agh_preprocess_device(
            self._h, C.c_void_p(xyz_t.data_ptr()), C.c_int64(xyz_t.stride(0) * 4), C.c_int64(xyz_t.shape[0]),
            C.c_int64(size_left), C.c_int(1 if dense else 0), _p(ws, C.c_double), C.c_double(cell_size), C.byref(nv),
            C.c_void_p(stream) if stream else None))
        self.n = nv.value
        return nv.value

    def find_handles(self, hands: np.ndarray, min_inliers: int = 3, min_length: float = 0.005):
        """HandleSearch::findHandles on hypothesis records; returns (handles, concatenated inlier indices)."""
        hands = np.ascontiguousarray(hands, HYP_DTYPE)
        H = hands.shape[0]
        out = np.zeros(max(H, 1), HANDLE_DTYPE)
        idx = np.zeros(max(H, 1), np.int32)
        n = C.c_int64(0)
        self._check(self.lib.agh_find_handles(self._h, hands.ctypes.data_as(C.c_void_p), C.c_int64(H), C.c_int32(min_inliers),
                                              C.c_double(min_length), out.ctypes.data_as(C.c_void_p), C.c_int64(out.shape[0]),
                                              _p(idx, C.c_int32), C.c_int64(idx.shape[0]), C.byref(n)))
        out = out[:n.value].copy()
        return out, idx[:int(out["n_inliers"].sum())].copy()

    def localize(self, xyz, size_left: int, workspace, samples=None, n_samples: int = 0, sample_seed: int = 1,
                 classify: bool = True, min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003,
                 dense: bool = False, phase: str = "both", filters_boundaries: bool = False):
        """agh_localize: raw capture -> voxels -> search -> SVM -> handles in one call with one synchronisation
        (grasp_localizer.cpp:95-103).  `samples`: indices into the voxelised cloud, or None: n_samples are drawn on the device.
        filters_boundaries: Localization::filterHands (hands within 2 cm of a face of `workspace` dropped) between the search
        and the classifier; an int passes through as is (the library refuses anything but 0 and 1).
        Returns a dict: handles, inlier_idx, hands (what the handle search ran on), samples, n_voxels, n_hypotheses."""
        on_device = hasattr(xyz, "is_cuda") and xyz.is_cuda  # a torch CUDA tensor (N, >= 3) float32: agh_localize_device
        if on_device:
            assert xyz.is_contiguous() and xyz.dim() == 2 and xyz.shape[1] >= 3
            xyz_ptr, n_pts, stride_b = C.c_void_p(xyz.data_ptr()), int(xyz.shape[0]), int(xyz.stride(0)) * 4
        else:
            xyz = np.ascontiguousarray(xyz, np.float32)
            assert xyz.ndim == 2 and xyz.shape[1] >= 3
            xyz_ptr, n_pts, stride_b = _p(xyz, C.c_float), xyz.shape[0], xyz.shape[1] * 4
        lp, samples, S, hcap = self._localize_params(size_left, workspace, samples, n_samples, sample_seed, classify, min_inliers,
                                                     min_length, cell_size, dense, filters_boundaries)
        if phase == "begin":  # agh_localize_begin: everything queued; localize_end() collects
            assert not on_device
            self._check(self.lib.agh_localize_begin(self._h, xyz_ptr, C.c_int64(stride_b), C.c_int64(n_pts), C.byref(lp)))
            self._loc_keep = (xyz, samples, lp)  # (the capture must stay valid until the end call)
            self._loc_S = S  # (like _loc_keep only once the chain is queued: a refused begin leaves the one in flight its own)
            return None
        fn = self.lib.agh_localize_device if on_device else self.lib.agh_localize
        return self._localize_blocking(fn, (xyz_ptr, C.c_int64(stride_b), C.c_int64(n_pts)), lp, S, hcap)

    def _localize_blocking(self, fn, capture_args, lp, S, hcap):
        """The tail of the one-call forms: the output buffers, the blocking library call, the result dict."""
        handles, idx, hands, sout = self._loc_bufs
        res = AghLocalizeResult()
        self._check(fn(self._h, *capture_args, C.byref(lp), handles.ctypes.data_as(C.c_void_p), C.c_int64(hcap),
                       _p(idx, C.c_int32), C.c_int64(hcap), hands.ctypes.data_as(C.c_void_p), C.c_int64(hcap), _p(sout, C.c_int32),
                       C.byref(res)))
        return self._localize_result(res, S)

    def _localize_params(self, size_left, workspace, samples, n_samples, sample_seed, classify, min_inliers, min_length, cell_size,
                         dense, filters_boundaries):
        """The agh_localize_params record of a single-capture chain, and output buffers large enough for it (self._loc_bufs)."""
        lp = AghLocalizeParams()
        lp.size_left, lp.dense, lp.classify = size_left, 1 if dense else 0, 1 if classify else 0
        ws = np.ascontiguousarray(workspace, np.float64)
        assert ws.size == 6
        for k in range(6):
            lp.workspace[k] = float(ws[k])
        lp.cell_size = cell_size
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.int32)
            lp.sample_idx = samples.ctypes.data_as(C.POINTER(C.c_int32))
            S = samples.shape[0]
        else:
            lp.sample_idx = None
            S = int(n_samples)
        lp.n_samples, lp.sample_seed, lp.min_inliers, lp.min_length = S, sample_seed, min_inliers, min_length
        lp.filters_boundaries = int(filters_boundaries)
        bufs = getattr(self, "_loc_bufs", None)
        hcap = max(min(8 * S, 8192), 1)
        if bufs is None or bufs[0].shape[0] < hcap or bufs[3].shape[0] < max(S, 1):
            self._loc_bufs = (np.zeros(hcap, HANDLE_DTYPE), np.zeros(hcap, np.int32), np.zeros(hcap, HYP_DTYPE),
                              np.zeros(max(S, 1), np.int32))
        return lp, samples, S, hcap

    def deproject(self, images) -> np.ndarray:
        """agh_deproject: the points k_deproject makes of a capture's depth images (see depth_image_records), (sum W x H, 3)
        float32, image 0 first, pixels row-major, invalid pixels NaN."""
        recs, _keep, on_device = depth_image_records(images)
        assert not on_device
        n = sum(int(r.width) * int(r.height) for r in recs)
        out = np.empty((n, 3), np.float32)
        got = self._check(self.lib.agh_deproject(self._h, recs, C.c_int32(len(recs)), _p(out, C.c_float), C.c_int64(n)))
        assert got == n
        return out

    def localize_depth(self, images, workspace, samples=None, n_samples: int = 0, sample_seed: int = 1, classify: bool = True,
                       min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003, phase: str = "both",
                       filters_boundaries: bool = False):
        """agh_localize_depth (torch CUDA tensors: agh_localize_depth_device): localize() straight from one or two depth images
        (see depth_image_records); image k is camera k.  phase="begin": agh_localize_depth_begin, collected by localize_end()."""
        recs, keep, on_device = depth_image_records(images)
        lp, samples, S, hcap = self._localize_params(0, workspace, samples, n_samples, sample_seed, classify, min_inliers, min_length,
                                                     cell_size, False, filters_boundaries)
        if phase == "begin":
            assert not on_device
            self._check(self.lib.agh_localize_depth_begin(self._h, recs, C.c_int32(len(recs)), C.byref(lp)))
            self._loc_keep = (keep, samples, lp)  # (the pixel buffers must stay valid until the end call)
            self._loc_S = S
            return None
        fn = self.lib.agh_localize_depth_device if on_device else self.lib.agh_localize_depth
        return self._localize_blocking(fn, (recs, C.c_int32(len(recs))), lp, S, hcap)

    def localize_masked(self, xyz, size_left: int, workspace, mask, n_samples: int = 0, sample_seed: int = 1, classify: bool = True,
                        min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003, dense: bool = False,
                        phase: str = "both", filters_boundaries: bool = False, samples=None):
        """agh_localize_masked (torch CUDA tensors: agh_localize_masked_device): localize() with its n_samples drawn among the
        voxels that hold a kept raw point with a non-zero byte in `mask` (one uint8 per raw point; None passes NULL, and
        `samples` goes through for the library to refuse).  phase="begin": agh_localize_masked_begin, collected by
        localize_end().  sample_mask_count() then gives the number of eligible voxels."""
        on_device = hasattr(xyz, "is_cuda") and xyz.is_cuda
        if on_device:
            assert xyz.is_contiguous() and xyz.dim() == 2 and xyz.shape[1] >= 3
            xyz_ptr, n_pts, stride_b = C.c_void_p(xyz.data_ptr()), int(xyz.shape[0]), int(xyz.stride(0)) * 4
            if mask is not None:
                assert mask.is_cuda and mask.dim() == 1 and mask.element_size() == 1 and mask.shape[0] == n_pts
                assert n_pts <= 1 or mask.stride(0) == 1
            mask_ptr = C.c_void_p(mask.data_ptr()) if mask is not None else None
        else:
            xyz = np.ascontiguousarray(xyz, np.float32)
            assert xyz.ndim == 2 and xyz.shape[1] >= 3
            xyz_ptr, n_pts, stride_b = _p(xyz, C.c_float), xyz.shape[0], xyz.shape[1] * 4
            if mask is not None:
                mask = np.ascontiguousarray(mask).view(np.uint8) if np.asarray(mask).dtype == np.bool_ else np.ascontiguousarray(mask, np.uint8)
                assert mask.shape == (n_pts,)
            mask_ptr = C.c_void_p(mask.ctypes.data) if mask is not None else None
        lp, samples, S, hcap = self._localize_params(size_left, workspace, samples, n_samples, sample_seed, classify, min_inliers,
                                                     min_length, cell_size, dense, filters_boundaries)
        if phase == "begin":
            assert not on_device
            self._check(self.lib.agh_localize_masked_begin(self._h, xyz_ptr, C.c_int64(stride_b), C.c_int64(n_pts), mask_ptr,
                                                           C.byref(lp)))
            self._loc_keep = (xyz, mask, samples, lp)
            self._loc_S = S
            return None
        fn = self.lib.agh_localize_masked_device if on_device else self.lib.agh_localize_masked
        return self._localize_blocking(fn, (xyz_ptr, C.c_int64(stride_b), C.c_int64(n_pts), mask_ptr), lp, S, hcap)

    def localize_depth_masked(self, images, masks, workspace, n_samples: int = 0, sample_seed: int = 1, classify: bool = True,
                              min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003, phase: str = "both",
                              filters_boundaries: bool = False, samples=None):
        """agh_localize_depth_masked (torch CUDA tensors: agh_localize_depth_masked_device): localize_depth() with its samples
        drawn under per-image masks (see sample_mask_records; `masks` None passes NULL).  phase="begin":
        agh_localize_depth_masked_begin, collected by localize_end()."""
        recs, keep, on_device = depth_image_records(images)
        mrecs, mkeep = sample_mask_records(masks, on_device) if masks is not None else (None, [])
        lp, samples, S, hcap = self._localize_params(0, workspace, samples, n_samples, sample_seed, classify, min_inliers, min_length,
                                                     cell_size, False, filters_boundaries)
        if phase == "begin":
            assert not on_device
            self._check(self.lib.agh_localize_depth_masked_begin(self._h, recs, mrecs, C.c_int32(len(recs)), C.byref(lp)))
            self._loc_keep = (keep, mkeep, samples, lp)
            self._loc_S = S
            return None
        fn = self.lib.agh_localize_depth_masked_device if on_device else self.lib.agh_localize_depth_masked
        return self._localize_blocking(fn, (recs, mrecs, C.c_int32(len(recs))), lp, S, hcap)

    def sample_mask_count(self) -> int:
        """agh_get_sample_mask_count: the eligible voxels of the last masked chain this context collected."""
        m = C.c_int64(0)
        self._check(self.lib.agh_get_sample_mask_count(self._h, C.byref(m)))
        return m.value

    def _localize_labeled(self, fn, capture_args, n_objects, lp, S, caps):
        """The tail of the labelled forms: the blocking call and one dict per object, as localize_batch's per capture."""
        K = int(n_objects)
        a = {"Ck": K if 1 <= K <= 64 else 0, "S_list": [S] * (K if 1 <= K <= 64 else 0)}
        out = self._batch_collect(a, caps, lambda *o: fn(self._h, *capture_args, C.c_int32(K), C.byref(lp), *o))
        self.n = out[0]["n_voxels"] if out else 0  # (one cloud, whose voxel count every object reports)
        return out

    def localize_labeled(self, xyz, size_left: int, workspace, labels, n_objects: int, n_samples: int = 0, sample_seed: int = 1,
                         classify: bool = True, min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003,
                         dense: bool = False, filters_boundaries: bool = False, samples=None, caps=None):
        """agh_localize_labeled (torch CUDA tensors: agh_localize_labeled_device): one capture, one label byte per raw point (0:
        no object, j + 1: object j), n_samples drawn for EACH of the n_objects objects among its own eligible voxels; one search,
        one handle search per object side by side, one synchronisation.  Returns a list of n_objects dicts shaped like
        localize_batch's; object j's equal localize_masked(mask = labels == j + 1).  label_counts() then gives the M_j.
        (`labels` None passes NULL and `samples` goes through, for the library to refuse.)"""
        on_device = hasattr(xyz, "is_cuda") and xyz.is_cuda
        if on_device:
            assert xyz.is_contiguous() and xyz.dim() == 2 and xyz.shape[1] >= 3
            xyz_ptr, n_pts, stride_b = C.c_void_p(xyz.data_ptr()), int(xyz.shape[0]), int(xyz.stride(0)) * 4
            if labels is not None:
                assert labels.is_cuda and labels.dim() == 1 and labels.element_size() == 1 and labels.shape[0] == n_pts
                assert n_pts <= 1 or labels.stride(0) == 1
            lab_ptr = C.c_void_p(labels.data_ptr()) if labels is not None else None
        else:
            xyz = np.ascontiguousarray(xyz, np.float32)
            assert xyz.ndim == 2 and xyz.shape[1] >= 3
            xyz_ptr, n_pts, stride_b = _p(xyz, C.c_float), xyz.shape[0], xyz.shape[1] * 4
            if labels is not None:
                labels = np.ascontiguousarray(labels, np.uint8)
                assert labels.shape == (n_pts,)
            lab_ptr = C.c_void_p(labels.ctypes.data) if labels is not None else None
        lp, samples, S, _ = self._localize_params(size_left, workspace, samples, n_samples, sample_seed, classify, min_inliers,
                                                  min_length, cell_size, dense, filters_boundaries)
        fn = self.lib.agh_localize_labeled_device if on_device else self.lib.agh_localize_labeled
        return self._localize_labeled(fn, (xyz_ptr, C.c_int64(stride_b), C.c_int64(n_pts), lab_ptr), n_objects, lp, S, caps)

    def localize_depth_labeled(self, images, labels, workspace, n_objects: int, n_samples: int = 0, sample_seed: int = 1,
                               classify: bool = True, min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003,
                               filters_boundaries: bool = False, samples=None, caps=None):
        """agh_localize_depth_labeled (torch CUDA tensors: agh_localize_depth_labeled_device): localize_labeled() straight from
        depth images with one label image per depth image (see label_image_records; `labels` None passes NULL)."""
        recs, keep, on_device = depth_image_records(images)
        lrecs, lkeep = label_image_records(labels, on_device) if labels is not None else (None, [])
        lp, samples, S, _ = self._localize_params(0, workspace, samples, n_samples, sample_seed, classify, min_inliers, min_length,
                                                  cell_size, False, filters_boundaries)
        fn = self.lib.agh_localize_depth_labeled_device if on_device else self.lib.agh_localize_depth_labeled
        return self._localize_labeled(fn, (recs, lrecs, C.c_int32(len(recs))), n_objects, lp, S, caps)

    # ---- clusters as the label source (include/agh.h, agh_localize_clustered*) ----
    def _localize_clustered(self, fn, capture_args, cp, lp, S, caps, fp=()):
        """(fp: a one-tuple with the agh_plane_fit_params record, or None for NULL, of a fitted call)"""
        K = int(cp.max_objects) if cp is not None else 0
        a = {"Ck": K if 1 <= K <= 64 else 0, "S_list": [S] * (K if 1 <= K <= 64 else 0)}
        cp_arg = C.byref(cp) if cp is not None else None
        fp_args = tuple(C.byref(f) if f is not None else None for f in fp)
        out = self._batch_collect(a, caps, lambda *o: fn(self._h, *capture_args, *fp_args, cp_arg, C.byref(lp), *o))
        self.n = out[0]["n_voxels"] if out else 0
        return out

    def localize_clustered(self, xyz, size_left: int, workspace, cp, n_samples: int = 0, sample_seed: int = 1,
                           classify: bool = True, min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003,
                           dense: bool = False, filters_boundaries: bool = False, samples=None, caps=None, fp=_NO_FIT):
        """agh_localize_clustered (torch CUDA tensors: agh_localize_clustered_device): localize_labeled() whose objects are the
        connected components of the voxels above the support plane of `cp` (cluster_params(); None passes NULL), found on the
        device inside the call.  Returns cp.max_objects dicts; cluster_info() and cluster_labels() then describe the objects.
        (`samples` goes through, for the library to refuse.)"""
        on_device = hasattr(xyz, "is_cuda") and xyz.is_cuda
        if on_device:
            assert xyz.dim() == 2 and xyz.shape[1] >= 3 and xyz.stride(1) == 1
            xyz_ptr, n_pts, stride_b = C.c_void_p(xyz.data_ptr()), int(xyz.shape[0]), int(xyz.stride(0)) * 4
        else:
            xyz = np.ascontiguousarray(xyz, np.float32)
            assert xyz.ndim == 2 and xyz.shape[1] >= 3
            xyz_ptr, n_pts, stride_b = _p(xyz, C.c_float), xyz.shape[0], xyz.shape[1] * 4
        lp, samples, S, _ = self._localize_params(size_left, workspace, samples, n_samples, sample_seed, classify, min_inliers,
                                                  min_length, cell_size, dense, filters_boundaries)
        if fp is not _NO_FIT:
            fn = self.lib.agh_localize_clustered_fit_device if on_device else self.lib.agh_localize_clustered_fit
            return self._localize_clustered(fn, (xyz_ptr, C.c_int64(stride_b), C.c_int64(n_pts)), cp, lp, S, caps, (fp,))
        fn = self.lib.agh_localize_clustered_device if on_device else self.lib.agh_localize_clustered
        return self._localize_clustered(fn, (xyz_ptr, C.c_int64(stride_b), C.c_int64(n_pts)), cp, lp, S, caps)

    def localize_depth_clustered(self, images, workspace, cp, n_samples: int = 0, sample_seed: int = 1, classify: bool = True,
                                 min_inliers: int = 3, min_length: float = 0.005, cell_size: float = 0.003,
                                 filters_boundaries: bool = False, samples=None, caps=None, fp=_NO_FIT):
        """agh_localize_depth_clustered (torch CUDA tensors: agh_localize_depth_clustered_device): localize_clustered() straight
        from depth images (see depth_image_records)."""
        recs, keep, on_device = depth_image_records(images)
        lp, samples, S, _ = self._localize_params(0, workspace, samples, n_samples, sample_seed, classify, min_inliers, min_length,
                                                  cell_size, False, filters_boundaries)
        if fp is not _NO_FIT:
            fn = self.lib.agh_localize_depth_clustered_fit_device if on_device else self.lib.agh_localize_depth_clustered_fit
            return self._localize_clustered(fn, (recs, C.c_int32(len(recs))), cp, lp, S, caps, (fp,))
        fn = self.lib.agh_localize_depth_clustered_device if on_device else self.lib.agh_localize_depth_clustered
        return self._localize_clustered(fn, (recs, C.c_int32(len(recs))), cp, lp, S, caps)

    # ---- a fitted plane for the clustered chain (include/agh.h, agh_localize_clustered_fit*) ----
    def localize_clustered_fit(self, xyz, size_left: int, workspace, fp, cp, **kw):
        """agh_localize_clustered_fit (torch CUDA tensors: agh_localize_clustered_fit_device): localize_clustered() with the
        support plane found on the device inside the call (`fp`: plane_fit_params(); None passes NULL); cp.plane is not read.
        plane_fit() and plane_fit_candidates() then describe the fit, cluster_info() and cluster_labels() the objects."""
        return self.localize_clustered(xyz, size_left, workspace, cp, fp=fp, **kw)

    def localize_depth_clustered_fit(self, images, workspace, fp, cp, **kw):
        """agh_localize_depth_clustered_fit (torch CUDA tensors: agh_localize_depth_clustered_fit_device): localize_clustered_fit()
        straight from depth images (see depth_image_records)."""
        return self.localize_depth_clustered(images, workspace, cp, fp=fp, **kw)

    def plane_fit(self) -> dict:
        """agh_get_plane_fit of the last fitted chain this context collected: plane (four doubles, zeros without a plane),
        n_voxels, n_inliers, n_refit, best_candidate (-1: none), found, refined."""
        r = AghPlaneFitResult()
        self._check(self.lib.agh_get_plane_fit(self._h, C.byref(r)))
        return {"plane": np.array(list(r.plane), np.float64), "n_voxels": r.n_voxels, "n_inliers": r.n_inliers, "n_refit": r.n_refit,
                "best_candidate": r.best_candidate, "found": r.found, "refined": r.refined}

    def plane_fit_candidates(self, cap: int = 256) -> dict:
        """agh_get_plane_fit_candidates: per candidate of the last fitted chain its three voxel indices (`idx`, (C, 3)), its plane
        before refit and orientation (`planes`, (C, 4)) and its inlier count (`counts`)."""
        idx = np.zeros((max(cap, 1), 3), np.int32)
        planes = np.zeros((max(cap, 1), 4), np.float64)
        counts = np.zeros(max(cap, 1), np.int64)
        n = self._check(self.lib.agh_get_plane_fit_candidates(self._h, _p(idx, C.c_int32), _p(planes, C.c_double), _p(counts, C.c_int64),
                                                              C.c_int32(cap)))
        return {"idx": idx[:n].copy(), "planes": planes[:n].copy(), "counts": counts[:n].copy()}

    def cluster_info(self, cap_objects: int = 64):
        """agh_get_cluster_info of the last clustered chain this context collected: a dict with n_foreground, n_components,
        n_objects, and per list of the call n_voxels (M_j) and ids (the object's smallest voxel index, -1: none)."""
        info = AghClusterInfo()
        m = np.full(max(cap_objects, 1), -2, np.int64)
        ids = np.full(max(cap_objects, 1), -2, np.int32)
        self._check(self.lib.agh_get_cluster_info(self._h, C.byref(info), _p(m, C.c_int64), _p(ids, C.c_int32), C.c_int32(cap_objects)))
        return {"n_foreground": info.n_foreground, "n_components": info.n_components, "n_objects": info.n_objects,
                "n_voxels": m[m > -2].copy(), "ids": ids[ids > -2].copy()}

    def cluster_labels(self, cap: int | None = None) -> np.ndarray:
        """agh_get_cluster_labels: per voxel of the bound cloud 0 or object + 1, of the last clustered chain collected."""
        cap = int(self.n) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), np.uint8)
        nv = self._check(self.lib.agh_get_cluster_labels(self._h, C.c_void_p(out.ctypes.data), C.c_int64(cap)))
        return out[:nv].copy()

    def label_counts(self, cap_objects: int = 64) -> np.ndarray:
        """agh_get_label_counts: the eligible voxels M_j of every object of the last labelled chain this context collected."""
        m = np.full(max(cap_objects, 1), -1, np.int64)  # (the call writes n_objects counts, none of them negative)
        self._check(self.lib.agh_get_label_counts(self._h, _p(m, C.c_int64), C.c_int32(cap_objects)))
        return m[m >= 0].copy()

    def localize_depth_begin(self, images, workspace, **kw):
        """agh_localize_depth_begin: the chain of this capture queued, nothing waited for; localize_end() collects it."""
        return self.localize_depth(images, workspace, phase="begin", **kw)

    def localize_depth_stage(self, images):
        """agh_localize_depth_stage: the NEXT capture's images up on a second stream, beside the chain in flight.  Pass images
        with the same pixel arrays to the next localize_depth_begin (the library recognises the set by pointers, sizes, strides
        and formats)."""
        recs, keep, on_device = depth_image_records(images)
        assert not on_device
        self._stage_keep = keep
        self._check(self.lib.agh_localize_depth_stage(self._h, recs, C.c_int32(len(recs))))

    @staticmethod
    def depth_batch_records(captures):
        """The flat agh_depth_image array of a batch and its n_images: `captures` is a list of image lists (see
        depth_image_records), capture k's images are the next n_images[k] records.  Returns (records, n_images, what keeps the
        pixel buffers alive, on_device); torch CUDA tensors as `data` (in every image) select the device form."""
        flat = [im for images in captures for im in images]
        recs, keep, on_device = depth_image_records(flat)
        n_images = (C.c_int32 * max(len(captures), 1))(*[len(images) for images in captures])
        return recs, n_images, keep, on_device

    def deproject_batch(self, captures) -> np.ndarray:
        """agh_deproject_batch: the points k_deproject_batch makes of a batch of captures' depth images, (sum W x H, 3) float32,
        capture after capture, each as deproject() returns it."""
        recs, n_images, _keep, on_device = self.depth_batch_records(captures)
        assert not on_device
        n = sum(int(r.width) * int(r.height) for r in recs)
        out = np.empty((n, 3), np.float32)
        got = self._check(self.lib.agh_deproject_batch(self._h, recs, n_images, C.c_int32(len(captures)), _p(out, C.c_float),
                                                       C.c_int64(n)))
        assert got == n
        return out

    def _depth_batch_args(self, captures, workspaces, kw):
        recs, n_images, keep, on_device = self.depth_batch_records(captures)
        a = self._batch_args([], 0, workspaces, kw.pop("samples", None), kw.pop("n_samples", 0), kw.pop("sample_seeds", None),
                             kw.pop("classify", True), kw.pop("min_inliers", 3), kw.pop("min_length", 0.005),
                             kw.pop("filters_boundaries", 0), kw.pop("cell_size", 0.003), False, Ck=len(captures))
        assert not kw, f"unknown arguments {sorted(kw)}"
        a.update(recs=recs, n_images=n_images, keep=keep, on_device=on_device)
        return a

    def localize_depth_batch(self, captures, workspaces, caps=None, **kw):
        """agh_localize_depth_batch (torch CUDA tensors as `data`: agh_localize_depth_batch_device): localize_batch() straight
        from depth images.  `captures`: a list of image lists (one or two images each, see depth_image_records); image j of a
        capture is its camera j.  workspaces, samples, n_samples, sample_seeds, classify, min_inliers, min_length,
        filters_boundaries, cell_size and caps as for localize_batch.  Returns a list of dicts, one per capture."""
        a = self._depth_batch_args(captures, workspaces, kw)
        fn = self.lib.agh_localize_depth_batch_device if a["on_device"] else self.lib.agh_localize_depth_batch
        return self._batch_collect(a, caps, lambda *out: fn(self._h, a["recs"], a["n_images"], a["lps"], C.c_int32(a["Ck"]), *out))

    def localize_depth_batch_begin(self, captures, workspaces, **kw):
        """agh_localize_depth_batch_begin (torch CUDA tensors: _begin_device): the depth batch's chain queued, nothing waited
        for; collected by localize_batch_end().  The pixel buffers are kept alive until then."""
        a = self._depth_batch_args(captures, workspaces, kw)
        fn = self.lib.agh_localize_depth_batch_begin_device if a["on_device"] else self.lib.agh_localize_depth_batch_begin
        self._check(fn(self._h, a["recs"], a["n_images"], a["lps"], C.c_int32(a["Ck"])))
        self._batch_pending = a

    def localize_batch(self, captures, sizes_left, workspaces, samples=None, n_samples=0, sample_seeds=None,
                       classify: bool = True, min_inliers: int = 3, min_length: float = 0.005, filters_boundaries=0,
                       cell_size: float = 0.003, dense=False, caps=None):
        """agh_localize_batch: the chain of localize() over a batch of captures in one call with one synchronisation.
        `captures`: a list of (N_k, >= 3) float32 arrays, or of torch CUDA tensors (agh_localize_batch_device, read in place
        with their row stride).  Per capture: sizes_left, workspaces, samples (None, or a list of arrays / None per capture),
        n_samples (an int for all, or a list), sample_seeds, dense (a bool for all, or a list).  caps: (handle_cap, idx_cap,
        hands_cap) of the output buffers (default: large enough).  Returns a list of the dicts localize() returns, one per
        capture; after an AghError, self.last_batch_counts holds the per-capture counts the library reported."""
        a = self._batch_args(captures, sizes_left, workspaces, samples, n_samples, sample_seeds, classify, min_inliers,
                             min_length, filters_boundaries, cell_size, dense)
        fn = self.lib.agh_localize_batch_device if a["on_device"] else self.lib.agh_localize_batch
        return self._batch_collect(a, caps, lambda *out: fn(self._h, a["ptrs"], a["strides"], a["ns"], a["lps"],
                                                            C.c_int32(a["Ck"]), *out))

    def _batch_args(self, captures, sizes_left, workspaces, samples, n_samples, sample_seeds, classify, min_inliers, min_length,
                    filters_boundaries, cell_size, dense, Ck=None):
        """The C arrays of a batch call: pointers, strides, counts and agh_localize_params records, and what keeps them alive.
        (Ck: the number of captures of a depth batch, which has no point arrays.)"""
        Ck = len(captures) if Ck is None else Ck
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * Ck
        sizes_left, dense_l, seeds = per(sizes_left), per(dense), per(1 if sample_seeds is None else sample_seeds)
        samples_l = per(samples) if isinstance(samples, (list, tuple)) else [samples] * Ck
        ns_l = per(n_samples)
        ws_a = np.asarray(workspaces, np.float64)
        ws_l = list(ws_a) if ws_a.ndim == 2 else [ws_a] * Ck
        on_device = len(captures) > 0 and hasattr(captures[0], "is_cuda") and captures[0].is_cuda
        keep, ptrs, strides, ns = self._capture_arrays(captures, on_device)
        lps = (AghLocalizeParams * max(Ck, 1))()
        S_list, sample_arrays = [], []
        for k in range(Ck):
            lp = lps[k]
            lp.size_left, lp.dense, lp.classify = int(sizes_left[k]), 1 if dense_l[k] else 0, 1 if classify else 0
            ws = np.ascontiguousarray(ws_l[k], np.float64)
            assert ws.size == 6
            for q in range(6):
                lp.workspace[q] = float(ws[q])
            lp.cell_size = cell_size
            if samples_l[k] is not None:
                s = np.ascontiguousarray(samples_l[k], np.int32)
                sample_arrays.append(s)
                lp.sample_idx = s.ctypes.data_as(C.POINTER(C.c_int32))
                S = s.shape[0]
            else:
                lp.sample_idx = None
                S = int(ns_l[k])
            S_list.append(S)
            lp.n_samples, lp.sample_seed, lp.min_inliers, lp.min_length = S, int(seeds[k]), min_inliers, min_length
            lp.filters_boundaries = int(filters_boundaries)
        return {"Ck": Ck, "on_device": on_device, "keep": keep, "sample_arrays": sample_arrays, "ptrs": ptrs, "strides": strides,
                "ns": ns, "lps": lps, "S_list": S_list}

    @staticmethod
    def _capture_arrays(captures, on_device):
        Ck = len(captures)
        keep, ptrs, strides, ns = [], (C.c_void_p * max(Ck, 1))(), (C.c_int64 * max(Ck, 1))(), (C.c_int64 * max(Ck, 1))()
        for k, xyz in enumerate(captures):
            if on_device:
                assert xyz.is_cuda and xyz.dim() == 2 and xyz.shape[1] >= 3 and xyz.stride(1) == 1
                ptrs[k], ns[k], strides[k] = xyz.data_ptr(), int(xyz.shape[0]), int(xyz.stride(0)) * 4
            else:
                xyz = np.ascontiguousarray(xyz, np.float32)
                assert xyz.ndim == 2 and xyz.shape[1] >= 3
                ptrs[k], ns[k], strides[k] = xyz.ctypes.data, xyz.shape[0], xyz.shape[1] * 4
            keep.append(xyz)
        return keep, ptrs, strides, ns

    def _batch_collect(self, a, caps, call):
        """Output buffers for the batch `a`, the collecting call, and its results as a list of dicts."""
        Ck, S_list = a["Ck"], a["S_list"]
        hcap = max(sum(min(8 * S, 8192) for S in S_list), 1)
        hc, ic, kc = caps if caps is not None else (hcap, hcap, hcap)
        handles, idx, hands = np.zeros(max(hc, 1), HANDLE_DTYPE), np.zeros(max(ic, 1), np.int32), np.zeros(max(kc, 1), HYP_DTYPE)
        sout = np.zeros(max(sum(S_list), 1), np.int32)
        res = (AghLocalizeBatchResult * max(Ck, 1))()
        rc = call(handles.ctypes.data_as(C.c_void_p), C.c_int64(hc), _p(idx, C.c_int32), C.c_int64(ic),
                  hands.ctypes.data_as(C.c_void_p), C.c_int64(kc), _p(sout, C.c_int32), res)
        self.last_batch_counts = [
            {"n_voxels": r.r.n_voxels, "n_hypotheses": r.r.n_hypotheses, "n_hands": r.r.n_hands, "n_handles": r.r.n_handles,
             "n_inlier_idx": r.r.n_inlier_idx, "first_handle": r.first_handle, "first_inlier_idx": r.first_inlier_idx,
             "first_hand": r.first_hand, "first_sample": r.first_sample} for r in res[:Ck]]
        self._check(rc)
        out = []
        for k in range(Ck):
            r = res[k]
            h0, i0, k0, s0 = r.first_handle, r.first_inlier_idx, r.first_hand, r.first_sample
            out.append({"handles": handles[h0:h0 + r.r.n_handles].copy(), "inlier_idx": idx[i0:i0 + r.r.n_inlier_idx].copy(),
                        "hands": hands[k0:k0 + r.r.n_hands].copy(), "samples": sout[s0:s0 + S_list[k]].copy(),
                        "n_voxels": int(r.r.n_voxels), "n_hypotheses": int(r.r.n_hypotheses)})
        self.n = sum(int(r.r.n_voxels) for r in res[:Ck])
        self.last_samples = sum(S_list)
        self.last_n = sum(int(r.r.n_hypotheses) for r in res[:Ck])
        return out

    def localize_batch_begin(self, captures, sizes_left, workspaces, samples=None, n_samples=0, sample_seeds=None,
                             classify: bool = True, min_inliers: int = 3, min_length: float = 0.005, filters_boundaries=0,
                             cell_size: float = 0.003, dense=False):
        """agh_localize_batch_begin (torch CUDA tensors: _begin_device): the batch's chain queued, nothing waited for; arguments
        as for localize_batch.  The captures are kept alive until localize_batch_end; the argument arrays the library copies
        (self._batch_pending: ptrs, strides, ns, lps, sample_arrays) are kept too, although it no longer needs them."""
        a = self._batch_args(captures, sizes_left, workspaces, samples, n_samples, sample_seeds, classify, min_inliers,
                             min_length, filters_boundaries, cell_size, dense)
        fn = self.lib.agh_localize_batch_begin_device if a["on_device"] else self.lib.agh_localize_batch_begin
        self._check(fn(self._h, a["ptrs"], a["strides"], a["ns"], a["lps"], C.c_int32(a["Ck"])))
        self._batch_pending = a

    @staticmethod
    def _batch_mask_pointers(a, masks):
        """The masks array of a masked points batch: one uint8 per raw point per capture (torch CUDA tensors, 1-D with unit
        stride, for device captures).  `masks` None passes NULL and a None entry a NULL mask, for the library to refuse."""
        if masks is None:
            return None, []
        Ck = a["Ck"]
        assert len(masks) == Ck
        ptrs, keep = (C.c_void_p * max(Ck, 1))(), []
        for k, m in enumerate(masks):
            n_pts = int(a["ns"][k])
            if m is None:
                ptrs[k] = None
            elif a["on_device"]:
                assert m.is_cuda and m.dim() == 1 and m.element_size() == 1 and m.shape[0] == n_pts
                assert n_pts <= 1 or m.stride(0) == 1
                ptrs[k] = m.data_ptr()
            else:
                m = np.ascontiguousarray(m).view(np.uint8) if np.asarray(m).dtype == np.bool_ else np.ascontiguousarray(m, np.uint8)
                assert m.shape == (n_pts,)
                ptrs[k] = m.ctypes.data
            keep.append(m)
        return ptrs, keep

    def _batch_masked_args(self, captures, sizes_left, workspaces, masks, kw):
        a = self._batch_args(captures, sizes_left, workspaces, kw.pop("samples", None), kw.pop("n_samples", 0),
                             kw.pop("sample_seeds", None), kw.pop("classify", True), kw.pop("min_inliers", 3),
                             kw.pop("min_length", 0.005), kw.pop("filters_boundaries", 0), kw.pop("cell_size", 0.003),
                             kw.pop("dense", False))
        assert not kw, f"unknown arguments {sorted(kw)}"
        a["mptrs"], a["mkeep"] = self._batch_mask_pointers(a, masks)
        return a

    def localize_batch_masked(self, captures, sizes_left, workspaces, masks, caps=None, **kw):
        """agh_localize_batch_masked (torch CUDA tensors: agh_localize_batch_masked_device): localize_batch() with capture k's
        n_samples drawn among the voxels that hold a kept raw point with a non-zero byte in masks[k] (one uint8 per raw point).
        The other arguments (by keyword) as for localize_batch; `samples` goes through for the library to refuse.
        batch_mask_counts() then gives the eligible voxels per capture."""
        a = self._batch_masked_args(captures, sizes_left, workspaces, masks, kw)
        fn = self.lib.agh_localize_batch_masked_device if a["on_device"] else self.lib.agh_localize_batch_masked
        return self._batch_collect(a, caps, lambda *out: fn(self._h, a["ptrs"], a["strides"], a["ns"], a["mptrs"], a["lps"],
                                                            C.c_int32(a["Ck"]), *out))

    def localize_batch_masked_begin(self, captures, sizes_left, workspaces, masks, **kw):
        """agh_localize_batch_masked_begin (torch CUDA tensors: _begin_device): the masked batch's chain queued, nothing waited
        for; collected by localize_batch_end().  Captures and masks are kept alive until then."""
        a = self._batch_masked_args(captures, sizes_left, workspaces, masks, kw)
        fn = self.lib.agh_localize_batch_masked_begin_device if a["on_device"] else self.lib.agh_localize_batch_masked_begin
        self._check(fn(self._h, a["ptrs"], a["strides"], a["ns"], a["mptrs"], a["lps"], C.c_int32(a["Ck"])))
        self._batch_pending = a

    def _depth_batch_masked_args(self, captures, masks, workspaces, kw):
        a = self._depth_batch_args(captures, workspaces, kw)
        if masks is None:
            a["mrecs"], a["mkeep"] = None, []
        else:
            assert len(masks) == len(captures) and all(len(m) == len(images) for m, images in zip(masks, captures))
            a["mrecs"], a["mkeep"] = sample_mask_records([m for ms in masks for m in ms], a["on_device"])
        return a

    def localize_depth_batch_masked(self, captures, masks, workspaces, caps=None, **kw):
        """agh_localize_depth_batch_masked (torch CUDA tensors: agh_localize_depth_batch_masked_device): localize_depth_batch()
        with every capture's samples drawn under its own masks.  `masks`: per capture a list with one entry per image (see
        sample_mask_records: an (H, W) uint8 array, or None for no eligible pixel); None passes NULL."""
        a = self._depth_batch_masked_args(captures, masks, workspaces, kw)
        fn = self.lib.agh_localize_depth_batch_masked_device if a["on_device"] else self.lib.agh_localize_depth_batch_masked
        return self._batch_collect(a, caps, lambda *out: fn(self._h, a["recs"], a["mrecs"], a["n_images"], a["lps"],
                                                            C.c_int32(a["Ck"]), *out))

    def localize_depth_batch_masked_begin(self, captures, masks, workspaces, **kw):
        """agh_localize_depth_batch_masked_begin (torch CUDA tensors: _begin_device): the masked depth batch's chain queued;
        collected by localize_batch_end().  Pixel and mask buffers are kept alive until then."""
        a = self._depth_batch_masked_args(captures, masks, workspaces, kw)
        fn = self.lib.agh_localize_depth_batch_masked_begin_device if a["on_device"] else self.lib.agh_localize_depth_batch_masked_begin
        self._check(fn(self._h, a["recs"], a["mrecs"], a["n_images"], a["lps"], C.c_int32(a["Ck"])))
        self._batch_pending = a

    def batch_mask_counts(self, cap_captures: int = 64) -> np.ndarray:
        """agh_get_batch_mask_counts: the eligible voxels M_k of every capture of the last masked batch this context collected."""
        m = np.full(max(cap_captures, 1), -1, np.int64)  # (the call writes n_captures counts, none of them negative)
        self._check(self.lib.agh_get_batch_mask_counts(self._h, _p(m, C.c_int64), C.c_int32(cap_captures)))
        return m[m >= 0].copy()

    # ---- label images in the batch chains (include/agh.h, agh_localize_batch_labeled*) ----

    @staticmethod
    def _batch_label_lists(a, n_objects):
        """A labelled batch has a list per (capture, object): a["Ck"] and a["S_list"] become the lists' (what _batch_collect
        sizes the outputs and reads results[] with), a["groups"] the objects per capture.  n_objects the library will refuse
        (None, an entry outside 1..64, more than 64 lists) leave no list to collect."""
        Ck = a["Ck"]
        a["n_captures"] = Ck
        if n_objects is None:
            a["n_obj"], groups = None, None
        else:
            groups = [int(K) for K in n_objects]
            assert len(groups) == Ck
            a["n_obj"] = (C.c_int32 * max(Ck, 1))(*groups)
            if any(K < 1 or K > 64 for K in groups) or sum(groups) > 64:
                groups = None
        a["groups"] = groups if groups is not None else []
        a["S_list"] = [S for K, S in zip(a["groups"], a["S_list"]) for _ in range(K)]
        a["Ck"] = len(a["S_list"])
        return a

    def _batch_labeled_collect(self, a, caps, call):
        """_batch_collect over the lists, regrouped: a list per capture of a list per object of the usual dicts."""
        flat = self._batch_collect(a, caps, call)
        out, l = [], 0
        for K in a["groups"]:
            out.append(flat[l:l + K])
            l += K
        self.n = sum(objs[0]["n_voxels"] for objs in out)  # (every list reports its capture's voxel count)
        return out

    def _batch_labeled_args(self, captures, sizes_left, workspaces, labels, n_objects, kw):
        a = self._batch_masked_args(captures, sizes_left, workspaces, labels, kw)
        return self._batch_label_lists(a, n_objects)

    def localize_batch_labeled(self, captures, sizes_left, workspaces, labels, n_objects, caps=None, **kw):
        """agh_localize_batch_labeled (torch CUDA tensors: agh_localize_batch_labeled_device): localize_batch() with one sample
        list per object of every capture.  labels[k]: one uint8 per raw point of capture k (0: no object, j + 1: object j of
        that capture); n_objects[k]: its objects; n_samples is per OBJECT.  The other arguments (by keyword) as for
        localize_batch.  Returns a list per capture of a list per object of the dicts localize_batch returns; capture k's equal
        localize_labeled on that capture alone.  batch_label_counts() then gives the eligible voxels per list."""
        a = self._batch_labeled_args(captures, sizes_left, workspaces, labels, n_objects, kw)
        fn = self.lib.agh_localize_batch_labeled_device if a["on_device"] else self.lib.agh_localize_batch_labeled
        return self._batch_labeled_collect(a, caps, lambda *out: fn(self._h, a["ptrs"], a["strides"], a["ns"], a["mptrs"], a["n_obj"],
                                                                    a["lps"], C.c_int32(a["n_captures"]), *out))

    def localize_batch_labeled_begin(self, captures, sizes_left, workspaces, labels, n_objects, **kw):
        """agh_localize_batch_labeled_begin (torch CUDA tensors: _begin_device): the labelled batch's chain queued, nothing
        waited for; collected by localize_batch_end().  Captures and labels are kept alive until then."""
        a = self._batch_labeled_args(captures, sizes_left, workspaces, labels, n_objects, kw)
        fn = self.lib.agh_localize_batch_labeled_begin_device if a["on_device"] else self.lib.agh_localize_batch_labeled_begin
        self._check(fn(self._h, a["ptrs"], a["strides"], a["ns"], a["mptrs"], a["n_obj"], a["lps"], C.c_int32(a["n_captures"])))
        self._batch_pending = a

    def _depth_batch_labeled_args(self, captures, labels, workspaces, n_objects, kw):
        a = self._depth_batch_args(captures, workspaces, kw)
        if labels is None:
            a["mrecs"], a["mkeep"] = None, []
        else:
            assert len(labels) == len(captures) and all(len(m) == len(images) for m, images in zip(labels, captures))
            a["mrecs"], a["mkeep"] = label_image_records([m for ms in labels for m in ms], a["on_device"])
        return self._batch_label_lists(a, n_objects)

    def localize_depth_batch_labeled(self, captures, labels, workspaces, n_objects, caps=None, **kw):
        """agh_localize_depth_batch_labeled (torch CUDA tensors: agh_localize_depth_batch_labeled_device):
        localize_depth_batch() with one sample list per object of every capture.  `labels`: per capture a list with one entry
        per image (see label_image_records: an (H, W) uint8 array, or None for no object in that image); None passes NULL."""
        a = self._depth_batch_labeled_args(captures, labels, workspaces, n_objects, kw)
        fn = self.lib.agh_localize_depth_batch_labeled_device if a["on_device"] else self.lib.agh_localize_depth_batch_labeled
        return self._batch_labeled_collect(a, caps, lambda *out: fn(self._h, a["recs"], a["mrecs"], a["n_images"], a["n_obj"], a["lps"],
                                                                    C.c_int32(a["n_captures"]), *out))

    def localize_depth_batch_labeled_begin(self, captures, labels, workspaces, n_objects, **kw):
        """agh_localize_depth_batch_labeled_begin (torch CUDA tensors: _begin_device): the labelled depth batch's chain queued;
        collected by localize_batch_end().  Pixel and label buffers are kept alive until then."""
        a = self._depth_batch_labeled_args(captures, labels, workspaces, n_objects, kw)
        fn = self.lib.agh_localize_depth_batch_labeled_begin_device if a["on_device"] else self.lib.agh_localize_depth_batch_labeled_begin
        self._check(fn(self._h, a["recs"], a["mrecs"], a["n_images"], a["n_obj"], a["lps"], C.c_int32(a["n_captures"])))
        self._batch_pending = a

    def batch_label_counts(self, cap_lists: int = 64) -> np.ndarray:
        """agh_get_batch_label_counts: the eligible voxels M_{k,j} of every list of the last labelled batch this context
        collected, in list order (capture after capture, object after object)."""
        m = np.full(max(cap_lists, 1), -1, np.int64)  # (the call writes L counts, none of them negative)
        self._check(self.lib.agh_get_batch_label_counts(self._h, _p(m, C.c_int64), C.c_int32(cap_lists)))
        return m[m >= 0].copy()

    # ---- clusters in the batch chains (include/agh.h, agh_localize_batch_clustered*) ----

    def _batch_cluster_lists(self, a, cps):
        """A clustered batch has cps[k].max_objects lists for capture k.  `cps`: a list of cluster_params() records, one per
        capture, or one record for all captures; None passes NULL, for the library to refuse."""
        Ck = a["Ck"]
        if cps is None:
            a["cps"] = None
            return self._batch_label_lists(a, None)
        if isinstance(cps, AghClusterParams):
            cps = [cps] * Ck
        assert len(cps) == Ck
        recs = (AghClusterParams * max(Ck, 1))()
        for k, cp in enumerate(cps):
            C.memmove(C.byref(recs[k]), C.byref(cp), C.sizeof(AghClusterParams))
        a["cps"] = recs
        return self._batch_label_lists(a, [int(cp.max_objects) for cp in cps])

    def localize_batch_clustered(self, captures, sizes_left, workspaces, cps, caps=None, **kw):
        """agh_localize_batch_clustered (torch CUDA tensors: agh_localize_batch_clustered_device): localize_batch_labeled()
        whose objects are, per capture, the connected components of its own voxels above the support plane of cps[k]
        (cluster_params(); a single record serves every capture), found on the device inside the call; n_samples is per OBJECT.
        Returns a list per capture of cps[k].max_objects dicts; capture k's equal localize_clustered on that capture alone.
        batch_cluster_info() and batch_cluster_labels() then describe the objects."""
        a = self._batch_cluster_lists(self._batch_masked_args(captures, sizes_left, workspaces, None, kw), cps)
        fn = self.lib.agh_localize_batch_clustered_device if a["on_device"] else self.lib.agh_localize_batch_clustered
        return self._batch_labeled_collect(a, caps, lambda *out: fn(self._h, a["ptrs"], a["strides"], a["ns"], a["cps"], a["lps"],
                                                                    C.c_int32(a["n_captures"]), *out))

    def localize_batch_clustered_begin(self, captures, sizes_left, workspaces, cps, **kw):
        """agh_localize_batch_clustered_begin (torch CUDA tensors: _begin_device): the clustered batch's chain queued, nothing
        waited for; collected by localize_batch_end().  The captures are kept alive until then."""
        a = self._batch_cluster_lists(self._batch_masked_args(captures, sizes_left, workspaces, None, kw), cps)
        fn = self.lib.agh_localize_batch_clustered_begin_device if a["on_device"] else self.lib.agh_localize_batch_clustered_begin
        self._check(fn(self._h, a["ptrs"], a["strides"], a["ns"], a["cps"], a["lps"], C.c_int32(a["n_captures"])))
        self._batch_pending = a

    def localize_depth_batch_clustered(self, captures, workspaces, cps, caps=None, **kw):
        """agh_localize_depth_batch_clustered (torch CUDA tensors as `data`: agh_localize_depth_batch_clustered_device):
        localize_batch_clustered() straight from depth images (`captures` as for localize_depth_batch)."""
        a = self._batch_cluster_lists(self._depth_batch_args(captures, workspaces, kw), cps)
        fn = self.lib.agh_localize_depth_batch_clustered_device if a["on_device"] else self.lib.agh_localize_depth_batch_clustered
        return self._batch_labeled_collect(a, caps, lambda *out: fn(self._h, a["recs"], a["n_images"], a["cps"], a["lps"],
                                                                    C.c_int32(a["n_captures"]), *out))

    def localize_depth_batch_clustered_begin(self, captures, workspaces, cps, **kw):
        """agh_localize_depth_batch_clustered_begin (torch CUDA tensors: _begin_device): the clustered depth batch's chain
        queued; collected by localize_batch_end().  The pixel buffers are kept alive until then."""
        a = self._batch_cluster_lists(self._depth_batch_args(captures, workspaces, kw), cps)
        fn = (self.lib.agh_localize_depth_batch_clustered_begin_device if a["on_device"]
              else self.lib.agh_localize_depth_batch_clustered_begin)
        self._check(fn(self._h, a["recs"], a["n_images"], a["cps"], a["lps"], C.c_int32(a["n_captures"])))
        self._batch_pending = a

    def batch_cluster_info(self, cap_captures: int = 64, cap_lists: int = 64):
        """agh_get_batch_cluster_info of the last clustered batch this context collected: a dict with, per capture,
        n_foreground, n_components and n_objects (arrays), and per list of the call n_voxels (M_l) and ids (the object's
        smallest capture-local voxel index, -1: none), in list order."""
        info = (AghClusterInfo * max(cap_captures, 1))()
        for r in info:
            r.n_foreground = -2
        m = np.full(max(cap_lists, 1), -2, np.int64)
        ids = np.full(max(cap_lists, 1), -2, np.int32)
        self._check(self.lib.agh_get_batch_cluster_info(self._h, info, _p(m, C.c_int64), _p(ids, C.c_int32), C.c_int32(cap_captures),
                                                        C.c_int32(cap_lists)))
        rows = [r for r in info if r.n_foreground > -2]
        return {"n_foreground": np.array([r.n_foreground for r in rows], np.int64),
                "n_components": np.array([r.n_components for r in rows], np.int64),
                "n_objects": np.array([r.n_objects for r in rows], np.int64),
                "n_voxels": m[m > -2].copy(), "ids": ids[ids > -2].copy()}

    def batch_cluster_labels(self, cap: int | None = None) -> np.ndarray:
        """agh_get_batch_cluster_labels: per voxel of the bound batch, in cloud()'s order, 0 or object + 1 (the object being
        capture-local), of the last clustered batch collected."""
        cap = int(self.n) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), np.uint8)
        nv = self._check(self.lib.agh_get_batch_cluster_labels(self._h, C.c_void_p(out.ctypes.data), C.c_int64(cap)))
        return out[:nv].copy()

    # ---- a fitted plane in the batch chains (include/agh.h, agh_localize_batch_clustered_fit*) ----

    @staticmethod
    def _batch_fit_records(a, fps):
        """`fps`: a list of plane_fit_params() records, one per capture, or one record for all captures; None passes NULL, for
        the library to refuse.  (Behind _batch_cluster_lists: a["Ck"] counts the lists by then.)"""
        Ck = a["n_captures"]
        if fps is None:
            a["fps"] = None
            return a
        if isinstance(fps, AghPlaneFitParams):
            fps = [fps] * Ck
        assert len(fps) == Ck
        recs = (AghPlaneFitParams * max(Ck, 1))()
        for k, fp in enumerate(fps):
            C.memmove(C.byref(recs[k]), C.byref(fp), C.sizeof(AghPlaneFitParams))
        a["fps"] = recs
        return a

    def localize_batch_clustered_fit(self, captures, sizes_left, workspaces, fps, cps, caps=None, **kw):
        """agh_localize_batch_clustered_fit (torch CUDA tensors: agh_localize_batch_clustered_fit_device):
        localize_batch_clustered() with every capture's support plane found on the device inside the call, on its own voxels
        with fps[k] (plane_fit_params(); a single record serves every capture); cps[k].plane is not read.  batch_plane_fit()
        and batch_plane_fit_candidates(k) then describe the fits, batch_cluster_info() and batch_cluster_labels() the objects."""
        a = self._batch_cluster_lists(self._batch_masked_args(captures, sizes_left, workspaces, None, kw), cps)
        self._batch_fit_records(a, fps)
        fn = self.lib.agh_localize_batch_clustered_fit_device if a["on_device"] else self.lib.agh_localize_batch_clustered_fit
        return self._batch_labeled_collect(a, caps, lambda *out: fn(self._h, a["ptrs"], a["strides"], a["ns"], a["fps"], a["cps"],
                                                                    a["lps"], C.c_int32(a["n_captures"]), *out))

    def localize_batch_clustered_fit_begin(self, captures, sizes_left, workspaces, fps, cps, **kw):
        """agh_localize_batch_clustered_fit_begin (torch CUDA tensors: _begin_device): the fitted batch's chain queued, nothing
        waited for; collected by localize_batch_end().  The captures are kept alive until then."""
        a = self._batch_cluster_lists(self._batch_masked_args(captures, sizes_left, workspaces, None, kw), cps)
        self._batch_fit_records(a, fps)
        fn = (self.lib.agh_localize_batch_clustered_fit_begin_device if a["on_device"]
              else self.lib.agh_localize_batch_clustered_fit_begin)
        self._check(fn(self._h, a["ptrs"], a["strides"], a["ns"], a["fps"], a["cps"], a["lps"], C.c_int32(a["n_captures"])))
        self._batch_pending = a

    def localize_depth_batch_clustered_fit(self, captures, workspaces, fps, cps, caps=None, **kw):
        """agh_localize_depth_batch_clustered_fit (torch CUDA tensors as `data`: agh_localize_depth_batch_clustered_fit_device):
        localize_batch_clustered_fit() straight from depth images (`captures` as for localize_depth_batch)."""
        a = self._batch_cluster_lists(self._depth_batch_args(captures, workspaces, kw), cps)
        self._batch_fit_records(a, fps)
        fn = (self.lib.agh_localize_depth_batch_clustered_fit_device if a["on_device"]
              else self.lib.agh_localize_depth_batch_clustered_fit)
        return self._batch_labeled_collect(a, caps, lambda *out: fn(self._h, a["recs"], a["n_images"], a["fps"], a["cps"], a["lps"],
                                                                    C.c_int32(a["n_captures"]), *out))

    def localize_depth_batch_clustered_fit_begin(self, captures, workspaces, fps, cps, **kw):
        """agh_localize_depth_batch_clustered_fit_begin (torch CUDA tensors: _begin_device): the fitted depth batch's chain
        queued; collected by localize_batch_end().  The pixel buffers are kept alive until then."""
        a = self._batch_cluster_lists(self._depth_batch_args(captures, workspaces, kw), cps)
        self._batch_fit_records(a, fps)
        fn = (self.lib.agh_localize_depth_batch_clustered_fit_begin_device if a["on_device"]
              else self.lib.agh_localize_depth_batch_clustered_fit_begin)
        self._check(fn(self._h, a["recs"], a["n_images"], a["fps"], a["cps"], a["lps"], C.c_int32(a["n_captures"])))
        self._batch_pending = a

    def batch_plane_fit(self, cap_captures: int = 64) -> list:
        """agh_get_batch_plane_fit of the last fitted batch this context collected: a list, in capture order, of the dicts
        plane_fit() returns."""
        recs = (AghPlaneFitResult * max(cap_captures, 1))()
        n = self._check(self.lib.agh_get_batch_plane_fit(self._h, recs, C.c_int32(cap_captures)))
        return [{"plane": np.array(list(r.plane), np.float64), "n_voxels": r.n_voxels, "n_inliers": r.n_inliers,
                 "n_refit": r.n_refit, "best_candidate": r.best_candidate, "found": r.found, "refined": r.refined}
                for r in recs[:n]]

    def batch_plane_fit_candidates(self, capture: int, cap: int = 256) -> dict:
        """agh_get_batch_plane_fit_candidates: plane_fit_candidates() for one capture of the last fitted batch (the voxel indices
        are capture-local)."""
        idx = np.zeros((max(cap, 1), 3), np.int32)
        planes = np.zeros((max(cap, 1), 4), np.float64)
        counts = np.zeros(max(cap, 1), np.int64)
        n = self._check(self.lib.agh_get_batch_plane_fit_candidates(self._h, C.c_int32(capture), _p(idx, C.c_int32),
                                                                    _p(planes, C.c_double), _p(counts, C.c_int64), C.c_int32(cap)))
        return {"idx": idx[:n].copy(), "planes": planes[:n].copy(), "counts": counts[:n].copy()}

    def localize_batch_stage(self, captures):
        """agh_localize_batch_stage: the NEXT batch's host captures up on a second stream, beside the chain in flight.  Returns
        the list of arrays to hand to the next localize_batch_begin (the library recognises the set by pointers, strides and
        counts); they are kept alive until a later stage call replaces them."""
        keep, ptrs, strides, ns = self._capture_arrays(captures, False)
        self._batch_stage_keep = (keep, ptrs, strides, ns)
        self._check(self.lib.agh_localize_batch_stage(self._h, ptrs, strides, ns, C.c_int32(len(keep))))
        return keep

    def localize_batch_end(self, caps=None):
        """agh_localize_batch_end: the one synchronisation and the results of the batch localize_batch_begin queued, as
        localize_batch returns them (caps and last_batch_counts likewise)."""
        a = getattr(self, "_batch_pending", None)
        self._batch_pending = None
        if a is None:
            # No localize_batch_begin of this object is pending: the library says so (AGH_ERR_STATE).  Should a chain be in flight
            # all the same (begun through the raw library), it is ended with room for the records of any batch and for no
            # output -- the library writes results[k] for up to 64 captures and skips a NULL samples_out.
            res = (AghLocalizeBatchResult * 64)()
            self._check(self.lib.agh_localize_batch_end(self._h, None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(0),
                                                        None, res))
            return []
        collect = self._batch_labeled_collect if "groups" in a else self._batch_collect  # (a labelled batch: a list per capture)
        return collect(a, caps, lambda *out: self.lib.agh_localize_batch_end(self._h, *out))

    def localize_begin(self, xyz, size_left: int, workspace, **kw):
        """agh_localize_begin: the chain of this capture queued, nothing waited for (see include/agh.h)."""
        return self.localize(xyz, size_left, workspace, phase="begin", **kw)

    def localize_stage(self, xyz):
        """agh_localize_stage: the NEXT capture up on a second stream, beside the chain in flight.  Pass the same array object to
        the next localize_begin (the library recognises the capture by pointer, stride and count)."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        self._stage_keep = xyz
        self._check(self.lib.agh_localize_stage(self._h, _p(xyz, C.c_float), C.c_int64(xyz.shape[1] * 4), C.c_int64(xyz.shape[0])))
        return xyz

    def localize_end(self):
        """agh_localize_end: the one synchronisation and the results of the chain localize_begin queued."""
        if getattr(self, "_loc_bufs", None) is None:  # (no begin before: the library says so)
            self._loc_bufs = (np.zeros(1, HANDLE_DTYPE), np.zeros(1, np.int32), np.zeros(1, HYP_DTYPE), np.zeros(1, np.int32))
            self._loc_S = 0
        handles, idx, hands, sout = self._loc_bufs
        hcap = handles.shape[0]
        res = AghLocalizeResult()
        self._check(self.lib.agh_localize_end(self._h, handles.ctypes.data_as(C.c_void_p), C.c_int64(hcap), _p(idx, C.c_int32),
                                              C.c_int64(hcap), hands.ctypes.data_as(C.c_void_p), C.c_int64(hcap),
                                              _p(sout, C.c_int32), C.byref(res)))
        self._loc_keep = None
        return self._localize_result(res, self._loc_S)

    def _localize_result(self, res, S):
        handles, idx, hands, sout = self._loc_bufs
        self.n = res.n_voxels
        self.last_samples = S
        self.last_n = res.n_hypotheses
        return {"handles": handles[:res.n_handles].copy(), "inlier_idx": idx[:res.n_inlier_idx].copy(),
                "hands": hands[:res.n_hands].copy(), "samples": sout[:S].copy(), "n_voxels": int(res.n_voxels),
                "n_hypotheses": int(res.n_hypotheses)}

    def remove_plane(self, max_iterations: int = 100, distance_threshold: float = 0.01, probability: float = 0.99,
                     seed: int = 12345, optimize: bool = True, cam_ids_by_position: bool = True) -> dict:
        """localizeHands' table-plane removal (agh_remove_plane): RANSAC plane on the current cloud, whose non-inliers
        then become the context's cloud.  Returns the agh_plane_result fields as a dict."""
        pp = AghPlaneParams(max_iterations, int(optimize), distance_threshold, probability, seed, int(cam_ids_by_position))
        res = AghPlaneResult()
        self._check(self.lib.agh_remove_plane(self._h, C.byref(pp), C.byref(res)))
        self.n = res.n_remaining
        return {"coefficients": np.array(res.coefficients[:], np.float32), "n_inliers": int(res.n_inliers),
                "n_remaining": int(res.n_remaining), "iterations": int(res.iterations), "found": bool(res.found)}

    def plane_inliers(self) -> np.ndarray:
        """PCL's inliers->indices of the last remove_plane."""
        k = self._check(self.lib.agh_get_plane_inliers(self._h, None, C.c_int64(0)))
        idx = np.zeros(max(k, 1), np.int32)
        k = self._check(self.lib.agh_get_plane_inliers(self._h, _p(idx, C.c_int32), C.c_int64(idx.size)))
        return idx[:k]

    def plane_candidates(self) -> dict:
        """The candidate planes the last remove_plane drew, their samples and inlier counts (drawing order)."""
        k = self._check(self.lib.agh_get_plane_candidates(self._h, None, None, None, C.c_int64(0)))
        planes = np.zeros((max(k, 1), 4), np.float32)
        samples = np.zeros((max(k, 1), 3), np.int32)
        counts = np.zeros(max(k, 1), np.int64)
        self._check(self.lib.agh_get_plane_candidates(self._h, _p(planes, C.c_float), _p(samples, C.c_int32),
                                                      _p(counts, C.c_int64), C.c_int64(k)))
        return {"planes": planes[:k], "samples": samples[:k], "counts": counts[:k]}

    def cloud(self):
        xyz = np.zeros((max(self.n, 1), 3), np.float32)
        cam = np.zeros(max(self.n, 1), np.int32)
        k = self._check(self.lib.agh_get_cloud(self._h, _p(xyz, C.c_float), _p(cam, C.c_int32), C.c_int64(self.n)))
        return xyz[:k], cam[:k]

    def find_hands(self, samples: np.ndarray, calculates_antipodal: bool = False) -> np.ndarray:
        samples = np.ascontiguousarray(samples, np.int32)
        cap = max(8 * samples.shape[0], 1)
        out = getattr(self, "_out_buf", None)  # (a fresh 2.5 MB numpy array per call is an mmap / munmap pair and page faults)
        if out is None or out.shape[0] < cap:
            out = self._out_buf = np.zeros(cap, HYP_DTYPE)
        n = C.c_int64(0)
        self._check(self.lib.agh_find_hands(self._h, _p(samples, C.c_int32), C.c_int64(samples.shape[0]),
                                            C.c_int(1 if calculates_antipodal else 0), out.ctypes.data_as(C.c_void_p),
                                            C.c_int64(cap), C.byref(n)))
        self.last_samples = samples.shape[0]
        self.last_n = n.value
        return out[:n.value].copy()

    def frames(self) -> np.ndarray:
        fr = np.zeros(self.last_samples, FRAME_DTYPE)
        n = self._check(self.lib.agh_get_frames(self._h, fr.ctypes.data_as(C.c_void_p), C.c_int64(fr.shape[0])))
        return fr[:n]

    def neighbor_counts(self):
        nt = np.zeros(self.last_samples, np.int32)
        nh = np.zeros(self.last_samples, np.int32)
        self._check(self.lib.agh_get_neighbor_counts(self._h, _p(nt, C.c_int32), _p(nh, C.c_int32),
                                                     C.c_int64(nt.shape[0])))
        return nt, nh

    def images(self) -> np.ndarray:
        im = np.zeros((max(self.last_n, 1), 8000), np.uint8)
        n = self._check(self.lib.agh_get_images(self._h, _p(im, C.c_uint8), C.c_int64(self.last_n)))
        return im[:n]

    def normals(self) -> np.ndarray:
        nr = np.zeros((self.n, 3), np.float64)
        self._check(self.lib.agh_get_normals(self._h, _p(nr, C.c_double), C.c_int64(self.n)))
        return nr

    # ---- training side (learning.cpp:3-163, 249-318) ----
    def set_training_images(self, on: bool = True):
        self._check(self.lib.agh_set_training_images(self._h, C.c_int(1 if on else 0)))

    def training_images(self) -> np.ndarray:
        """(H, 3, 250) packed images of the last find_hands(calculates_antipodal=True): cam = -1, 0, 1."""
        last_n = getattr(self, "last_n", 0)
        im = np.zeros((max(last_n, 1), 3, 250), "<u4")
        n = self._check(self.lib.agh_get_training_images(self._h, _p(im, C.c_uint32), C.c_int64(last_n)))
        return im[:n]

    def hog_images(self, packed: np.ndarray) -> np.ndarray:
        packed = np.ascontiguousarray(packed, "<u4").reshape(-1, 250)
        desc = np.zeros((packed.shape[0], 3528), np.float32)
        self._check(self.lib.agh_hog_images(self._h, _p(packed, C.c_uint32), C.c_int64(packed.shape[0]), _p(desc, C.c_float)))
        return desc

    def train_svm(self, packed: np.ndarray, labels: np.ndarray, C_: float = 1.0, max_iter: int = 1000,
                  eps: float = 1.1920928955078125e-07, kernel: int = SVM_LINEAR) -> dict:
        """convertData's CvSVM::train.  LINEAR: 'w' is the compacted vector; POLY2: 'sv' (n_sv x 3528) and 'alpha'."""
        packed = np.ascontiguousarray(packed, "<u4").reshape(-1, 250)
        lab = np.ascontiguousarray(np.where(np.asarray(labels) > 0, 1, -1), np.int8)
        n = packed.shape[0]
        assert lab.shape[0] == n
        cap = 1 if kernel == SVM_LINEAR else n
        sv = np.zeros((cap, 3528), np.float32)
        alpha = np.zeros(cap, np.float64)
        n_sv = C.c_int32(0)
        rho = C.c_double(0)
        info = np.zeros(6, np.int32)
        self._check(self.lib.agh_train_svm(self._h, _p(packed, C.c_uint32), _p(lab, C.c_int8), C.c_int64(n), C.c_int32(kernel),
                                           C.c_double(C_), C.c_int32(max_iter), C.c_double(eps), _p(sv, C.c_float),
                                           C.c_int64(cap), _p(alpha, C.c_double), C.byref(n_sv), C.byref(rho),
                                           _p(info, C.c_int32)))
        return {"w": sv[0].copy(), "sv": sv[: n_sv.value].copy(), "alpha": alpha[: n_sv.value].copy(), "rho": rho.value,
                "kernel": kernel, "iterations": int(info[0]), "n_sv": int(info[1]), "n_neg": int(info[2]),
                "n_pos": int(info[3]), "rows_computed": int(info[4]), "rows_reused": int(info[5])}

    def load_svm_model(self, kernel: int, sv: np.ndarray, alpha: np.ndarray, rho: float):
        sv = np.ascontiguousarray(sv, np.float32).reshape(-1, 3528)
        alpha = np.ascontiguousarray(alpha, np.float64)
        self._check(self.lib.agh_load_svm_model(self._h, C.c_int32(kernel), _p(sv, C.c_float), C.c_int32(sv.shape[0]),
                                                C.c_int32(3528), _p(alpha, C.c_double), C.c_double(rho)))

    def learning_points(self, hyp: int):
        """(3, n_b) points_for_learning of hypothesis `hyp` and the camera id of each column."""
        n = C.c_int64(0)
        rc = self.lib.agh_get_learning_points(self._h, C.c_int64(hyp), None, None, C.c_int64(0), C.byref(n))
        if rc not in (0, -4):  # AGH_ERR_CAPACITY reports the size
            self._check(rc)
        pts = np.zeros((max(n.value, 1), 3), np.float64)
        cam = np.zeros(max(n.value, 1), np.int32)
        self._check(self.lib.agh_get_learning_points(self._h, C.c_int64(hyp), _p(pts, C.c_double), _p(cam, C.c_int32),
                                                     C.c_int64(n.value), C.byref(n)))
        return pts[: n.value].T.copy(), cam[: n.value].copy()

    def load_svm(self, w: np.ndarray, rho: float):
        w = np.ascontiguousarray(w, np.float32)
        self._check(self.lib.agh_load_svm(self._h, _p(w, C.c_float), C.c_int32(w.size), C.c_double(rho)))

    def load_svm_file(self, path: str):
        self._check(self.lib.agh_load_svm_file(self._h, path.encode()))

    def classify(self) -> np.ndarray:
        keep = np.zeros(max(self.last_n, 1), np.uint8)
        nk = C.c_int64(0)
        self._check(self.lib.agh_classify(self._h, _p(keep, C.c_uint8), C.c_int64(self.last_n), C.byref(nk)))
        return keep[:self.last_n]

    def epoch(self):
        """(stamp, hypothesis count) of the last find_hands call."""
        e, n = C.c_int32(0), C.c_int64(0)
        self._check(self.lib.agh_get_epoch(self._h, C.byref(e), C.byref(n)))
        return e.value, n.value

    def packed_images(self) -> np.ndarray:
        """(H, 250) packed occupancy images of the last find_hands call."""
        im = np.zeros((max(self.last_n, 1), 250), "<u4")
        n = self._check(self.lib.agh_get_packed_images(self._h, _p(im, C.c_uint32), C.c_int64(self.last_n)))
        return im[:n]

    def classify_images(self, packed: np.ndarray):
        """Learning::classify on packed images that belong to no search: (keep, decision values)."""
        packed = np.ascontiguousarray(packed, "<u4").reshape(-1, 250)
        n = packed.shape[0]
        keep = np.zeros(max(n, 1), np.uint8)
        sums = np.zeros(max(n, 1), np.float64)
        self._check(self.lib.agh_classify_images(self._h, _p(packed, C.c_uint32), C.c_int64(n), _p(keep, C.c_uint8),
                                                 _p(sums, C.c_double)))
        return keep[:n], sums[:n]

    # ---- multi-GPU: samples of one cloud sharded over the ranks of a communicator ----
    def comm_init(self, rank: int, n_ranks: int, unique_id: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self.lib.agh_comm_init(self._h, C.c_int32(rank), C.c_int32(n_ranks), buf))

    def comm_destroy(self):
        self._check(self.lib.agh_comm_destroy(self._h))

    def comm_set_segment_records(self, records: int):
        self._check(self.lib.agh_comm_set_segment_records(self._h, C.c_int64(records)))

    def comm_inject_fault(self, sites: int):
        """agh_comm_inject_fault (testing aid): this rank fails on its own at the named sites of its next sharded call."""
        self._check(self.lib.agh_comm_inject_fault(self._h, C.c_int32(sites)))

    def comm_rank(self):
        r, n = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.agh_comm_rank(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def comm_last_exchange(self):
        """(bytes one rank contributed, ranks, True if RCCL moved them) of the last sharded search's hypothesis all-gather."""
        b, n, v = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        self._check(self.lib.agh_comm_last_exchange(self._h, C.byref(b), C.byref(n), C.byref(v)))
        return b.value, n.value, bool(v.value)

    def find_hands_sharded(self, samples: np.ndarray, calculates_antipodal: bool = False, cap: int | None = None) -> np.ndarray:
        samples = np.ascontiguousarray(samples, np.int32)
        cap = max(8 * samples.shape[0], 1) if cap is None else cap
        out = np.zeros(cap, HYP_DTYPE)
        n = C.c_int64(0)
        self._check(self.lib.agh_find_hands_sharded(self._h, _p(samples, C.c_int32), C.c_int64(samples.shape[0]),
                                                    C.c_int(1 if calculates_antipodal else 0),
                                                    out.ctypes.data_as(C.c_void_p), C.c_int64(cap), C.byref(n)))
        r, g = self.comm_rank()
        lo, hi = shard_slice(samples.shape[0], r, g)
        self.last_samples = hi - lo
        self.shard_n = n.value
        e, mine = self.epoch()
        self.last_n = max(mine, 0)
        return out[:n.value].copy()

    def classify_sharded(self):
        """(records with svm_keep set, keep flags) of the last find_hands_sharded."""
        n = self.shard_n
        out = np.zeros(max(n, 1), HYP_DTYPE)
        keep = np.zeros(max(n, 1), np.uint8)
        nk = C.c_int64(0)
        self._check(self.lib.agh_classify_sharded(self._h, out.ctypes.data_as(C.c_void_p), _p(keep, C.c_uint8), C.c_int64(n),
                                                  C.byref(nk)))
        return out[:n].copy(), keep[:n].copy()

    def find_hands_sharded_torch(self, samples_t, out_t, nout_t, calculates_antipodal: bool = False, stream=None):
        S = samples_t.shape[0]
        cap = out_t.numel() // 160
        r, g = self.comm_rank()
        lo, hi = shard_slice(S, r, g)
        self.last_samples = hi - lo
        self._check(self.lib.agh_find_hands_sharded_device(
            self._h, C.c_void_p(samples_t.data_ptr()), C.c_int64(S), C.c_int(1 if calculates_antipodal else 0),
            C.c_void_p(out_t.data_ptr()), C.c_int64(cap), C.c_void_p(nout_t.data_ptr()),
            C.c_void_p(stream) if stream else None))

    def classify_sharded_torch(self, keep_t=None, stream=None):
        self._check(self.lib.agh_classify_sharded_device(
            self._h, C.c_void_p(keep_t.data_ptr()) if keep_t is not None else None, C.c_void_p(stream) if stream else None))

    def hog(self):
        desc = np.zeros((max(self.last_n, 1), 3528), np.float32)
        sums = np.zeros(max(self.last_n, 1), np.float64)
        n = self._check(self.lib.agh_get_hog(self._h, _p(desc, C.c_float), _p(sums, C.c_double), C.c_int64(self.last_n)))
        return desc[:n], sums[:n]

    def timing(self, counts: bool = False):
        """Summed kernel times [ms] per phase since the previous call; with counts=True also the number of timed launches behind
        each sum (profile level 3 times every fourth call only)."""
        t = AghTiming()
        self._check(self.lib.agh_get_timing(self._h, C.byref(t)))
        ms = {t.name[i].decode(): float(t.ms[i]) for i in range(t.n)}
        if counts:
            cnt = (C.c_int32 * 16)()
            self._check(self.lib.agh_get_timing_counts(self._h, cnt, C.c_int32(16)))
            return ms, {t.name[i].decode(): int(cnt[i]) for i in range(t.n)}
        return ms

    def grid_stats(self) -> dict:
        """Grid builds of this context: all of them, the cold ones (bounding box first) and the misses (a cloud outside the
        descriptor kept from the previous build)."""
        v = (C.c_int64 * 3)()
        self._check(self.lib.agh_get_grid_stats(self._h, v, C.c_int32(3)))
        return {"builds": int(v[0]), "cold": int(v[1]), "misses": int(v[2])}

    def grid_desc(self, cloud: int = 0) -> dict:
        """The grid descriptor the last build used for cloud `cloud` of the batch: origin, cell size, cells per axis, open faces."""
        mn, dim = (C.c_double * 3)(), (C.c_int32 * 3)()
        cell, opn = C.c_double(0.0), C.c_uint32(0)
        self._check(self.lib.agh_get_grid_desc(self._h, C.c_int32(cloud), mn, C.byref(cell), dim, C.byref(opn)))
        return {"mn": tuple(float(v) for v in mn), "cell": float(cell.value), "dim": tuple(int(v) for v in dim),
                "open": int(opn.value)}

    def set_profile(self, level: int):
        self._check(self.lib.agh_set_profile(self._h, C.c_int32(level)))

    def synchronize(self):
        self._check(self.lib.agh_synchronize(self._h))

    def selftest_math(self, n: int = 1 << 20, seed: int = 1) -> int:
        return int(self.lib.agh_selftest_math(self._h, C.c_int64(n), C.c_uint64(seed)))

    # ---- device-resident API (torch tensors) ----
    def set_cloud_torch(self, xyz_t, cam_t, stream=None):
        """xyz_t: float32 CUDA tensor (N, 3) or (N, 8) contiguous; cam_t: int32 CUDA tensor (N,) or None."""
        assert xyz_t.is_cuda and xyz_t.is_contiguous()
        self._keep = [xyz_t, cam_t]
        self.n = xyz_t.shape[0]
        self._check(self.lib.agh_set_cloud_device(
            self._h, C.c_void_p(xyz_t.data_ptr()), C.c_int64(xyz_t.stride(0) * 4),
            C.c_void_p(cam_t.data_ptr()) if cam_t is not None else None, C.c_int64(self.n),
            C.c_void_p(stream) if stream else None))

    def find_hands_torch(self, samples_t, out_t, nout_t, calculates_antipodal: bool = False, stream=None):
        """samples_t int32 CUDA (S,), out_t uint8 CUDA (cap*160,), nout_t int64 CUDA (1,).  Asynchronous."""
        S = samples_t.shape[0]
        cap = out_t.numel() // 160
        self.last_samples = S
        self._check(self.lib.agh_find_hands_device(
            self._h, C.c_void_p(samples_t.data_ptr()), C.c_int64(S), C.c_int(1 if calculates_antipodal else 0),
            C.c_void_p(out_t.data_ptr()), C.c_int64(cap), C.c_void_p(nout_t.data_ptr()),
            C.c_void_p(stream) if stream else None))

    def classify_torch(self, keep_t=None, stream=None):
        self._check(self.lib.agh_classify_device(self._h, C.c_void_p(keep_t.data_ptr()) if keep_t is not None else None,
                                                 C.c_void_p(stream) if stream else None))
