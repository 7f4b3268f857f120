/*
 * agh.h -- C ABI of libagile_grasp_hip.so, the MI355X-native (gfx950) grasp-hypothesis search.
 *
 * This is the drop-in boundary for agile_grasp's per-sample hot path.  The reference has no FFI; the seam is
 * a set of C++ methods (paths relative to the reference repository):
 *
 *   agh_create / agh_destroy        <- HandSearch::HandSearch(...)               include/agile_grasp/hand_search.h:77-85
 *   agh_set_cloud[_device]          <- kd-tree build inside HandSearch::findHands src/agile_grasp/hand_search.cpp:10-11
 *   agh_find_hands[_device]         <- HandSearch::findHands(cloud, pts_cam_source, indices, ...)
 *                                                                                 include/agile_grasp/hand_search.h:101-104,
 *                                                                                 src/agile_grasp/hand_search.cpp:4-62
 *   agh_load_svm[_file]             <- CvSVM::load in Learning::classify          src/agile_grasp/learning.cpp:185
 *   agh_classify                    <- Learning::classify(hands, svm, cam_pos)    include/agile_grasp/learning.h:122-123,
 *                                                                                 src/agile_grasp/learning.cpp:165-247
 *   agh_hypothesis                  <- GraspHypothesis                            include/agile_grasp/grasp_hypothesis.h:46-231
 *
 * The header-only C++ adapter in include/agile_grasp_amd/ keeps the reference's class and method names on top of
 * this ABI.  Conventions: every function returns AGH_OK (0) or a negative agh_status; no
 * exception crosses the ABI; all buffers are caller-owned; one context per host thread; a context owns its HIP
 * stream unless a stream is passed in.  There is NO CPU fallback: without a usable HIP device agh_create fails.
 */
#ifndef AGH_H
#define AGH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGH_VERSION 1

typedef enum agh_status
{
  AGH_OK = 0,
  AGH_ERR_INVALID_ARGUMENT = -1,
  AGH_ERR_NO_DEVICE = -2,       /* no HIP device / wrong architecture: the product path never falls back to the CPU */
  AGH_ERR_HIP = -3,             /* a HIP runtime call failed; see agh_last_error */
  AGH_ERR_CAPACITY = -4,        /* output buffer too small, or a neighbourhood exceeds the kernels' LDS capacity */
  AGH_ERR_NO_CLOUD = -5,
  AGH_ERR_NO_SVM = -6,
  AGH_ERR_IO = -7,
  AGH_ERR_STATE = -8,
  AGH_ERR_RETRY = -9            /* the call's result is incomplete because the context ran in a cheaper configuration than
                                 * this input needs; it has switched itself (for good): repeat the call.  Two cases: a Taubin
                                 * neighbourhood beyond the first capacity class of the kernels (the launches of the larger
                                 * classes are skipped until a cloud needs them), and a rank that overflowed its exchange
                                 * segment in a sharded search (both conditions reach every rank through the segment
                                 * headers, so all ranks repeat together).  Host-buffer entry points repeat by themselves; the
                                 * asynchronous device variants report it at the next agh_synchronize. */
} agh_status;

#define AGH_NORMALS_DETERMINISTIC 0 /* Quadric(is_deterministic = true): all neighbours (quadric.cpp:194-212) */
#define AGH_NORMALS_RAND50 1        /* HandSearch default: 50 draws of glibc rand() % n in sample order (quadric.cpp:177-193) */

typedef struct agh_params
{
  double finger_width;        /* find_grasps.cpp:13 */
  double hand_outer_diameter; /* find_grasps.cpp:14 */
  double hand_depth;          /* find_grasps.cpp:15 */
  double hand_height;         /* find_grasps.cpp:17 */
  double init_bite;           /* find_grasps.cpp:16 */
  double nn_radius_taubin;    /* hand_search.h:85 (0.03) */
  double nn_radius_hands;     /* hand_search.h:85 (0.08) */
  double nn_radius_normals;   /* hand_search.cpp:20 (0.01) */
  double cam_origin[2][3];    /* translations of cam_tf_left / cam_tf_right (hand_search.cpp:72-74) */
  int32_t normals_mode;       /* AGH_NORMALS_* */
  uint32_t rand_seed;         /* srand() seed for AGH_NORMALS_RAND50 */
  int32_t device;             /* HIP device ordinal */
  int32_t profile;            /* 1: time every kernel with HIP events (agh_get_timing); 2: only k_hand_sweep (start / stop events
                                 attached to its dispatch); 3: the same on every fourth call (a timed launch costs ~6 us) */
} agh_params;

/* One grasp hypothesis, fixed size (160 B).  The variable-size points_for_learning_ of the reference
 * (grasp_hypothesis.h:220) stays on the device as an 80x100 occupancy image consumed by agh_classify. */
typedef struct agh_hypothesis
{
  double axis[3];      /* getAxis() */
  double approach[3];  /* getApproach() */
  double binormal[3];  /* getBinormal() */
  double bottom[3];    /* getGraspBottom() */
  double surface[3];   /* getGraspSurface() */
  double width;        /* getGraspWidth() */
  int32_t sample;      /* position in the sample-index list */
  int32_t orientation; /* 0..7, angle = -pi + k*pi/4 (rotating_hand.cpp:13-15) */
  int32_t cam_source;  /* getCamSource() */
  int32_t n_in_box;    /* columns of points_for_learning_ */
  uint8_t half_antipodal, full_antipodal; /* isHalfAntipodal(), isFullAntipodal() */
  uint8_t svm_keep;    /* set by agh_classify: 1 iff CvSVM::predict == 1 (learning.cpp:225-227) */
  uint8_t valid;
  int32_t finger_index; /* eroded hand index (finger_hand.cpp:190) */
  int32_t depth_index;  /* successful deepen steps (finger_hand.cpp:204-225) */
  int32_t epoch;        /* stamp of the agh_find_hands* call that produced the record (process-wide counter, never 0):
                           the device-side state behind agh_classify / agh_get_learning_points / agh_get_packed_images
                           belongs to ONE call, and a record with another stamp must not be matched against it */
} agh_hypothesis;

/* Per-sample local frame (Quadric's results: quadric.h getters) -- for stage-wise parity tests and plotting. */
typedef struct agh_frame
{
  double sample[3];
  double normal[3];
  double axis[3];
  double binormal[3];
  double params[10];
  double eigenvalue;
  int32_t n_nb;
  int32_t majority_cam;
  int32_t max_index;
  int32_t valid;
} agh_frame;

/* Kernel times of the last find_hands call, milliseconds, measured with HIP events on the context's stream. */
#define AGH_TIMING_SLOTS 16
typedef struct agh_timing
{
  float ms[AGH_TIMING_SLOTS];
  const char* name[AGH_TIMING_SLOTS];
  int32_t n;
  float total_ms;
} agh_timing; /* (this layout is frozen: a caller built against an earlier header passes a buffer of exactly this size;
                 what was added later has its own getter, agh_get_timing_counts) */

typedef struct agh_ctx agh_ctx;

void agh_default_params(agh_params* p);
int agh_create(const agh_params* p, agh_ctx** out);
void agh_destroy(agh_ctx* ctx);
const char* agh_last_error(const agh_ctx* ctx); /* ctx may be NULL: error of the last failed agh_create */

/* Upload (host pointers) or adopt (device pointers) a cloud and build the uniform search grid on the GPU.
 * xyz: x,y,z float32 at byte offset 0 of each point; stride_bytes = 12 (packed) or 32 (pcl::PointXYZRGBA).
 * cam_source: 0/1 per point (Eigen::VectorXi pts_cam_source), may be NULL (all 0).
 * The host variant returns when xyz and cam_source have been READ (the caller may free or overwrite them at once); the grid
 * build is then still queued on the context's stream, in front of whatever uses the cloud next -- a search on another stream
 * waits for it first -- and an asynchronous failure of the build surfaces at that call's synchronisation.  That promise holds
 * for pageable AND for page-locked sources (hipHostMalloc / hipHostRegister): a copy from page-locked memory is truly
 * asynchronous, so the call then waits for the two copies (not for the build) before it returns.  Upload from page-locked
 * memory if the caller can: a pageable upload goes through the runtime's staging buffers. */
int agh_set_cloud(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, const int32_t* cam_source, int64_t n);
int agh_set_cloud_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, const int32_t* d_cam_source,
  int64_t n, void* hip_stream);

/* A BATCH of clouds in one context (BASELINE config C5: a batch of 8 x 300k-point clouds): the n_clouds clouds lie end to
 * end in one point array, cloud k = points [offsets[k], offsets[k + 1]) (offsets: n_clouds + 1 host integers, offsets[0] =
 * 0; at most 64 clouds, 2^30 points in total).  Every cloud gets its own search grid, so a radius search only sees the
 * points of its own cloud; point and sample indices of all later calls are positions in the common array.  One
 * agh_find_hands* call then searches samples of ALL clouds in one launch set -- thousands of independent work-groups more
 * per kernel, which is what fills the GPU when a single cloud's 2000 samples do not -- and agh_hypothesis::sample is the
 * position in that call's sample list, as always.  All clouds share the context's hand geometry; each may have its own camera
 * origins (agh_set_cloud_cam_origins below; without it, the context's).  agh_set_cloud* is the batch of one. */
int agh_set_cloud_batch(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, const int32_t* cam_source, const int64_t* offsets,
  int32_t n_clouds);
int agh_set_cloud_batch_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, const int32_t* d_cam_source,
  const int64_t* offsets, int32_t n_clouds, void* hip_stream);

/* Camera origins per cloud of a batch (two sensor pairs in one cell, two capture sessions in one directory -- the reference sets
 * up one Localization per rig with setCameraTransforms): row k (2 x 3 doubles, as agh_params::cam_origin) is used for every sample
 * and point of cloud k in place of the context's own origins -- the sign of the Taubin normals and the majority-camera vector, the
 * camera-side test of the hand orientations, and source_to_center of every occupancy image (the classifier's and the three
 * training images).  cam_origin == NULL (n_clouds ignored) clears the table.  1 <= n_clouds <= 64; a non-finite entry is
 * AGH_ERR_INVALID_ARGUMENT.
 * The table belongs to the context and is sticky: it survives new clouds and new batches until it is cleared or replaced.  The
 * caller's buffer has been read when the call returns (it is staged in pinned memory of the context); the upload is queued on the
 * context's stream, in front of whatever searches next -- a search on another stream waits for it first; searches of the previous
 * table that still run on another stream must have finished, as before a new cloud.
 * The table is checked against the bound batch at the calls that use the origins -- agh_find_hands*, agh_find_hands_sharded*,
 * agh_localize* (a batch of one: one row) and agh_localize_batch* (capture k = cloud k: n_captures rows): if the batch does not have
 * exactly the table's number of clouds, the call returns AGH_ERR_INVALID_ARGUMENT, the error text names both counts, and nothing is
 * launched (a sharded call stays collective: the rank takes part without searching and every rank returns an error).  A table of
 * one row on a single cloud is legal and gives exactly the results of a context created with those origins.  With no table every
 * result and every launch is what it is without this call.  Between agh_localize_begin and _end the setter returns AGH_ERR_STATE;
 * the chain and its in-call repeats search with the table that was set when it began.  The ranks of a communicator must hold the
 * same table (the parameter check of agh_comm_init* covers the one held then).
 * Hand geometry stays per context: per-cloud geometry would need per-cloud finger tables and is not offered.
 * agh_get_cloud_cam_origins copies the table held (host-side, allowed mid-chain) and returns its rows, 0 = none; AGH_ERR_CAPACITY
 * if cap_clouds is smaller. */
int agh_set_cloud_cam_origins(agh_ctx* ctx, const double* cam_origin, int32_t n_clouds);
int agh_get_cloud_cam_origins(agh_ctx* ctx, double* cam_origin_out, int32_t cap_clouds);

/* The head of Localization::localizeHands (localization.cpp:17-45) on the GPU, followed by the grid build: camera id of
 * raw point i = (i >= size_left); removal of points with a non-finite coordinate (skipped when dense != 0, like
 * pcl::removeNaNFromPointCloud on an is_dense cloud) WITHOUT re-indexing the camera ids (the reference's behaviour);
 * workspace box {xmin,xmax,ymin,ymax,zmin,zmax} (filterWorkspace, :216-245); per-camera voxelisation with cell_size
 * (voxelizeCloud, :247-355; the reference passes 0.003) in lexicographic voxel order, camera 0 block first.  The
 * voxelised cloud becomes the context's cloud (as after agh_set_cloud) and can be read back with agh_get_cloud.
 * The device variant synchronises hip_stream once per cloud for the voxel count (which sizes the search grid); the lattice
 * size, which sizes the voxel bitmap, costs a second synchronisation only for the first cloud of a context or when a cloud's
 * lattice outgrew the bitmap kept from the previous one.  The host variant returns when the caller's buffer has been read;
 * the grid build is still queued on the context's stream (as after agh_set_cloud).  AGH_ERR_CAPACITY if the kept points
 * span more than 2^33 lattice cells. */
int agh_preprocess(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, int64_t size_left, int dense,
  const double workspace[6], double cell_size, int64_t* n_voxels_out);
int agh_preprocess_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, int64_t size_left,
  int dense, const double workspace[6], double cell_size, int64_t* n_voxels_out, void* hip_stream);
/* HandleSearch::findHandles + Handle (handle_search.cpp:4-128, handle.cpp:3-74) on a list of hypotheses (normally the
 * ones Learning::classify kept; grasp_localizer.cpp:103 passes min_inliers from the launch file and min_length 0.005).
 * handles_out receives up to handle_cap records, inlier_idx_out the concatenated inlier lists (indices into hands, in
 * the order handle.cpp sees them).  At most 8192 hands and 2048 inliers per seed (AGH_ERR_CAPACITY beyond). */
typedef struct agh_handle
{
  double axis[3];         /* Handle::getAxis: principal direction of the inliers' axes (sign: that of the first inlier) */
  double center[3];       /* getCenter: grasp bottom of the inlier nearest the middle of the handle */
  double approach[3];     /* getApproach */
  double binormal[3];     /* approach x axis */
  double hands_center[3]; /* getHandsCenter: grasp surface of that inlier */
  double width;           /* getWidth: mean grasp width of the inliers */
  int32_t n_inliers;
  int32_t first_inlier;   /* offset of this handle's inliers in inlier_idx_out */
} agh_handle;
int agh_find_handles(agh_ctx* ctx, const agh_hypothesis* hands, int64_t n_hands, int32_t min_inliers, double min_length,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, int64_t* n_handles_out);

/* The chain the reference's online caller runs per cloud (GraspLocalizer::localizeGrasps, grasp_localizer.cpp:95-103:
 * localizeHands -> predictAntipodalHands -> findHandles) as ONE call with ONE synchronisation: raw capture in, handles out.
 * Preprocessing (as agh_preprocess), grid build, sample selection, hand search, classification (as agh_classify), compaction of
 * the kept hands and the handle search (as agh_find_handles) are queued on the context's stream without a host round trip in
 * between: the voxel count, the hypothesis count and the number of kept hands stay on the device, launches are sized for their
 * bounds (n, 8 x n_samples, min(8 x n_samples, 8192)).  The results equal those of the four separate calls on the same
 * samples, bit for bit.  The first cloud of a context (no voxel bitmap to speculate with yet) and a cloud whose lattice
 * outgrew the bitmap take the preprocessing's own synchronisations once.
 *
 * sample_idx: n_samples indices into the VOXELISED cloud (localizeHands' `indices`; validated on the device:
 * AGH_ERR_INVALID_ARGUMENT), or NULL: n_samples indices are drawn on the device -- one per stratum
 * [k N / S, (k + 1) N / S) of the N voxels, offset splitmix64(sample_seed ^ k * 0x9E3779B97F4A7C15) % width, i.e. sorted,
 * distinct, every point equally likely (hand_search.cpp:36-39 draws a uniform subset with pcl::RandomSample seeded by the
 * clock: not reproducible, never part of parity); with N < S every point is a sample.  The list can be read back (samples_out).
 * classify != 0: Learning::classify between the search and the handle search (needs agh_load_svm*); 0: every hypothesis
 * is handed to the handle search (at most 8192).
 * hands_out (optional, hands_cap records): the hands the handle search ran on, in list order -- inlier_idx_out indexes them.
 * filters_boundaries != 0 (1; any other value but 0 is AGH_ERR_INVALID_ARGUMENT): Localization::filterHands
 * (localization.cpp:364-388) between the search and the classifier, as the reference's nodes run it (grasp_localizer.cpp:21,
 * nodes/test.cpp:72) -- a hypothesis whose grasp surface lies closer than MIN_DIST = 0.02 to a face of `workspace` (the box the
 * preprocessing crops with), |surface[k / 2] - workspace[k]| < 0.02 for some k, is dropped.  The results then equal
 * agh_find_hands -> filterHands -> agh_classify -> agh_find_handles on the same samples, bit for bit: hands_out, n_hands and
 * inlier_idx_out refer to the filtered (and, with classify, kept) list; n_hypotheses stays the search's unfiltered count; the
 * 8192-hand limit of the handle search counts the hands that survive the filter.  A filtered hypothesis is never classified:
 * its device-side record carries svm_keep = 0, and no HOG descriptor or SVM sum is computed for it.
 * After the call the context holds the voxelised cloud and the search's results like after the separate calls
 * (agh_get_cloud, agh_get_frames, agh_get_images ...). */
typedef struct agh_localize_params
{
  int64_t size_left;       /* camera id of raw point i = (i >= size_left) */
  int32_t dense;           /* as agh_preprocess */
  int32_t classify;
  double workspace[6];
  double cell_size;        /* the reference passes 0.003 */
  const int32_t* sample_idx;
  int64_t n_samples;
  uint64_t sample_seed;
  int32_t min_inliers;     /* grasp_localizer.cpp:103: from the launch file */
  int32_t filters_boundaries; /* 0: off; 1: Localization::filterHands between the search and the classifier (above) */
  double min_length;       /* 0.005 */
} agh_localize_params;
typedef struct agh_localize_result
{
  int64_t n_voxels, n_hypotheses, n_hands, n_handles, n_inlier_idx;
} agh_localize_result;
int agh_localize(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
/* The same with the raw capture already in device memory (a depth pipeline that runs on the GPU): d_xyz is read in place with
 * the caller's stride and must stay valid until the call returns; the results still come back into host buffers.  Without the
 * 8 MB upload of a 700k-point capture the chain is 0.16 ms shorter. */
int agh_localize_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
/* The same chain as two calls, so that the NEXT capture goes up while this one is searched (the caller of
 * grasp_localizer.cpp:95-103 is handed one cloud after the other; the 8 MB upload of a 700k-point capture is 0.16 ms of a
 * 0.8 ms call, serial in front of everything):
 *   agh_localize_begin(ctx, cloud k)      queues the whole chain of cloud k and returns without waiting
 *   agh_localize_stage(ctx, cloud k + 1)  copies capture k + 1 into the context's second raw buffer on a stream of its own,
 *                                         beside cloud k's kernels (a pageable source: the call lasts as long as the copy)
 *   agh_localize_end(ctx, outputs)        the one synchronisation; cloud k's results, exactly agh_localize's
 *   agh_localize_begin(ctx, cloud k + 1)  recognises the staged capture (same pointer, stride and count): no upload
 * agh_localize(...) is begin + end.  One chain may be in flight (AGH_ERR_STATE for a second begin, or an end without a begin).
 * Between begin and end the chain owns the context's buffers and its cloud: only agh_localize_stage, agh_localize_depth_stage,
 * agh_localize_end,
 * agh_get_cloud_cam_origins, agh_get_depth_filter, agh_get_voxel_filter, agh_get_hand_filter, agh_get_hand_clearance,
 * agh_get_handle_ranking, agh_synchronize (it waits, and leaves the chain's results to agh_localize_end), agh_last_error,
 * agh_destroy, the host-side counters (agh_get_timing, agh_get_timing_counts, agh_get_grid_stats, agh_get_grid_desc) and the
 * communicator's bookkeeping (agh_comm_rank, agh_comm_init*, agh_comm_destroy, agh_comm_inject_fault,
 * agh_comm_set_segment_records, agh_comm_last_*) may be called on the context.  Every other call on it returns AGH_ERR_STATE
 * without touching anything: agh_set_cloud*, agh_set_cloud_cam_origins, agh_set_depth_filter, agh_set_voxel_filter, agh_set_hand_filter, agh_set_hand_clearance,
 * agh_set_handle_ranking, agh_rank_handles, agh_preprocess*, agh_find_hands*, agh_classify*,
 * agh_find_handles, agh_localize* (agh_localize_depth_batch*, agh_localize_masked*, agh_localize_masked_begin,
 * agh_localize_depth_masked*, agh_localize_depth_masked_begin, agh_localize_labeled*, agh_localize_depth_labeled*,
 * agh_localize_clustered*, agh_localize_depth_clustered*, agh_localize_clustered_fit*, agh_localize_depth_clustered_fit*,
 * agh_localize_batch_masked*, agh_localize_batch_masked_begin*, agh_localize_depth_batch_masked*,
 * agh_localize_depth_batch_masked_begin*, agh_localize_batch_labeled*, agh_localize_batch_labeled_begin*,
 * agh_localize_depth_batch_labeled*, agh_localize_depth_batch_labeled_begin*, agh_localize_batch_clustered*,
 * agh_localize_batch_clustered_begin*, agh_localize_depth_batch_clustered*, agh_localize_depth_batch_clustered_begin*,
 * agh_localize_batch_clustered_fit*, agh_localize_batch_clustered_fit_begin*, agh_localize_depth_batch_clustered_fit* and
 * agh_localize_depth_batch_clustered_fit_begin* among them), agh_deproject, agh_deproject_batch,
 * agh_remove_plane, agh_get_cloud, agh_get_sample_mask_count, agh_get_label_counts, agh_get_cluster_info,
 * agh_get_cluster_labels, agh_get_plane_fit, agh_get_plane_fit_candidates, agh_get_batch_mask_counts,
 * agh_get_batch_label_counts, agh_get_batch_cluster_info, agh_get_batch_cluster_labels, agh_get_batch_plane_fit,
 * agh_get_batch_plane_fit_candidates, agh_get_depth_filter_counts, agh_get_voxel_filter_counts, agh_get_hand_filter_counts, agh_get_hand_clearance_counts,
 * agh_get_handle_scores, agh_get_handle_ranking_counts, agh_get_hand_margins,
 * agh_fuse_depth, agh_fuse_depth_device, agh_get_depth_fusion_counts, agh_get_fused_depth and every getter of device results (frames, normals,
 * neighbour counts, images, HOG, learning points, plane results, agh_get_epoch), agh_load_svm*, the training calls
 * (agh_set_training_images, agh_get_training_images, agh_hog_images, agh_train_svm), agh_set_profile and agh_selftest_math.  The
 * sharded calls are collective and do not return early: on such a context they take part without searching, and every rank of
 * the call returns an error (this one AGH_ERR_STATE); the chain is not disturbed.
 * The capture handed to begin must stay valid
 * and unchanged until the agh_localize_end of its chain has returned, the one handed to stage until the agh_localize_end of the
 * chain that adopts it has (a pageable source has been read when agh_localize_stage returns; a pinned one is read asynchronously);
 * sample_idx is copied by begin.  A staged capture that the next begin does not name is dropped (its copy may still be running:
 * keep the source until that begin's agh_localize_end, which waits for the copy too, or an agh_synchronize). */
int agh_localize_begin(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_localize_params* lp);
int agh_localize_stage(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n);
int agh_localize_end(agh_ctx* ctx, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);

/* The same chain straight from DEPTH IMAGES: a depth sensor's driver produces a depth image per camera, and a host-side
 * nodelet expands it into the points agh_localize takes (/camera/depth_registered/points, launch/single_camera_grasps.launch).
 * Here the images go up as they are (2 or 4 bytes per pixel instead of 12..32 per point) and one kernel, k_deproject,
 * back-projects them on the context's stream into the raw buffer an upload would have filled; the chain then runs unchanged on
 * that packed stride-12 array of sum W x H points, image 0 first, pixels row-major.
 * n_images is 1 or 2; image k is camera k: a point's camera id is its image's index.  lp->size_left and lp->dense are
 * ignored: the chain runs with size_left = W0 x H0 and dense = 1.  With dense = 1 the voxeliser ranks by RAW index and its
 * workspace comparisons are false for NaN, so the invalid pixels fall out there and every kept point keeps the right id;
 * dense = 0 would shift camera 1's first points into camera 0 (the reference does not re-index after its NaN removal) --
 * harmless for a few drop-outs, wrong for the 10-40 % invalid pixels of a depth image.
 * Arithmetic, all float32, evaluated left to right, never contracted: the host rounds once, kx = (float) (1.0 / fx), ky,
 * cxf = (float) cx, cyf, and the twelve pose entries; per pixel (u, v): z = (float) raw * depth_scale (U16) or the pixel
 * (F32); x = (((float) u - cxf) * z) * kx, y likewise with v, cyf, ky; X = ((r00 * x + r01 * y) + r02 * z) + t0, Y and Z
 * with their rows of the pose.  An invalid pixel (U16: raw 0; F32: a value not in (0, +inf)) writes three quiet NaNs.
 * agh_localize_depth returns, bit for bit (epoch aside), what agh_localize returns for the array agh_deproject writes, with
 * stride 12, size_left = W0 x H0, dense = 1 and the same lp.
 * The pose does NOT set the camera origins, which stay the context's (agh_params::cam_origin, or the one-row table of
 * agh_set_cloud_cam_origins): a caller sets cam_origin[k] to the translation of image k's pose.
 * AGH_ERR_INVALID_ARGUMENT, the text naming the image and the field, nothing launched: NULL images or data; n_images not 1
 * or 2; width or height outside 1..8192; a row_stride_bytes below width x element size or no multiple of the element size;
 * an unknown format; for agh_localize_depth_device a data pointer that is no multiple of the element size (a host image may
 * lie anywhere: its copy repacks it); fx or fy zero or non-finite; a non-finite cx, cy or pose entry; for U16 a depth_scale that is non-finite
 * or <= 0.  Everything else -- AGH_ERR_NO_SVM, AGH_ERR_CAPACITY, AGH_ERR_STATE mid-chain, the one-row rule for a camera-origin
 * table, the repeats inside the call -- is as for agh_localize. */
#define AGH_DEPTH_U16 0   /* uint16 raw units (ROS 16UC1); 0 = no reading */
#define AGH_DEPTH_F32 1   /* float32 metres (ROS 32FC1); valid iff 0 < z < +inf */
typedef struct agh_depth_image
{
  const void* data;          /* row-major, row v at data + v * row_stride_bytes */
  int32_t width, height;     /* 1 .. 8192 each */
  int64_t row_stride_bytes;  /* >= width * element size, a multiple of the element size */
  int32_t format;            /* AGH_DEPTH_* */
  float depth_scale;         /* U16: metres per unit (0.001f); F32: ignored */
  double fx, fy, cx, cy;     /* pinhole intrinsics, pixels */
  double pose[12];           /* row-major 3x4 [R|t]: camera optical frame -> cloud frame */
} agh_depth_image;
/* Introspection and tests: the points k_deproject makes of the images, sum W x H packed float32 triples, into host memory.
 * Returns the point count, or AGH_ERR_CAPACITY if cap_points is smaller.  Refused (AGH_ERR_STATE) while a chain is in flight. */
int agh_deproject(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, float* xyz_out, int64_t cap_points);
/* Host images (uploaded with their rows packed into a depth buffer of the context) ... */
int agh_localize_depth(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
/* ... or images whose `data` are device pointers, aligned to the element size, read in place with their row strides (valid
 * until the call returns). */
int agh_localize_depth_device(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
/* The two halves, as agh_localize_begin / agh_localize_stage: a chain begun with agh_localize_depth_begin is collected with
 * agh_localize_end; agh_localize_depth_stage copies the NEXT capture's images into a second depth buffer on the stage stream
 * (allowed between begin and end, and without a chain), and the next agh_localize_depth_begin adopts them when n_images and
 * every (data, width, height, row_stride_bytes, format) match: the depth buffers change places, the chain waits for the copy,
 * nothing is uploaded (intrinsics, scale and pose are read at begin).  The context still has ONE staged set, of any kind: a
 * newer stage of any kind replaces it; a begin of another kind drops it, and the chain waits for its copy; a points begin
 * never adopts depth images and a depth begin never adopts points.  The image records are copied by the calls; the pixel
 * buffers follow agh_localize_begin's lifetime rules. */
int agh_localize_depth_begin(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_localize_params* lp);
int agh_localize_depth_stage(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images);

/* The same chains with their samples drawn UNDER A MASK: "find grasps on this object".  A caller of the chain owns a capture and
 * a per-point (per-pixel) object mask from a detector or segmenter; explicit sample_idx cannot express it, because they index
 * the voxelised cloud, which is built inside the call.  The whole cloud stays in the search (the hand sweep needs the scene for
 * its collision tests); only where the SAMPLES are drawn is restricted.
 * mask: one byte per raw point of the capture, packed, entry i belongs to raw point i; any non-zero byte means "eligible".
 *  1. A voxel of the voxelised cloud is eligible iff at least one raw point with a non-zero mask byte was kept by the
 *     preprocessing (finite unless dense, inside workspace) and falls into it -- into the voxel of the point's own camera block
 *     (camera ids by the voxeliser's rule: rank in the NaN-free cloud >= size_left for dense = 0, the raw index for dense = 1).
 *     A masked point that the preprocessing drops makes nothing eligible.
 *  2. E is the list of the eligible voxel indices, ascending; M = |E|.
 *  3. Sample k of S = n_samples is E[stratum draw of agh_localize with M in the place of N]; with M < S the first M samples are
 *     E[0..M) and the rest are unused slots, INT32_MIN in samples_out, as for N < S.  M = 0 is no error: AGH_OK with zero
 *     hypotheses, hands and handles.
 *  4. Everything behind the sample list is the chain of agh_localize, unchanged: the results equal, bit for bit (epoch aside),
 *     what agh_localize returns on the same capture and lp with sample_idx set to the list samples_out reports (INT32_MIN
 *     slots included: an explicit list may carry them, they are skipped).  With an all-ones mask the call equals agh_localize
 *     with sample_idx = NULL and the same seed.
 *  5. A mask together with lp->sample_idx != NULL is AGH_ERR_INVALID_ARGUMENT: an explicit list needs no mask.
 *  6. The mask stage runs for n_samples = 0 too: agh_get_sample_mask_count is what a caller sizes S with.
 * agh_localize_masked_device: d_xyz and d_mask are device pointers, read in place (valid until the call returns); d_mask may
 * have any byte alignment.  agh_localize_masked_begin queues the chain as agh_localize_begin does; agh_localize_end collects it.
 * The depth forms: masks[k] belongs to images[k], same width and height, one byte per pixel, row v at
 * data + v * row_stride_bytes (>= width).  data == NULL: NO pixel of that image is eligible (a caller with one mask for a
 * two-camera capture wants samples on the masked view only); all NULL is AGH_ERR_INVALID_ARGUMENT.
 * agh_localize_depth_masked equals agh_localize_masked on the array agh_deproject writes (stride 12, size_left = W0 x H0,
 * dense = 1) with the masks' rows packed end to end in image order, a NULL mask contributing zeros; a masked invalid pixel is a
 * NaN point and is dropped like any other.  agh_localize_depth_masked_device: the images' and the masks' data are device
 * pointers.
 * Errors, nothing launched: a NULL mask (points) or NULL masks (depth), or a mask row stride below the width ->
 * AGH_ERR_INVALID_ARGUMENT; every validation, error text and status of the unmasked twin; AGH_ERR_STATE while a chain or a
 * batch is in flight.
 * Staging: a masked begin of host data never adopts a staged set; it drops a pending one as a begin of another kind does (the
 * chain waits for its copy).  The mask is copied by begin into a buffer of the context (depth masks repacked to one byte per
 * pixel, image after image); a device mask of the points form is read in place and follows the capture's lifetime rules.  The
 * repeats inside the call (the lattice that outgrew the kept bitmap, the capacity classes) need the caller's mask in no other
 * way than they need the caller's capture.  One more bitmap of the voxel bitmap's size is held by a context that made a masked
 * call; the chain's one synchronisation stays one.
 * Not built: a _stage call for masks, for one capture or a batch (the batch forms are agh_localize_batch_masked* below);
 * masks and label images in the batch chains mixed in one call (agh_localize_batch*, agh_localize_depth_batch*; label images
 * alone: agh_localize_batch_labeled* below; for ONE capture, several objects with one sample list each:
 * agh_localize_labeled* below); sharded variants. */
typedef struct agh_sample_mask
{
  const uint8_t* data;       /* one byte per pixel, non-zero = eligible; NULL: no pixel of this image is */
  int64_t row_stride_bytes;  /* >= the image's width */
} agh_sample_mask;
int agh_localize_masked(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const uint8_t* mask,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
int agh_localize_masked_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const uint8_t* d_mask,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
int agh_localize_masked_begin(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const uint8_t* mask,
  const agh_localize_params* lp);
int agh_localize_depth_masked(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, int32_t n_images,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
int agh_localize_depth_masked_device(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, int32_t n_images,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result);
int agh_localize_depth_masked_begin(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, int32_t n_images,
  const agh_localize_params* lp);
/* The eligible voxels (M) of the last masked chain this context collected.  AGH_ERR_STATE if the last chain collected had no
 * mask, if there was none, or while a chain is in flight. */
int agh_get_sample_mask_count(agh_ctx* ctx, int64_t* n_eligible);

/* The same chains with one sample list PER OBJECT of a LABEL IMAGE: "grasps on each of these objects" (bin picking).  An instance
 * segmenter hands over one label image with several objects in it; K calls of agh_localize_masked would upload, voxelise and
 * grid the same capture K times and synchronise K times.  Here the capture is preprocessed ONCE, the search runs ONCE over the
 * n_objects x S samples, the kept hands are compacted into one list per object and the handle search runs ONCE for all lists,
 * side by side (the tail of agh_localize_batch, with "object" in the place of "capture"); one synchronisation.
 * labels: one byte per raw point (per pixel); 0 = no object, j + 1 = object j, 0 <= j < n_objects; a byte above n_objects
 * belongs to no object (it is not an error: a device label array cannot be validated without a round trip).
 *  1. 1 <= n_objects <= 64 (the lists the batch tail holds).
 *  2. lp->n_samples = S is the number of samples of EACH object and lp->sample_seed is every object's seed;
 *     n_objects x S <= 2^24.  A violation of 1 or 2 is AGH_ERR_INVALID_ARGUMENT, nothing launched; so is lp->sample_idx != NULL,
 *     as with a mask.
 *  3. Eligibility is the mask rule, per object: a voxel is eligible for object j iff at least one raw point with label j + 1
 *     was kept by the preprocessing and falls into it, in its own camera block.  One voxel may be eligible for several objects.
 *     E_j is the ascending list of object j's eligible voxel indices, M_j = |E_j|.
 *  4. Sample k of object j is E_j[stratum draw of agh_localize with M_j in the place of N]; with M_j < S the list is E_j followed
 *     by INT32_MIN slots.  M_j = 0 is no error: that object has zero hypotheses, hands and handles.
 *  5. The search runs once over the n_objects x S samples in object order, on the whole cloud; classification, the boundary
 *     filter (filters_boundaries) and the handle search are those of agh_localize.
 *  6. Outputs are laid out as agh_localize_batch's: every output is the concatenation of the objects' spans in object order;
 *     results[j] (n_objects records) holds object j's counts and the starts of its spans; samples_out holds n_objects x S voxel
 *     indices; agh_hypothesis::sample is the position in object j's own list; object j's inlier indices point into its own span
 *     of hands_out; results[j].r.n_voxels is the cloud's voxel count, for every j.  The 8192-hand limit applies per object (the
 *     error text names the object).  Buffers that are too small: AGH_ERR_CAPACITY with every results[j] filled.
 *  7. Equality, with AGH_NORMALS_DETERMINISTIC: object j's span of every output and results[j].r equal, bit for bit (epoch
 *     aside), what agh_localize_masked returns for the same capture and lp with mask[i] = (labels[i] == j + 1), and M_j equals
 *     that call's agh_get_sample_mask_count; with n_objects = 1 and labels 0 / 1 the call equals agh_localize_masked.
 *     With AGH_NORMALS_RAND50 the rand() stream runs through the call's whole sample list, hence through the objects in order:
 *     only object 0 equals its masked twin.
 *  8. The depth forms: labels[k] belongs to images[k] as a mask does (same width and height, row v at data + v *
 *     row_stride_bytes); data == NULL: no pixel of that image belongs to an object; all NULL is AGH_ERR_INVALID_ARGUMENT.  The
 *     chain runs with size_left = W0 x H0 and dense = 1, and the call equals agh_localize_labeled on the array agh_deproject
 *     writes, with the label rows packed end to end and a NULL image contributing zeros.
 *  9. Every validation, status and error text not named here is the masked twin's: AGH_ERR_STATE while a chain or a batch of any
 *     kind is in flight; a pending staged set is dropped, as a masked begin drops it; the repeats inside the call (a lattice that
 *     outgrew the kept bitmap, the capacity classes, the declined handle walk) work as in the masked call and read the labels
 *     where the first pass left them.  agh_localize_labeled_device / agh_localize_depth_labeled_device: the points (images') and
 *     labels' data are device pointers, read in place, the labels at any byte alignment.
 * 10. One synchronisation in the steady state, as agh_localize; the label stage adds none.  After the call the context holds
 *     the voxelised cloud as a single bound cloud.  A context that made a labelled call holds one 32-bit word per word of the
 *     voxel bitmap and one 64-bit object set per raw point -- nothing of n_objects x the lattice.
 * agh_get_label_counts: the M_j of the last labelled chain this context collected (n_objects entries).  AGH_ERR_STATE if the
 * last chain collected was not labelled (agh_get_sample_mask_count returns AGH_ERR_STATE after a labelled call), if there was
 * none, or while a chain is in flight; AGH_ERR_CAPACITY if cap_objects is below n_objects.
 * Not built: _begin / _end and _stage forms; labels in the batch chains beyond 64 lists per call (the batch forms are
 * agh_localize_batch_labeled* below); more than 64 objects; labels wider than a byte;
 * sharded variants. */
typedef struct agh_label_image   /* depth form: as agh_sample_mask, the bytes being labels */
{
  const uint8_t* data;           /* NULL: no pixel of this image belongs to an object */
  int64_t row_stride_bytes;      /* >= the image's width */
} agh_label_image;
struct agh_localize_batch_result;  /* (defined below, with agh_localize_batch) */
int agh_localize_labeled(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const uint8_t* labels, int32_t n_objects,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_labeled_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const uint8_t* d_labels,
  int32_t n_objects, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_depth_labeled(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels, int32_t n_images,
  int32_t n_objects, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_depth_labeled_device(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels, int32_t n_images,
  int32_t n_objects, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_get_label_counts(agh_ctx* ctx, int64_t* n_eligible, int32_t cap_objects);

/* The labelled chain WITHOUT A SEGMENTER: "grasps on each object on this table".  A fixed cell knows its support plane from
 * calibration; given that plane, the objects are the connected components of the voxels that stand above it.  The call finds them
 * on the device, behind the grid build and in front of the sample draw, and from there on it IS agh_localize_labeled with
 * n_objects = max_objects: one preprocessing, one search over max_objects x S samples on the WHOLE cloud (the table stays in the
 * hand sweep's collision tests: nothing is removed), one handle search for all lists, one synchronisation, no host round trip.
 * Everything below is stated on the voxelised cloud of the call: voxel v is a position in it, p_v its float32 point.  Both
 * cameras' voxels take part; camera ids play no role.
 *  1. Height: h = ((a * x + b * y) + c * z) + d in double on the float coordinates, evaluated left to right, never contracted.
 *     Voxel v is FOREGROUND iff min_height < h < max_height, both strict; a non-finite h is background.
 *  2. Adjacency: dx = p_u.x - p_v.x, dy, dz likewise, in float32; d2 = (dx * dx + dy * dy) + dz * dz in float32, never
 *     contracted; u and v are adjacent iff d2 <= (float) (tolerance * tolerance).  The rule is symmetric by construction.
 *  3. Components are the connected components of that graph over the foreground voxels; a component's id is its smallest voxel
 *     index, its size its voxel count.
 *  4. Objects are the components of size >= min_voxels, ordered by size descending, ties to the smaller id; object j is the j-th
 *     of them, j < K = max_objects.  Further components are counted (agh_cluster_info::n_components) but get no list; with
 *     fewer than K objects the remaining lists are empty (M_j = 0 is a legal empty object, as for labels).  A voxel belongs to
 *     at most one object.
 *  5. E_j is the ascending list of object j's voxel indices, M_j its length; sample k of object j is E_j[stratum draw of
 *     agh_localize with M_j in the place of N], and with M_j < S the list is E_j followed by INT32_MIN slots: rule 4 of
 *     agh_localize_labeled with another source of the object sets.
 *  6. Outputs are laid out as agh_localize_labeled's, results[j] for j < K.  Equality, with AGH_NORMALS_DETERMINISTIC: object
 *     j's span of every output (handles, inlier indices, hands, samples) and results[j].r equal, bit for bit (epoch aside), what
 *     agh_localize returns on the same capture and lp with object j's reported list as explicit sample_idx, INT32_MIN slots
 *     carried.  The result does not depend on the order of any atomic operation.
 *  7. AGH_ERR_INVALID_ARGUMENT, the text naming the field, nothing launched: a non-finite field; |a^2 + b^2 + c^2 - 1| > 1e-6;
 *     min_height >= max_height; tolerance <= 0 or > 0.05 (a larger ball walks hundreds of grid cells per voxel; the bound is a
 *     stated limit, not a measured one); min_voxels < 1; max_objects outside 1 .. 64; max_objects x n_samples > 2^24;
 *     lp->sample_idx != NULL; cp == NULL.
 *  8. Everything else is as agh_localize_labeled: AGH_ERR_NO_SVM; AGH_ERR_CAPACITY with results filled; AGH_ERR_STATE while a
 *     chain or a batch of any kind is in flight; the one-row rule for a camera-origin table; the repeats inside the call (the
 *     lattice that outgrew the kept bitmap re-enters with the same agh_cluster_params; the capacity classes and the declined
 *     handle walk run on the lists already drawn); no foreground at all is AGH_OK with K empty objects.  The _device forms read
 *     device points (images) in place; the depth forms run with size_left = W0 x H0 and dense = 1 and equal the points form on
 *     the array agh_deproject writes.
 *  9. agh_get_cluster_info / agh_get_cluster_labels describe the last chain this context collected if it was clustered: the
 *     counts, the M_j and ids (max_objects entries each, 0 and -1 for a list without an object; either array may be NULL), and
 *     per voxel of the bound cloud 0 or j + 1 (the return value is the voxel count; AGH_ERR_CAPACITY if cap is below it).
 *     AGH_ERR_STATE after a chain of another kind, if there was none, or while a chain is in flight; after a clustered call
 *     agh_get_label_counts and agh_get_sample_mask_count return AGH_ERR_STATE.
 * 10. A context that made a clustered call holds two 32-bit words and a byte per raw point beside the labelled chain's buffers.
 * Not built: more than 64 objects (a caller without a calibrated plane: agh_localize_clustered_fit below finds it inside the
 * call); _begin / _end, _stage and sharded forms of this
 * single-capture call.  Several captures per call, _begin / _end included, are agh_localize_batch_clustered* below; batch and sharded
 * chains do not combine.  The 8192-hand limit holds per object. */
typedef struct agh_cluster_params
{
  double plane[4];      /* a, b, c, d of the support plane, (a, b, c) a unit vector pointing from the table towards the objects */
  double min_height;    /* a voxel is FOREGROUND iff min_height < h < max_height, both strict */
  double max_height;
  double tolerance;     /* two foreground voxels are adjacent iff their distance is <= tolerance (rule 2) */
  int32_t min_voxels;   /* components with fewer voxels are no objects (>= 1) */
  int32_t max_objects;  /* K: 1 .. 64; the call has K lists, as agh_localize_labeled with n_objects = K */
} agh_cluster_params;
void agh_default_cluster_params(agh_cluster_params* p);  /* plane 0,0,1,0; heights 0.01 / 0.5; tolerance 0.01; min_voxels 50; max_objects 16 */
int agh_localize_clustered(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_clustered_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_depth_clustered(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_depth_clustered_device(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
typedef struct agh_cluster_info
{
  int64_t n_foreground, n_components, n_objects;  /* n_components: all, before min_voxels; n_objects: those with a list (<= K) */
} agh_cluster_info;
int agh_get_cluster_info(agh_ctx* ctx, agh_cluster_info* info, int64_t* n_voxels /* M_j */, int32_t* ids /* smallest voxel index */,
  int32_t cap_objects);
int agh_get_cluster_labels(agh_ctx* ctx, uint8_t* labels_out, int64_t cap);  /* per voxel of the bound cloud: 0 or j + 1 */

/* The clustered chain WITH THE SUPPORT PLANE FITTED ON THE DEVICE: a mobile base, a hand-held sensor or a cell whose table moves
 * has no calibrated plane.  agh_localize_clustered_fit finds the dominant plane of the voxelised cloud behind the preprocessing
 * and in front of the cluster stage, writes it into a record in device memory that the cluster kernels read, and from there on IS
 * agh_localize_clustered: nothing returns to the host, the chain keeps its one synchronisation, the table stays in the cloud.  The
 * finder is this project's own, made for the device (agh_remove_plane restates PCL's serial RANSAC and deletes the plane):
 * candidates drawn in parallel, one scoring pass with integer counts, a refit from exact integer moments.
 * Everything is stated on the voxelised cloud of the call: N its voxels, p_v voxel v's float32 point promoted to double; all
 * arithmetic is double, never contracted, products and sums evaluated in the order written.
 *  1. Draw.  Candidate c < C = n_candidates takes the voxels i_s = splitmix64(seed ^ ((3 c + s) * 0x9E3779B97F4A7C15)) % N,
 *     s = 0, 1, 2 (the generator of agh_localize's sample strata; the product wraps at 2^64).  N < 3 is "no plane": every
 *     candidate is invalid and its reported indices are -1.
 *  2. Candidate.  u = p1 - p0, v = p2 - p0; n = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x);
 *     l2 = (n_x n_x + n_y n_y) + n_z n_z.  The candidate is INVALID, count 0 and a reported plane of zeros, unless l2 is finite
 *     and > 0 (a repeated index is such a case).  Otherwise n /= sqrt(l2), three divisions, and d = -((n_x x0 + n_y y0) + n_z z0).
 *  3. Score.  Voxel v is an inlier of c iff fabs(((a x + b y) + c z) + d) <= distance_threshold: rule 1 of
 *     agh_localize_clustered's evaluation order.  The count is an integer.
 *  4. Choice.  The candidate with the largest count, ties to the smaller c; found = (its count >= max(min_inliers, 3)).  No
 *     early termination: every candidate is scored.
 *  5. Refit (refine and found).  Over the chosen candidate's inliers the float32 differences dx = x - x0, dy, dz against the
 *     candidate's own p0; an inlier with any |difference| >= 8 is left out; q = (int64) rint((double) dx * 65536.0) and likewise;
 *     n_refit and the int64 sums Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of the q and their products (|q| < 2^19 and at most
 *     2^24 contributors: no sum can overflow; derived, not measured).  Skipped when n_refit < 3 or > 2^24.  Nn = (double) n_refit;
 *     m_x = ((double) Sx / Nn) * 2^-16 and likewise; M00 = ((double) Sxx / Nn) * 2^-32 - m_x m_x, and likewise M01, M02, M11,
 *     M12, M22; (a, b, c) = the unit eigenvector of M's smallest eigenvalue (the library's smallest_eigvec3: one Householder
 *     reflection, bisection, twisted factorisation).  A non-finite component leaves the candidate's plane standing; otherwise
 *     c_x = (double) x0 + m_x and likewise, d = -((a c_x + b c_y) + c c_z), refined = 1.
 *  6. Orientation.  s = ((a o_x + b o_y) + c o_z) + d at camera 0's origin in force for the call (agh_params::cam_origin[0], or
 *     row 0 of a one-row agh_set_cloud_cam_origins table); s < 0 negates all four numbers; s == 0 or a non-finite s leaves them.
 *  7. Use.  With found, the call equals agh_localize_clustered on the same capture, lp and cp with cp.plane set to the reported
 *     plane, bit for bit (epoch aside): every output, results[j], agh_get_cluster_info and agh_get_cluster_labels.  Without found
 *     it returns AGH_OK with K empty objects and no foreground (the device record carries a NaN plane, background by rule 1 of
 *     agh_localize_clustered), and the reported plane is zeros.
 *  8. The same call twice gives the same bits: counts and sums are integers, nothing depends on the order of an atomic operation.
 *  9. The _device forms read device points (images) in place; the depth forms equal the points form on the array agh_deproject
 *     writes, as agh_localize_depth_clustered does.
 * 10. cp->plane is ignored and not validated; every other field of cp and lp follows agh_localize_clustered's rules 7 and 8.
 *     AGH_ERR_INVALID_ARGUMENT, the text naming the field, nothing launched: n_candidates outside 1 .. 256; refine not 0 or 1;
 *     min_inliers < 3; reserved != 0; distance_threshold not finite, <= 0 or > 0.05; fp == NULL.  AGH_ERR_NO_SVM, AGH_ERR_CAPACITY
 *     with results filled, AGH_ERR_STATE while a chain or a batch is in flight, the one-row rule for a camera-origin table and the
 *     repeats inside the call (a lattice that outgrew the kept bitmap re-enters with the same fit parameters) are the clustered
 *     call's.
 * 11. agh_get_plane_fit and agh_get_plane_fit_candidates describe the last chain this context collected if it was a fitted one
 *     (AGH_ERR_STATE otherwise, and while a chain is in flight): the result record -- it arrives in pinned memory with the chain's
 *     one synchronisation -- and, for introspection (the call copies from the device and may synchronise), per candidate its three
 *     voxel indices, its plane BEFORE refit and orientation, and its count; any of the three arrays may be NULL, the return value
 *     is C, AGH_ERR_CAPACITY if cap is below it.  After a fitted call agh_get_cluster_info and agh_get_cluster_labels work as
 *     after agh_localize_clustered; agh_get_label_counts and agh_get_sample_mask_count return AGH_ERR_STATE.
 * 12. A context's first fitted call allocates 256 candidates (indices, planes, counts), ten sums and one record on the device,
 *     and one result record in pinned memory: nothing per point.
 * Not built: batch forms of THIS call's own (the batch forms are agh_localize_batch_clustered_fit* below, _begin / _end forms
 * among them: one fit stage for up to 64 captures); _begin / _end forms for a single capture; _stage forms; sharded forms; more
 * than 256 candidates; a termination rule. */
typedef struct agh_plane_fit_params
{
  int32_t  n_candidates;        /* C: 1 .. 256 */
  int32_t  refine;              /* 0 or 1 */
  int32_t  min_inliers;         /* >= 3: a best count below it is "no plane" */
  int32_t  reserved;            /* must be 0 */
  double   distance_threshold;  /* finite, > 0, <= 0.05 */
  uint64_t seed;
} agh_plane_fit_params;
typedef struct agh_plane_fit_result
{
  double  plane[4];             /* the plane the cluster stage used; zeros when found == 0 */
  int64_t n_voxels, n_inliers, n_refit;
  int32_t best_candidate;       /* -1: none */
  int32_t found, refined, reserved;
} agh_plane_fit_result;
void agh_default_plane_fit_params(agh_plane_fit_params* p);  /* 128 candidates; refine 1; min_inliers 3; threshold 0.01; seed 1 */
int agh_localize_clustered_fit(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_plane_fit_params* fp,
  const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_clustered_fit_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const agh_plane_fit_params* fp,
  const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_depth_clustered_fit(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_plane_fit_params* fp,
  const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, struct agh_localize_batch_result* results);
int agh_localize_depth_clustered_fit_device(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out,
  int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  struct agh_localize_batch_result* results);
int agh_get_plane_fit(agh_ctx* ctx, agh_plane_fit_result* out);
int agh_get_plane_fit_candidates(agh_ctx* ctx, int32_t* idx /* 3 per candidate */, double* planes /* 4 per candidate */,
  int64_t* counts, int32_t cap);

/* The chain of agh_localize over a BATCH of captures in one call, with ONE synchronisation (offline evaluation over a
 * directory of PCD pairs, a cell with several sensors or arms): 1 <= n_captures <= 64, fewer than 2^30 raw points in all.
 * Capture k is xyz[k] (stride_bytes[k], n[k] points) with its own record lp[k]: size_left, dense, workspace, sample_idx /
 * n_samples / sample_seed are per capture; classify, cell_size, min_inliers, min_length and filters_boundaries must be equal
 * across the batch (AGH_ERR_INVALID_ARGUMENT otherwise).  Hand geometry is the context's; camera origins are the context's, or
 * per capture with agh_set_cloud_cam_origins (row k = capture k's rig).  The voxelised captures lie end to end in one cloud
 * batch (capture k = cloud k), are searched in one launch set, classified together, and their kept hands go through the handle
 * search side by side, one list per capture.
 * Capture k's results equal what agh_localize returns for capture k alone on the same samples, bit for bit: n_voxels,
 * n_hypotheses, every field of every hand record but epoch (one call stamps one epoch), every handle field and the inlier
 * lists.  agh_hypothesis::sample is the position in capture k's own sample list, samples_out holds capture-local voxel indices
 * (sum of n_samples entries, in capture order), capture k's inlier indices point into capture k's own span of hands_out, and
 * a drawn list is agh_localize's strata over capture k's own voxel count with capture k's seed.  Every output is the
 * concatenation of the captures' spans in capture order; results[k] (n_captures records) holds capture k's counts and the
 * start of its spans.  The 8192-hand limit of the handle search applies per capture.
 * Errors: output buffers too small -> AGH_ERR_CAPACITY with every results[k] filled (size and repeat); a sample index outside
 * its capture's voxelised cloud -> AGH_ERR_INVALID_ARGUMENT, the error text names the capture; classify without an SVM ->
 * AGH_ERR_NO_SVM; a call while an agh_localize_begin chain is in flight -> AGH_ERR_STATE, the chain untouched (and
 * agh_localize_begin refuses while a batch runs).  Capacity-class AGH_ERR_RETRY is repeated inside the call, as agh_localize
 * does.  Synchronisations: one in the steady state.  The first batch of a context (no voxel bitmaps yet) takes one more, for the
 * lattice sizes; a batch whose lattices outgrew the kept bitmap slots is run once more, in the same call, with slots sized from
 * them.  Every stage -- preprocessing (a bitmap slot per capture), search, classification, compaction and handle search --
 * runs once for the whole batch.  With filters_boundaries the boundary filter is applied at the
 * compaction, against each hand's own capture's workspace (the classifier runs on every hypothesis of the batch).
 * After the call the context holds the voxelised batch as its bound batch of clouds, as after agh_set_cloud_batch (agh_get_cloud,
 * agh_get_frames, agh_get_images ... see the whole batch); a failed call leaves the context as a failed agh_localize does. */
typedef struct agh_localize_batch_result
{
  agh_localize_result r; /* this capture's counts, exactly as agh_localize reports them for it */
  int64_t first_handle, first_inlier_idx, first_hand, first_sample; /* its spans in the concatenated outputs */
} agh_localize_batch_result;
int agh_localize_batch(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
/* The same with the captures in device memory: xyz[k] (a host array of device pointers) is read in place with stride_bytes[k]
 * and must stay valid until the call returns. */
int agh_localize_batch_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
/* The same batch as two calls, so that the NEXT batch's captures go up while this one is searched (a walk over a directory of
 * PCD pairs; the upload of 8 x 8 MB is a third of a blocking call, serial in front of its first kernel):
 *   agh_localize_batch_begin(ctx, batch k)      validates as agh_localize_batch does (same status codes and error texts), copies
 *                                               the pointer, stride and count arrays, the lp records and every explicit
 *                                               sample_idx list, queues the whole chain and returns without waiting.  The first
 *                                               batch of a context, or one after the kept bitmap slots were dropped, takes the
 *                                               synchronisation for the lattice sizes here.
 *   agh_localize_batch_stage(ctx, batch k + 1)  copies the next batch's host captures, packed end to end, into the context's
 *                                               second raw buffer on a stream of its own, beside batch k's kernels (pageable
 *                                               sources: the call lasts as long as the copies; pinned ones are read
 *                                               asynchronously).  Allowed with or without a chain in flight.
 *   agh_localize_batch_end(ctx, outputs)        the one synchronisation, the repeats agh_localize_batch runs inside the call
 *                                               (from the raw buffer the batch was read from: a staged set is not touched), and
 *                                               batch k's outputs, results[k], status and bound batch, exactly
 *                                               agh_localize_batch's -- AGH_ERR_CAPACITY with results filled included.  The chain
 *                                               is over whatever it returns.
 *   agh_localize_batch_begin(ctx, batch k + 1)  adopts the staged set if n_captures and every (xyz[k], stride_bytes[k], n[k])
 *                                               are the staged ones: the two raw buffers change places, nothing is uploaded.
 * agh_localize_batch(...) is begin + end; agh_localize_batch_begin_device reads device captures in place (nothing to stage).
 * The context has ONE chain and ONE staged set, of either kind.  A begin of either kind while a chain of either kind is in
 * flight (agh_localize_depth_batch* and agh_localize_depth_batch_begin* included, agh_localize_masked*,
 * agh_localize_masked_begin, agh_localize_depth_masked* and agh_localize_depth_masked_begin too, and agh_localize_labeled*
 * and agh_localize_depth_labeled*, agh_localize_batch_masked*, agh_localize_batch_masked_begin*,
 * agh_localize_depth_batch_masked* and agh_localize_depth_batch_masked_begin*, agh_localize_batch_labeled*,
 * agh_localize_batch_labeled_begin*, agh_localize_depth_batch_labeled* and agh_localize_depth_batch_labeled_begin*;
 * agh_localize_clustered* and agh_localize_depth_clustered*; agh_localize_clustered_fit* and
 * agh_localize_depth_clustered_fit*; agh_localize_batch_clustered*,
 * agh_localize_batch_clustered_begin*, agh_localize_depth_batch_clustered* and agh_localize_depth_batch_clustered_begin*;
 * agh_localize_batch_clustered_fit*, agh_localize_batch_clustered_fit_begin*, agh_localize_depth_batch_clustered_fit* and
 * agh_localize_depth_batch_clustered_fit_begin*;
 * agh_deproject_batch, agh_get_sample_mask_count, agh_get_label_counts, agh_get_cluster_info, agh_get_cluster_labels,
 * agh_get_plane_fit, agh_get_plane_fit_candidates, agh_get_batch_mask_counts, agh_get_batch_label_counts, agh_get_batch_cluster_info,
 * agh_get_batch_cluster_labels, agh_get_batch_plane_fit, agh_get_batch_plane_fit_candidates, agh_set_depth_filter,
 * agh_get_depth_filter_counts, agh_set_voxel_filter, agh_get_voxel_filter_counts, agh_set_hand_filter,
 * agh_get_hand_filter_counts, agh_set_hand_clearance and agh_get_hand_clearance_counts are refused as well, and so are
 * agh_set_handle_ranking, agh_rank_handles, agh_get_handle_scores, agh_get_handle_ranking_counts, agh_get_hand_margins,
 * agh_fuse_depth, agh_fuse_depth_device, agh_get_depth_fusion_counts and agh_get_fused_depth; agh_get_hand_clearance
 * and agh_get_handle_ranking are host-side and allowed, as agh_get_hand_filter),
 * agh_localize_batch_end without an agh_localize_batch_begin in flight (agh_localize_end for a batch chain likewise):
 * AGH_ERR_STATE, the chain untouched.  Between agh_localize_batch_begin and _end the calls allowed on the context are those
 * listed at agh_localize_begin, with agh_localize_batch_stage / agh_localize_batch_end (and agh_localize_stage) in place of
 * agh_localize_end; every other call returns AGH_ERR_STATE without touching anything, a sharded call makes the rank a bystander,
 * agh_destroy waits for both streams.  agh_set_cloud_cam_origins is among the refused: the batch searches with the table held at
 * begin, whose row count is checked there.
 * A newer stage call of either kind replaces what was staged.  agh_localize_batch_begin adopts only a staged batch,
 * agh_localize_begin only a capture of agh_localize_stage; a staged set that a begin (of host captures) does not adopt is
 * dropped, and the chain waits for its copies.
 * Lifetimes: the arrays, lp records and sample lists handed to begin may be freed when it returns.  The captures handed to
 * begin must stay valid and unchanged until the agh_localize_batch_end of their chain has returned; those handed to stage until
 * the end of the chain that adopts or drops them has (pageable ones have been read when stage returns), or an
 * agh_synchronize. */
int agh_localize_batch_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures);
int agh_localize_batch_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures);
int agh_localize_batch_stage(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n, int32_t n_captures);
int agh_localize_batch_end(agh_ctx* ctx, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);

/* The batch chain straight from DEPTH IMAGES: the two fast ways into the chain together (a cell with several sensor pairs owns
 * depth images, not points).  `images` is ONE flat array in capture order: n_images[k] is 1 or 2, capture k's images are the
 * next n_images[k] records, image j of a capture is its camera j.  One kernel, k_deproject_batch, back-projects every image of
 * every capture (up to 64 x 2 = 128 views, a table in device memory) on the context's stream into the raw buffer: capture k's
 * points packed, stride 12, image 0 first, pixels row-major, the captures end to end in capture order -- what
 * agh_localize_batch builds from host points -- and the batch chain runs unchanged from there.  lp[k].size_left and
 * lp[k].dense are ignored: capture k runs with size_left = W0 x H0 of its own image 0 and dense = 1 (see agh_localize_depth).
 * The arithmetic is agh_localize_depth's, word for word.
 * Equality: capture k's results equal, bit for bit (epoch aside), what agh_localize_depth returns for capture k's images alone
 * with lp[k]; they therefore also equal agh_localize_batch on the arrays agh_deproject writes, with stride 12,
 * size_left = W0 x H0 and dense = 1.
 * Everything of agh_localize_batch holds unchanged: the concatenated outputs and their spans, results[k], the per-capture
 * 8192-hand limit, AGH_ERR_CAPACITY with every results[k] filled (size and repeat), the fields of lp that must be equal
 * across the batch, the synchronisations, the repeats inside the call (they re-run from the points in the raw buffer), and the
 * voxelised batch bound as the context's batch of clouds afterwards (camera id = image index).
 * Camera origins stay the context's, or row k of agh_set_cloud_cam_origins for capture k: the poses do NOT set them.
 * AGH_ERR_INVALID_ARGUMENT, nothing launched: n_captures outside 1..64; an n_images[k] other than 1 or 2; 2^30 points or more
 * in all; every per-image rule of agh_localize_depth, the text naming the capture and the image ("capture 3, image 1: fx must
 * be finite and not zero").  AGH_ERR_NO_SVM, the row count of a camera-origin table (n_captures rows) and AGH_ERR_STATE while a
 * chain of any kind is in flight are as for agh_localize_batch.
 * agh_localize_depth_batch_device: the images' `data` are device pointers, aligned to the element size, read in place with
 * their row strides, valid until the call (or the chain's agh_localize_batch_end) has returned.
 * agh_localize_depth_batch_begin[_device] queue the chain as agh_localize_batch_begin does and are collected with
 * agh_localize_batch_end; between the two the rules of agh_localize_batch_begin hold.  The records, n_images and lp are copied
 * by begin; host pixel buffers must stay valid and unchanged until agh_localize_batch_end has returned.  A begin of host images
 * drops a pending staged set of any kind (agh_localize_stage, agh_localize_depth_stage, agh_localize_batch_stage), and the
 * chain waits for its copies.
 * agh_deproject_batch: introspection and tests, as agh_deproject -- the points k_deproject_batch makes of host images, into
 * host memory; returns the point count, AGH_ERR_CAPACITY if cap_points is smaller, AGH_ERR_STATE while a chain is in flight or
 * a batch runs.
 * Not built: a _stage call for depth batches (for a single capture the staged depth stream measured 0.035 to 0.04 ms slower
 * than the staged points stream, and the images are a sixth of the bytes: to be revisited only with a measurement), and
 * points and depth captures mixed in one batch. */
int agh_localize_depth_batch(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images, const agh_localize_params* lp,
  int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_depth_batch_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_depth_batch_begin(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_begin_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures);
int agh_deproject_batch(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images, int32_t n_captures, float* xyz_out,
  int64_t cap_points);

/* A DEPTH FILTER for every call that back-projects depth images: a real sensor's image holds, along every depth edge, flying
 * pixels -- readings interpolated between an object and what lies behind it -- besides speckles and readings outside the
 * sensor's trusted range.  Back-projected they are voxels floating in the free space beside objects, exactly where the hand
 * sweep tests finger clearance, and one of them vetoes a placement.  agh_set_depth_filter makes the deprojection itself look at
 * every pixel's neighbours; no host pass over the pixels, no new agh_localize_* variant.
 * The setting is sticky, per context, as agh_set_cloud_cam_origins' table is: it holds until it is cleared (NULL) or replaced,
 * across clouds, batches and chains, and costs no device work (the parameters travel as kernel arguments).  With a filter
 * set, EVERY call that deprojects applies it: agh_deproject and agh_deproject_batch, and all agh_localize_depth* and
 * agh_localize_depth_batch* forms (_device, _begin, _begin_device, _masked, _labeled, _clustered, _clustered_fit).
 * agh_localize_depth_stage stays a pure copy: the filter that counts is the one set when the adopting begin deprojects.  The
 * repeats inside a call re-run from the points already in the raw buffer: they neither filter again nor count again.  With no
 * filter set every launch is exactly what it was: k_deproject / k_deproject_batch with their arguments.
 * The filter, per image, independently of every other image (an image's neighbours are its own pixels only: the two images of a
 * capture, and the captures of a batch, never support one another).  The host rounds the four doubles once to float32:
 * ja = (float) max_jump_abs, jr = (float) max_jump_rel, zlo = (float) z_min, zhi = (float) z_max.
 *  1. Depth and validity are k_deproject's: U16: z = (float) raw * depth_scale, valid iff raw != 0; F32: z is the pixel, valid
 *     iff 0 < z < +inf.
 *  2. A valid pixel is IN RANGE iff z >= zlo && z <= zhi (both ends inclusive).
 *  3. For an in-range pixel p: tol = ja + (jr * z_p), float32, not contracted.  Its support is the number of pixels q != p of the
 *     (2 radius + 1)^2 window around p that are inside the image, in range, and satisfy fabsf(z_q - z_p) <= tol.  Pixels outside
 *     the image never support.  Support is counted on the in-range set of step 2, NOT on the filter's own output: one pass,
 *     independent of any order.  The tolerance follows the CENTRE pixel, so support is not symmetric: with jr > 0 a far pixel
 *     may count a nearer one that does not count it back.
 *  4. p is kept iff it is in range and its support is at least min_support.  A kept pixel's point is exactly what k_deproject
 *     writes for it (the same float32 expression, left to right); every other pixel writes the three quiet NaNs an invalid
 *     pixel writes, which the voxeliser, the masks, labels, clusters and the plane fit already handle.
 * agh_set_depth_filter checks every field: radius 1 or 2; min_support in 1 .. (2 radius + 1)^2 - 1; max_jump_abs and
 * max_jump_rel finite and >= 0; z_min finite and >= 0; z_max > z_min (+inf allowed).  A violation returns
 * AGH_ERR_INVALID_ARGUMENT, the text names the field, and the filter held before stays in force.  NULL clears the filter.
 * Mid-chain (single or batch) it returns AGH_ERR_STATE without touching the chain.
 * agh_get_depth_filter copies the filter held and returns 1, or returns 0 if none is set (host-side, allowed mid-chain).
 * agh_get_depth_filter_counts: per view of the last deprojection that ran with a filter, in launch order (capture k's images
 * follow capture k - 1's): n_valid = n_out_of_range + n_unsupported + n_kept.  Returns the number of views, or 0 if the last
 * deprojection ran unfiltered (or none ran); AGH_ERR_CAPACITY if cap_views is smaller; AGH_ERR_STATE mid-chain.  One small copy
 * and one synchronisation.
 * Not built: temporal filtering and hole filling inside the filter (a burst is fused ahead of it: agh_fuse_depth below),
 * lens distortion, per-image parameters (the points forms have a filter of their own: agh_set_voxel_filter below). */
typedef struct agh_depth_filter_params
{
  int32_t radius;        /* 1 or 2: window (2 radius + 1)^2 */
  int32_t min_support;   /* 1 .. (2 radius + 1)^2 - 1 */
  double max_jump_abs;   /* metres, finite, >= 0 */
  double max_jump_rel;   /* per metre of depth, finite, >= 0 */
  double z_min, z_max;   /* metres; z_min finite >= 0; z_max > z_min, may be +inf */
} agh_depth_filter_params;
typedef struct agh_depth_filter_counts
{
  int64_t n_valid;         /* pixels the format calls valid */
  int64_t n_out_of_range;  /* valid, outside [z_min, z_max] */
  int64_t n_unsupported;   /* in range, support below min_support */
  int64_t n_kept;
} agh_depth_filter_counts;
void agh_default_depth_filter_params(agh_depth_filter_params* p);  /* radius 1; min_support 3; 0.01 / 0.01; z_min 0; z_max +inf */
int agh_set_depth_filter(agh_ctx* ctx, const agh_depth_filter_params* fp);
int agh_get_depth_filter(agh_ctx* ctx, agh_depth_filter_params* out);
int agh_get_depth_filter_counts(agh_ctx* ctx, agh_depth_filter_counts* out, int32_t cap_views);

/* DEPTH FUSION: a burst of depth frames of ONE fixed camera, fused on the device into one depth image ahead of everything above.
 * Between two picks the scene is static and the driver delivers 5 to 15 frames; a single frame of a structured-light or stereo
 * sensor has 10 to 40 % invalid pixels, different ones in every frame, and millimetres of noise on the valid ones.  The sweep
 * treats every hole as free space and the noise roughens the surfaces the normals are fitted on.  agh_fuse_depth turns the burst
 * into one image in a buffer of the context and hands back an agh_depth_image whose `data` is that DEVICE pointer: the record
 * goes into every agh_*depth*_device call of the same context (single, batch, masked, labelled, clustered, fitted), so the depth
 * filter and the hand filter's observed-space test see the fused image.  No new chain variant, and no kernel of the chain changes.
 * One kernel, k_depth_fuse, reads the n_frames x W x H readings once and writes W x H.
 * agh_fuse_depth takes n_frames (1 .. 16) records of one camera: all of the same width, height and format; the row strides may
 * differ per frame; depth_scale, fx, fy, cx, cy and the twelve pose entries must be BIT-EQUAL in all frames (a difference is an
 * error: mixing cameras must not pass silently).  The host rounds once to float32: sa = (float) max_spread_abs,
 * sr = (float) max_spread_rel.  Every pixel is treated independently of every other pixel; frames are taken in ascending
 * frame index.
 *  1. READING AND VALIDITY are k_deproject's.  U16: valid iff raw != 0, and z = (float) raw * depth_scale.  F32: valid iff
 *     0 < z < +inf; NaN, negative values, both zeros and +inf are invalid.  m is the number of frames in which the pixel is valid.
 *  2. MEDIAN.  The valid readings sorted ascending (U16: the raw integers; F32: the floats); med is the LOWER median, element
 *     (m - 1) / 2 in integer division.  With two equally large clusters the nearer surface wins.
 *  3. CONSENSUS.  zm is the depth of med; tol = sa + (sr * zm), float32, left to right, never contracted.  A valid reading is in
 *     the consensus iff fabsf(z - zm) <= tol; the comparison is closed.  k is the number of consensus members.  The median is
 *     always a member: with sa = sr = 0 the consensus is the set of readings equal to the median, and the result is the median.
 *  4. DECISION, in this order.  m == 0: EMPTY.  m < min_valid: UNSUPPORTED.  k < min_valid: INCONSISTENT -- a pixel that keeps
 *     changing sides, where writing either side would be a guess.  Otherwise FUSED.  Every pixel that is not FUSED writes the
 *     format's invalid value: U16 writes 0, F32 writes a quiet NaN.
 *  5. VALUE of a FUSED pixel.  U16: (sum + k / 2) / k in unsigned integer arithmetic, sum the sum of the members' raw values (at
 *     most 16 x 65535).  F32: s is the first member, then s = s + z for every further member in frame order; the value is
 *     s / (float) k with a correctly rounded float32 division.  An overflowing sum writes +inf: an invalid pixel by rule 1 that
 *     still counts as FUSED.
 *  6. OUTPUT.  The slot's device buffer receives a W x H image of the frames' format with tight rows.  fused_out receives that
 *     pointer and row_stride_bytes = width x element size, and width, height, format, depth_scale, intrinsics and pose of frame
 *     0.  The record is a legal image for every agh_*depth*_device call of the same context, and stays valid until that slot is
 *     fused again or the context is destroyed.
 *  7. COUNTS per slot: n_pixels = n_empty + n_unsupported + n_inconsistent + n_fused; n_filled counts the FUSED pixels whose
 *     reading in the LAST frame was invalid -- the holes of the newest frame that the burst closed.
 * SLOTS run 0 .. 127: two images per capture for a full 64-capture depth batch.  A slot's buffer is made on first use and
 * regrown when an image is larger.
 * ORDERING.  The fuse is queued on the context's stream and returns without waiting for the kernel.  A chain called next on the
 * same context is behind it on that stream: agh_fuse_depth followed by agh_localize_depth_device needs no synchronisation in
 * between, and the chain's one synchronisation stays one.  agh_fuse_depth (host frames, packed into a staging buffer of the
 * context that the kernel reads) returns when the caller's frames have been READ, pageable or page-locked, as agh_set_cloud
 * does.  agh_fuse_depth_device: the frames' data are device pointers, aligned to the element size, read in place with their
 * strides; they must stay valid until the next synchronisation of the context.  The counts go to pinned memory;
 * agh_get_depth_fusion_counts (1, or 0 if the slot was never fused) and agh_get_fused_depth wait on an event recorded behind
 * that slot's kernel, a wait that is free once any later synchronisation has passed.  agh_get_fused_depth copies the slot's
 * image, rows tight, into pixels_out and its record (data: the device pointer) into record_out, which may be NULL; it returns
 * the bytes written, 0 if the slot was never fused, AGH_ERR_CAPACITY if cap_bytes is smaller than the image (record_out is filled
 * then too: width x height x element size says what is needed).
 * ERRORS, each AGH_ERR_INVALID_ARGUMENT, the text naming the frame and the field, nothing launched and the slot's previous image
 * untouched: NULL frames, params or fused_out; n_frames outside 1 .. 16; slot outside 0 .. 127; min_valid outside
 * 1 .. n_frames (the default of 2 with ONE frame is therefore refused: a single frame is passed with min_valid = 1); a spread
 * that is non-finite or negative; a non-zero reserved; per frame every rule agh_localize_depth applies to an image ("frame 3:
 * fx must be finite and not zero"); a frame that differs from frame 0 in a field that must be equal ("frame 2: cx differs from
 * frame 0").
 * MID-CHAIN (single or batch) agh_fuse_depth, agh_fuse_depth_device, agh_get_depth_fusion_counts and agh_get_fused_depth return
 * AGH_ERR_STATE without touching anything.
 * Not built: fusing the next burst under a chain in flight; a ring of frames kept by the context between calls (the device form
 * lets the caller own the ring); motion compensation; spatial hole filling; confidence outputs.
 * The contract is a numpy model the kernel matches bit for bit: tests/depth_fusion_cases.py. */
typedef struct agh_depth_fusion_params
{
  int32_t min_valid;       /* 1 .. n_frames */
  int32_t reserved;        /* 0 */
  double max_spread_abs;   /* metres, finite, >= 0 */
  double max_spread_rel;   /* per metre of depth, finite, >= 0 */
} agh_depth_fusion_params;
typedef struct agh_depth_fusion_counts
{
  int64_t n_pixels;        /* W x H */
  int64_t n_empty;         /* no frame valid */
  int64_t n_unsupported;   /* fewer than min_valid frames valid */
  int64_t n_inconsistent;  /* fewer than min_valid readings in the consensus */
  int64_t n_fused;
  int64_t n_filled;        /* fused, and invalid in the last frame */
} agh_depth_fusion_counts;
void agh_default_depth_fusion_params(agh_depth_fusion_params* p);  /* min_valid 2; 0.005 m; 0.005 per metre */
int agh_fuse_depth(agh_ctx* ctx, const agh_depth_image* frames, int32_t n_frames, const agh_depth_fusion_params* fp, int32_t slot,
  agh_depth_image* fused_out);
int agh_fuse_depth_device(agh_ctx* ctx, const agh_depth_image* frames, int32_t n_frames, const agh_depth_fusion_params* fp,
  int32_t slot, agh_depth_image* fused_out);
int agh_get_depth_fusion_counts(agh_ctx* ctx, int32_t slot, agh_depth_fusion_counts* out);
int agh_get_fused_depth(agh_ctx* ctx, int32_t slot, void* pixels_out, int64_t cap_bytes, agh_depth_image* record_out);

/* A VOXEL FILTER for every call that voxelises: the depth filter above only helps callers who hand over depth images.  A cloud
 * from a stereo matcher, a lidar, a fused map or a driver that already deprojected carries stray returns in free space; each
 * becomes a voxel of its own, in the space where the hand sweep tests finger clearance, and vetoes a placement.
 * agh_set_voxel_filter prunes voxels without enough occupied neighbours inside the voxeliser, on the bitmap it already holds
 * (k_vox_prune, between the mark and the count): no host pass over the points, no new agh_localize_* variant, and everything
 * downstream simply sees a smaller cloud.
 *  1. The lattice of each camera -- its origin (the per-camera minimum of the kept raw points), its dims, the voxel of a point
 *     -- is the unfiltered voxeliser's, unchanged: the filter never moves the minimum.  The result is the UNFILTERED voxel list
 *     with rows taken out: same order, same float32 coordinates for the survivors.  It is NOT the voxelisation of the raw points
 *     that survive, whose minimum, and with it every coordinate, could differ.
 *  2. Let O_c be the voxels camera c's kept points occupy.  The support of v = (ix, iy, iz) in O_c is the number of w in O_c,
 *     w != v, with dx^2 + dy^2 + dz^2 <= radius^2 in voxel units (an integer ball of B(radius) = 7, 33, 123, 257 positions for
 *     radius 1, 2, 3, 4).  Positions outside the lattice (a coordinate < 0 or >= its dim) never support.  The two cameras of a
 *     capture never support one another (their lattices have different origins), nor do the captures of a batch.
 *  3. v is kept iff its support is at least min_neighbors.  Support is counted on O_c, never on the filter's own output: one
 *     pass, independent of any order, not iterated.
 *  4. After the stage THE voxel bitmap is the pruned one: the voxel counts (n_voxels), the cloud (agh_get_cloud), the drawn
 *     samples' strata, masks, labels, clusters (agh_get_cluster_labels) and the plane fit all refer to the survivors.
 *  5. Masks and labels: a voxel is eligible, or carries object j, iff a masked / labelled kept raw point falls into a SURVIVING
 *     voxel; a point whose voxel was pruned marks nothing.
 *  6. The setting is sticky, per context, until it is cleared (NULL) or replaced, across clouds, batches and chains.  With a
 *     filter set EVERY call that voxelises applies it: agh_preprocess*, every agh_localize* form on points and on depth images
 *     (there it runs after the depth filter, if both are set), every batch form including _begin / _stage / _end streams, and the
 *     repeat inside a call after the lattice outgrew the bitmap.  agh_set_cloud* takes clouds as they are.  It costs no device
 *     work at set time (the two ints travel as kernel arguments); with no filter set every launch is exactly what it was.
 *  7. agh_set_voxel_filter checks both fields: radius 1 .. 4; min_neighbors 1 .. B(radius) - 1.  A violation returns
 *     AGH_ERR_INVALID_ARGUMENT, the text names the field, and the filter held before stays in force.  Mid-chain (single or
 *     batch) it returns AGH_ERR_STATE without touching the chain.  agh_get_voxel_filter copies the filter held and returns 1, or
 *     returns 0 if none is set (host-side, allowed mid-chain).
 *  8. agh_get_voxel_filter_counts: per capture of the last voxelisation, if it ran filtered: n_occupied = n_pruned + n_kept per
 *     camera, n_kept being the voxel count.  Returns the number of captures (1 for the single forms), or 0 if it ran unfiltered
 *     (or none ran); AGH_ERR_CAPACITY if cap_captures is smaller; AGH_ERR_STATE mid-chain.  One synchronisation, no copy: the
 *     counts ride in the voxeliser's pinned descriptor.
 *  9. A capture whose voxels are all pruned behaves as one whose points all fall outside the workspace: zero voxels, empty
 *     lists, no error; the other captures of a batch are untouched.
 * 10. The lattice limit stays 2^28 words.  With a filter set the context holds a SECOND bitmap of the first one's capacity (the
 *     voxeliser's bitmap memory doubles: 2 x 4 bytes x the lattice's words, per slot of a batch), made by the first filtered
 *     voxelisation, dropped and regrown with the first; AGH_ERR_HIP with hipMalloc's text if it does not fit.
 * Not built: iterated or statistical (mean-distance) removal; support across cameras or captures; per-capture parameters in a
 * batch; a filter for agh_set_cloud*, whose clouds the caller has voxelised. */
typedef struct agh_voxel_filter_params
{
  int32_t radius;         /* 1 .. 4, in voxels */
  int32_t min_neighbors;  /* 1 .. B(radius) - 1;  B = 7, 33, 123, 257 for radius 1, 2, 3, 4 */
} agh_voxel_filter_params;
typedef struct agh_voxel_filter_counts
{
  int64_t n_occupied[2];  /* voxels the kept points occupy, per camera */
  int64_t n_pruned[2];
  int64_t n_kept[2];      /* n_occupied = n_pruned + n_kept; the voxel count per camera */
} agh_voxel_filter_counts;
void agh_default_voxel_filter_params(agh_voxel_filter_params* p);  /* radius 2; min_neighbors 4 */
int agh_set_voxel_filter(agh_ctx* ctx, const agh_voxel_filter_params* fp);
int agh_get_voxel_filter(agh_ctx* ctx, agh_voxel_filter_params* out);
int agh_get_voxel_filter_counts(agh_ctx* ctx, agh_voxel_filter_counts* out, int32_t cap_captures);

/* A HAND FILTER on the way out: every agh_localize* call hands back each hand the sweep found collision-free, and a cell can
 * execute only some of them.  agh_set_hand_filter makes the chain itself drop, between the search and the classifier, the hands
 * that fail up to three tests (k_hand_filter, one drop byte per hypothesis): no second synchronisation, no classifier work on
 * hands nobody can use, and the 8192-hand limit of the handle search counts the survivors.  Each criterion is off in the
 * defaults; a hand counts under the FIRST criterion that drops it, in the order below.
 *  1. APPROACH CONE (approach_on): approach_dir is a unit vector, |a^2 + b^2 + c^2 - 1| <= 1e-6, min_approach_cos in [-1, 1].  A
 *     hand is dropped iff ((a0 * d0 + a1 * d1) + a2 * d2) < min_approach_cos, a = agh_hypothesis::approach (hand -> object),
 *     d = approach_dir: float64, left to right, never contracted.  The threshold is a cosine, so that it can lie exactly on a hand.
 *  2. APERTURE (width_on): finite, 0 <= min_width <= max_width.  Dropped iff width < min_width || width > max_width.
 *  3. OBSERVED SPACE (view_on; the depth forms only): the sweep treats everything without a point as free, so with one view
 *     the far side of every object is "free".  2 x probes_per_finger x 3 probes per hand sample the volume the two fingers
 *     sweep: with s the sample's point of the voxelised cloud (float32 widened), h = (bottom - s) . binormal, d the bite of
 *     the record's depth_index (the sweep's own table: init_bite, then += 0.005 depth_index times), n = probes_per_finger,
 *       c = h -+ (hand_outer_diameter / 2 - finger_width / 2)        (finger 0, finger 1)
 *       y = (d - hand_depth) + (j + 0.5) x (hand_depth / n)          (j = 0 .. n - 1)
 *       z = -hand_height, 0, +hand_height
 *       w = ((s + c x binormal) + y x approach) + z x axis           (per coordinate)
 *     and a probe is SEEN in image k iff, with e = w - t and q = R^T e from the image's float64 pose (q.x = (R00 e0 + R10 e1)
 *     + R20 e2, ...): q.z > 0; the pixel (floor(((fx q.x) / q.z + cx) + 0.5), floor(((fy q.y) / q.z + cy) + 0.5)) lies inside
 *     the image; the pixel is valid by its format's rule; and q.z <= (double) z_pix + depth_margin, z_pix the float32 depth
 *     as k_deproject computes it.  A probe seen in no image of its capture is unobserved; the hand is dropped iff more than
 *     max_unobserved probes are.  The images are read AS UPLOADED: the depth filter (agh_set_depth_filter) changes the points
 *     the chain makes of them, never what this test sees.  A pose whose rotation part is not orthonormal (an entry of
 *     |R^T R - I| above 1e-4) is AGH_ERR_INVALID_ARGUMENT, the text naming the image.  With view_on set EVERY agh_localize* form
 *     that takes points is refused with AGH_ERR_INVALID_ARGUMENT, nothing launched: the criterion needs depth images, and a
 *     safety filter must not silently not apply.
 *  A NaN in a tested field compares false and the hand is kept, as the boundary filter keeps it (a probe with a NaN coordinate
 *  is not counted as unobserved).  tests/hand_filter_cases.py is the numpy model the kernel matches decision for decision.
 *  The setting is sticky per context until cleared (fp == NULL) or replaced; setting it does no device work; an invalid field
 *  returns AGH_ERR_INVALID_ARGUMENT, the text names it, and the filter held before stays; mid-chain (single or batch) it
 *  returns AGH_ERR_STATE.  agh_get_hand_filter copies the filter held and returns 1, or 0 if none is set (host-side, allowed
 *  mid-chain).  It applies to every agh_localize* chain form, batches and _begin / _stage / _end streams included, and to
 *  their repeats; with filters_boundaries too a hand is dropped if either filter says so.  hands_out, the handles and the inlier
 *  lists are those of the stage-wise route over the surviving hands; n_hypotheses stays the search's unfiltered count.  The
 *  stage-wise and sharded calls (agh_find_hands*, agh_classify*) are not touched.  With no filter set nothing new is launched.
 *  agh_get_hand_filter_counts: one record per list of the last chain collected, in the order of its results (the call
 *  itself, a batch's captures, or the (capture, object) pairs), if it ran with a filter.  Returns the number of lists, 0 if it
 *  ran unfiltered (or none ran), AGH_ERR_CAPACITY if cap_lists is smaller, AGH_ERR_STATE mid-chain.  No copy, no
 *  synchronisation: the counts arrive in pinned memory with the chain's own synchronisation. */
typedef struct agh_hand_filter_params
{
  int32_t approach_on;        /* 0 / 1 */
  int32_t width_on;           /* 0 / 1 */
  int32_t view_on;            /* 0 / 1 */
  int32_t probes_per_finger;  /* 1 .. 16 */
  double approach_dir[3];     /* unit vector, cloud frame */
  double min_approach_cos;    /* -1 .. 1 */
  double min_width, max_width;  /* metres, 0 <= min <= max */
  double depth_margin;        /* metres, finite, >= 0 */
  int32_t max_unobserved;     /* >= 0 */
  int32_t reserved;           /* 0 */
} agh_hand_filter_params;
typedef struct agh_hand_filter_counts
{
  int64_t n_hypotheses;        /* what the search found for the list */
  int64_t n_dropped_approach;
  int64_t n_dropped_width;
  int64_t n_dropped_unobserved;
  int64_t n_kept;              /* n_hypotheses less the three (before the classifier and the boundary filter) */
} agh_hand_filter_counts;
/* every criterion off; approach_dir (0, 0, 1), min_approach_cos -1; widths 0 .. 0.1; 4 probes, margin 0.01, max_unobserved 0 */
void agh_default_hand_filter_params(agh_hand_filter_params* p);
int agh_set_hand_filter(agh_ctx* ctx, const agh_hand_filter_params* fp);
int agh_get_hand_filter(agh_ctx* ctx, agh_hand_filter_params* out);
int agh_get_hand_filter_counts(agh_ctx* ctx, agh_hand_filter_counts* out, int32_t cap_lists);

/* HAND CLEARANCE: the sweep proves a hand collision-free against the points of the 8 cm ball around its sample, cropped to
 * +- hand_height, and against the two finger columns and the half-space behind the hand's back only (FingerHand::evaluateFingers).
 * The gripper's body (flange, camera mount, wrist) and the volume it sweeps on its way in along `approach` are never tested: a hand
 * lying almost flat on the table, or one reached under a shelf board, comes back collision-free.  agh_set_hand_clearance makes
 * every agh_localize* chain drop, between the search and the classifier and behind the hand filter (k_hand_clearance, the same drop
 * byte per hypothesis), the hands whose CORRIDOR -- an oriented box behind the palm, swept backwards along the approach -- holds
 * more than max_points points of the capture's own voxelised cloud.  All arithmetic is float64, left to right, never contracted.
 *  1. PALM POINT.  agh_hypothesis::bottom is NOT the palm: it is the deepest point of the object between the fingers.  The palm
 *     is derived as the hand filter derives its probes: s = the float32 point of the voxelised cloud at samples[H.sample],
 *     widened; h = ((b0 - s0) n0 + (b1 - s1) n1) + (b2 - s2) n2, b = bottom, n = binormal; y0 = depths[clamp(depth_index)] -
 *     hand_depth, the sweep's own bite table (init_bite, then += 0.005 depth_index times);
 *       o = (s + h x binormal) + y0 x approach                       (per coordinate)
 *  2. POINT IN CORRIDOR.  For a point p of the cloud (float32 widened), e = p - o, yb = (e0 a0 + e1 a1) + e2 a2 with
 *     a = approach, xb the same with the binormal, zb with the axis.  p is IN the corridor iff
 *       -far_offset <= yb && yb <= -near_offset && fabs(xb) <= half_width && fabs(zb) <= half_height
 *     All four comparisons are closed.  A NaN anywhere compares false: the point is not counted, so a record with a NaN field is
 *     kept, as the other filters keep it.
 *  3. POINTS TESTED: all voxels of the capture the hypothesis's list belongs to, both cameras.  A batch capture sees only its own
 *     cloud; a labelled or clustered list sees the whole cloud of its capture.  The voxel filter (agh_set_voxel_filter), if set,
 *     has already pruned: the clearance test sees what the sweep saw.
 *  4. DECISION.  A hand is dropped iff its count exceeds max_points.  The decision equals a brute-force count over all points: the
 *     count is an integer and depends on no traversal order, no atomic order and no early exit.
 *  5. ORDER.  The hand filter's three criteria come first: a hand they drop is not tested and does not count here.
 *     filters_boundaries stays independent: a hand goes if either says so.
 *  6. agh_get_hand_filter_counts keeps its meaning exactly: it returns 0 when only a clearance is set, and with both set its
 *     n_kept is still "before the classifier, the boundary filter and the clearance".
 *  7. SCOPE.  As agh_set_hand_filter: sticky per context until cleared (cp == NULL) or replaced; setting it does no device work;
 *     an invalid field returns AGH_ERR_INVALID_ARGUMENT, the text names it, and the setting held before stays.  It applies to
 *     every agh_localize* chain form -- points and depth, single, batch and _begin / _stage / _end, masked, labelled, clustered
 *     and fitted -- and to every in-call repeat that re-queues the search; it needs no depth images, so no form is refused.  The
 *     stage-wise and sharded calls (agh_find_hands*, agh_classify*) are not touched.  Only surviving hands reach the classifier,
 *     the 8192-hand limit, hands_out and the handle search; n_hypotheses stays the search's unfiltered count.  With nothing set
 *     nothing new is launched or allocated.
 *  8. MID-CHAIN (single or batch) agh_set_hand_clearance and agh_get_hand_clearance_counts return AGH_ERR_STATE;
 *     agh_get_hand_clearance (1 and a copy, or 0 if none is set) is host-side and allowed mid-chain.  The counts arrive in pinned
 *     memory with the chain's one synchronisation: one record per list of the last chain collected, in the order of its results,
 *     if it ran with a clearance; returns the number of lists, 0 if it ran without (or none ran), AGH_ERR_CAPACITY if cap_lists is
 *     smaller.
 *  The bounds far_offset <= 0.5 and half_width, half_height <= 0.25 are stated limits, not measured ones: they bound the grid cells
 *  one hand may walk (the corridor's bounding box is at most 1 m across).  tests/hand_clearance_cases.py is the numpy model the
 *  kernel matches decision for decision. */
typedef struct agh_hand_clearance_params
{
  double near_offset;   /* metres behind the palm where the corridor begins, finite, >= 0 */
  double far_offset;    /* ... and ends: near_offset < far_offset <= 0.5 */
  double half_width;    /* along the binormal, 0 < . <= 0.25 */
  double half_height;   /* along the axis, 0 < . <= 0.25 */
  int32_t max_points;   /* >= 0: a hand is dropped iff MORE points than this lie in its corridor */
  int32_t reserved;     /* 0 */
} agh_hand_clearance_params;
typedef struct agh_hand_clearance_counts
{
  int64_t n_tested;     /* the list's hypotheses that the hand filter (if set) kept */
  int64_t n_dropped;
  int64_t n_kept;       /* n_tested - n_dropped */
} agh_hand_clearance_counts;
/* near_offset 0, far_offset 0.12, half_width 0.05, half_height 0.04, max_points 0 */
void agh_default_hand_clearance_params(agh_hand_clearance_params* p);
int agh_set_hand_clearance(agh_ctx* ctx, const agh_hand_clearance_params* cp);
int agh_get_hand_clearance(agh_ctx* ctx, agh_hand_clearance_params* out);
int agh_get_hand_clearance_counts(agh_ctx* ctx, agh_hand_clearance_counts* out, int32_t cap_lists);

/* HANDLE RANKING: the chains end with the handle list in discovery order, the handle search's seed order (handle_search.cpp:79),
 * and the classifier's decision value never leaves the device.  A cell executes one grasp per pick, so every caller sorted the
 * handles itself, without the best criterion to sort by.  agh_set_handle_ranking makes every agh_localize* chain return each
 * list's handles_out span in RANK ORDER (k_handle_rank, queued behind k_handle_build; the chain's one synchronisation stays one).
 * The reference publishes its handles unranked: this is a capability on top of it, and with nothing set every result, launch and
 * allocation is what it was.  All arithmetic is float64, evaluated left to right, never contracted (-ffp-contract=off).
 *  1. INPUTS.  A handle of a list has inliers in[0..n) into the list's hands (hands_out).  g_k is the MARGIN of hand in[k]: minus
 *     the decision sum the classifier kernels store (k_hog_svm stores sum = -rho + res and keeps a hand iff sum <= 0; the
 *     general-model path uses the same convention), so kept hands have g >= 0.  With classify == 0, g = 0.0.
 *  2. THE WAVE SUM W(v, n), the only sum whose order matters: p[l] = ((v[l] + v[l+64]) + v[l+128]) + ... for l < 64, starting
 *     from +0.0, absent entries add nothing; then p[l] = p[l] + p[l ^ o] for o = 32, 16, 8, 4, 2, 1 (as k_handle_build sums its
 *     axis moments); the result is p[0].
 *  3. THE SEVEN TERMS, in terms[] order, with c = handle.center, a = handle.approach:
 *       t_support = (double) min(n, support_cap) / (double) support_cap
 *       t_margin = W(g, n) / (double) n
 *       t_approach = (a0 d0 + a1 d1) + a2 d2, d = approach_dir
 *       t_position = (c0 p0 + c1 p1) + c2 p2, p = position_dir
 *       t_distance = sqrt((e0 e0 + e1 e1) + e2 e2), e = c - ref_point
 *       t_width = fabs(handle.width - preferred_width)
 *       t_length = max_k(x_k) - min_k(x_k), x_k = (axis0 b0 + axis1 b1) + axis2 b2 over the inliers' bottom b, by fmax / fmin
 *         from -inf / +inf (order cannot matter)
 *  4. THE SCORE.  score = (((((w_support t1 + w_margin t2) + w_approach t3) + w_position t4) + w_distance t5) + w_width t6) +
 *     w_length t7.  Every term is always computed: a NaN term makes the score NaN even under weight 0.
 *  5. best_inlier: the first k in inlier order with the largest g_k; a NaN g never wins; 0 if none wins.
 *  6. ORDER.  With min_score = -inf no handle is left out.  Else a handle is left out iff !(score >= min_score) -- a NaN score is
 *     therefore left out whenever min_score is finite -- and counted in n_below.  The rest are ordered by score descending, NaN scores after every number, ties (decided by ==, so
 *     +0 and -0 tie) by ascending index, the handle's position in the unranked list.  The first max_handles are returned
 *     (0: all).  The order is total: it depends on no sort algorithm and on the order of no atomic.
 *  7. OUTPUTS.  results[l].r.n_handles is the number returned, and AGH_ERR_CAPACITY for handle_cap is judged on it.
 *     inlier_idx_out, n_inlier_idx, hands_out and every first_inlier are exactly the unranked call's: only the handle records
 *     move, so no index needs rewriting.  n_hypotheses and n_hands keep their meaning.
 *  8. SCOPE.  Sticky per context until cleared (rp == NULL) or replaced; the setter does no device work; an invalid field -- a
 *     non-finite one other than min_score = -inf, approach_dir off unit length by more than 1e-6, support_cap < 1, max_handles
 *     < 0 -- returns AGH_ERR_INVALID_ARGUMENT, the text names it, and the setting held before stays.  It applies to every
 *     agh_localize* chain form -- points and depth, single, batch and _begin / _stage / _end, masked, labelled, clustered and
 *     fitted -- and to every in-call repeat.  A chain call with w_margin != 0 and classify == 0 returns AGH_ERR_INVALID_ARGUMENT
 *     and launches nothing.  Set-then-clear is the same as never set.
 *  9. MID-CHAIN (single or batch) agh_set_handle_ranking and agh_rank_handles return AGH_ERR_STATE; agh_get_handle_ranking (1 and
 *     a copy, or 0 if none is set) is host-side and allowed mid-chain.  agh_get_handle_scores, agh_get_handle_ranking_counts and
 *     agh_get_hand_margins return AGH_ERR_STATE while a chain is in flight and when the last chain collected ran without a
 *     ranking; else the number of records written (scores: laid out as handles_out, all lists; margins: per hand, laid out as
 *     hands_out; counts: one per list), AGH_ERR_CAPACITY if the room is smaller.  They arrive in pinned memory with the chain's
 *     one synchronisation.
 * 10. STAGE-WISE.  agh_rank_handles takes host buffers and runs the same kernel on one list: the same order on agh_find_handles'
 *     output (margins NULL: zeros).  Refused on the host: rp NULL or an invalid record (AGH_ERR_INVALID_ARGUMENT); n_hands or
 *     n_handles above 8192 (AGH_ERR_CAPACITY); an n_inliers < 1, a span outside n_idx, an index outside n_hands
 *     (AGH_ERR_INVALID_ARGUMENT).  counts is filled before AGH_ERR_CAPACITY for cap.
 *  Not built: ranking in the sharded calls; a per-capture ranking record in a batch; terms that need the cloud, such as clearance
 *  counts or unobserved probes; reordering of inlier_idx_out.  tests/handle_ranking_cases.py is the numpy model the kernel
 *  matches bit for bit. */
typedef struct agh_handle_ranking_params
{
  double w_support, w_margin, w_approach, w_position, w_distance, w_width, w_length;
  double approach_dir[3];   /* unit within 1e-6 */
  double position_dir[3];   /* any finite vector; (0,0,1) = highest first */
  double ref_point[3];
  double preferred_width;
  double min_score;         /* -inf: none */
  int32_t support_cap;      /* >= 1 */
  int32_t max_handles;      /* 0: all; else top-k per list */
} agh_handle_ranking_params;
typedef struct agh_handle_score
{
  double score;
  double terms[7];
  int32_t index;            /* position in the unranked list */
  int32_t best_inlier;
} agh_handle_score;         /* 72 bytes, frozen */
typedef struct agh_handle_ranking_counts
{
  int64_t n_found;          /* the handles of the unranked list */
  int64_t n_below;          /* left out by min_score */
  int64_t n_returned;
} agh_handle_ranking_counts;
/* w_support 1, w_margin 1, other weights 0; approach_dir (0,0,-1); position_dir (0,0,1); ref_point 0; preferred_width 0;
 * min_score -inf; support_cap 10; max_handles 0 */
void agh_default_handle_ranking_params(agh_handle_ranking_params* p);
int agh_set_handle_ranking(agh_ctx* ctx, const agh_handle_ranking_params* rp);
int agh_get_handle_ranking(agh_ctx* ctx, agh_handle_ranking_params* out);
int agh_get_handle_scores(agh_ctx* ctx, agh_handle_score* out, int64_t cap);
int agh_get_handle_ranking_counts(agh_ctx* ctx, agh_handle_ranking_counts* out, int32_t cap_lists);
int agh_get_hand_margins(agh_ctx* ctx, double* out, int64_t cap);
int agh_rank_handles(agh_ctx* ctx, const agh_handle_ranking_params* rp, const agh_hypothesis* hands, int64_t n_hands,
  const double* margins, const agh_handle* handles, int64_t n_handles, const int32_t* inlier_idx, int64_t n_idx,
  agh_handle* handles_out, agh_handle_score* scores_out, int64_t cap, agh_handle_ranking_counts* counts);

/* The batch chains with every capture's samples drawn UNDER ITS OWN MASK: a cell with several sensor pairs and one detector per
 * sensor hands over, per rig, a capture and an object mask, and wants handles on the masked object of every rig from one call.
 * agh_localize_masked once per capture pays the single chain per capture, one after the other; an explicit sample_idx cannot
 * stand in for a mask, because it indexes the voxelised cloud, which only exists inside the call.
 * Points forms: masks is a host array of n_captures pointers; masks[k] holds one byte per raw point of capture k, packed, any
 * non-zero byte means "eligible".  Depth forms: masks is ONE flat array parallel to `images`: masks[i] belongs to images[i], has
 * its width and height, row v at data + v * row_stride_bytes (>= width); data == NULL: no pixel of that image is eligible.
 *  1. Rules 1 to 3 of agh_localize_masked hold per capture: E_k is the ascending list of capture k's eligible CAPTURE-LOCAL voxel
 *     indices, M_k = |E_k|, and sample t of capture k is E_k[stratum draw of agh_localize with M_k in the place of N,
 *     lp[k].n_samples and lp[k].sample_seed]; with M_k < lp[k].n_samples the list is E_k followed by INT32_MIN slots.  M_k = 0
 *     is no error: that capture has zero hypotheses, hands and handles, and the other captures are not affected.
 *  2. Equality per capture with the masked call: capture k's span of every output and results[k].r equal, bit for bit (epoch
 *     aside), what agh_localize_masked returns for capture k alone with masks[k] and lp[k], and M_k equals that call's
 *     agh_get_sample_mask_count.  The depth form's twin is agh_localize_depth_masked on capture k's images and masks.
 *  3. Equality with the unmasked batch: the results equal agh_localize_batch (agh_localize_depth_batch) on the same captures
 *     with each lp[k].sample_idx set to capture k's reported list; with all-ones masks the call equals the unmasked batch with
 *     sample_idx = NULL and the same seeds.
 *  4. Every capture of a masked batch has a mask.  AGH_ERR_INVALID_ARGUMENT, nothing launched, the text naming the capture (and
 *     the image, for a stride): masks == NULL; a NULL masks[k] (points); a depth capture whose mask records ALL have
 *     data == NULL; an lp[k].sample_idx != NULL; a mask row stride below the width.  Every validation, status and text of the
 *     unmasked batch twin holds as well: the fields that must be equal across the batch, n_captures in 1..64, 2^30 points,
 *     AGH_ERR_NO_SVM, the row count of a camera-origin table, the per-image rules.
 *  5. The output layout of agh_localize_batch* holds unchanged: samples_out holds capture-local indices, the per-capture spans
 *     and results[k], the per-capture 8192-hand limit, AGH_ERR_CAPACITY with every results[k] filled, one synchronisation in the
 *     steady state, and the first batch of a context takes the synchronisation for the lattice sizes.  The repeats inside the
 *     call -- the batch once more when the lattices outgrew the kept slots, the capacity classes -- read the masks where the
 *     first pass left them and search the lists already drawn.
 *  6. The mask stage runs for n_samples = 0 too.  agh_get_batch_mask_counts writes the M_k (n_captures entries) of the last
 *     batch chain this context collected, if that chain was masked; AGH_ERR_CAPACITY if cap_captures is below its n_captures;
 *     AGH_ERR_STATE if no chain was collected, if the last one was not a masked batch, or while a chain is in flight.  After a
 *     masked batch agh_get_sample_mask_count and agh_get_label_counts return AGH_ERR_STATE.
 *  7. A call while a chain of any kind is in flight returns AGH_ERR_STATE with the chain untouched.  The _begin forms queue the
 *     chain as agh_localize_batch_begin does and are collected with agh_localize_batch_end (the blocking forms are begin + end);
 *     between the two the rules of agh_localize_batch_begin hold.  A masked begin of host data never adopts a staged set: it
 *     drops a pending one, and the chain waits for its copies.
 *  8. Lifetimes: host masks are copied by begin into a buffer of the context, depth masks repacked to one byte per pixel in
 *     point order (a pageable mask has been read when begin returns; a pinned one follows the captures' lifetime rules, as
 *     the captures' own copies do).  Device points masks (_device: xyz[k] and masks[k] are device pointers) are read in place,
 *     at any byte alignment, and follow the captures' lifetime rules.  Device depth masks are repacked into the same buffer by
 *     device-to-device copies queued at begin; they must stay valid until the call (or agh_localize_batch_end) has returned.
 *  9. A context's first masked batch adds: one more set of bitmap slots of the batch's bitmap size, one byte and one 32-bit
 *     word per raw point, and the slots' block counts -- nothing else that scales with n_captures x the largest lattice.
 * Not built: a _stage call for masks; masks and label images in the batch chains mixed in one call (label images in the batch
 * chains alone: agh_localize_batch_labeled* below); masked and unmasked captures mixed in one batch (an
 * all-ones mask says "unmasked"); sharded variants. */
int agh_localize_batch_masked(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_batch_masked_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_batch_masked_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_batch_masked_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_masked(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_depth_batch_masked_device(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks,
  const int32_t* n_images, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_depth_batch_masked_begin(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks,
  const int32_t* n_images, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_masked_begin_device(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks,
  const int32_t* n_images, const agh_localize_params* lp, int32_t n_captures);
int agh_get_batch_mask_counts(agh_ctx* ctx, int64_t* n_eligible, int32_t cap_captures);

/* The batch chains with one sample list PER OBJECT of every capture's LABEL IMAGE: "grasps on each object, for every rig of the
 * cell" -- several sensor pairs, each with an instance segmenter.  agh_localize_labeled once per capture pays the single chain
 * and one synchronisation per capture, one after the other.  Here the batch is preprocessed once (agh_localize_batch*), one
 * label stage runs for all captures (capture on blockIdx.y, no launch per capture or per list), the search runs once over all
 * lists, and the batch tail compacts and walks one list per (capture, object) side by side; one synchronisation.
 * Points forms: labels is a host array of n_captures pointers.  Depth forms: labels is ONE flat array parallel to `images`, as
 * masks is in the masked batch.
 *  1. Lists.  n_objects[k] is the number of objects of capture k; list l = first_list[k] + j is object j of capture k, first_list
 *     being the exclusive prefix sum of n_objects; L = sum of n_objects[k] is the number of lists of the call.
 *     1 <= n_objects[k] <= 64 and L <= 64 (the lists the batch tail holds; this is not lifted here).  lp[k].n_samples = S_k is
 *     the number of samples of EACH object of capture k and lp[k].sample_seed the seed of every object of capture k;
 *     sum of n_objects[k] x S_k <= 2^24.  Any violation, or lp[k].sample_idx != NULL, is AGH_ERR_INVALID_ARGUMENT with nothing
 *     launched; the error text names the capture.
 *  2. Labels.  Points forms: labels[k] holds one byte per raw point of capture k; all n_captures entries are required, a NULL
 *     entry is an error that names the capture.  Depth forms: labels[i] belongs to images[i], has its width and height, row v
 *     at data + v * row_stride_bytes; data == NULL: no pixel of that image belongs to an object; a capture whose label records
 *     ALL have data == NULL is an error, and so is a row stride below the image width (the text names the capture and the
 *     image).  Byte 0: no object; byte j + 1: object j of THIS capture; a byte above n_objects[k]: no object, and no error.
 *  3. Eligibility and draw are rules 3 and 4 of agh_localize_labeled, per capture: E_{k,j} is the ascending list of the
 *     CAPTURE-LOCAL voxel indices that hold a kept raw point of capture k with label j + 1, in its own camera block;
 *     M_{k,j} = |E_{k,j}|; sample t of list (k, j) is E_{k,j}[stratum draw of agh_localize with M_{k,j}, S_k, seed_k]; with
 *     M_{k,j} < S_k the list is E_{k,j} followed by INT32_MIN slots.  M_{k,j} = 0 is no error: that list has no hypotheses,
 *     hands or handles, and no other list is affected.  The label stage runs for S_k = 0 too.
 *  4. Outputs: the layout of agh_localize_batch with L spans in list order.  results has L records; results[l].r holds list l's
 *     counts, its n_voxels is capture k's voxel count; first_* are the starts of list l's spans.  samples_out holds capture-local
 *     voxel indices, sum of n_objects[k] x S_k entries.  agh_hypothesis::sample is the position in the list's own sample list;
 *     inlier indices point into the list's own span of hands_out.  The 8192-hand limit holds per list (the error text says
 *     "capture k, object j").  Buffers that are too small: AGH_ERR_CAPACITY with every results[l] filled.
 *  5. Equality, with AGH_NORMALS_DETERMINISTIC: the spans of lists first_list[k] .. first_list[k] + n_objects[k] - 1 equal, bit
 *     for bit (epoch aside), what agh_localize_labeled returns for capture k alone with labels[k], n_objects[k] and lp[k] (the
 *     depth form's twin is agh_localize_depth_labeled); list (k, j) therefore equals agh_localize_masked on capture k with the
 *     mask labels[k] == j + 1, and M_{k,j} equals the twin's agh_get_label_counts.  With AGH_NORMALS_RAND50 the rand() stream
 *     runs through the whole sample list of the call: only list 0 equals its twin.
 *  6. Everything else is the unmasked batch twin's: classify, cell_size, min_inliers, min_length and filters_boundaries must be
 *     equal across the batch; n_captures in 1..64, fewer than 2^30 points; AGH_ERR_NO_SVM; a camera-origin table needs
 *     n_captures rows -- origins are per CAPTURE, not per list (the search derives a sample's cloud from its index in the
 *     common voxel array); the boundary filter uses the list's capture's workspace; one synchronisation in the steady state,
 *     the first batch of a context takes the one for the lattice sizes; an outgrown-slot repeat reads the labels where the
 *     first pass left them, capacity-class and declined-walk repeats work on the lists already drawn; AGH_ERR_STATE while a
 *     chain of any kind is in flight, that chain untouched; a begin of host data never adopts a staged set and drops a pending
 *     one; after the call the voxelised batch is the context's bound batch of n_captures clouds.  The _begin forms are collected
 *     with agh_localize_batch_end; the blocking forms are begin + end.
 *  7. agh_get_batch_label_counts writes the L values M_{k,j} of the last chain collected, in list order.  AGH_ERR_STATE if that
 *     chain was not a labelled batch, if there was none, or while a chain is in flight; AGH_ERR_CAPACITY if cap_lists < L.
 *     After a labelled batch agh_get_sample_mask_count, agh_get_label_counts and agh_get_batch_mask_counts return
 *     AGH_ERR_STATE; agh_get_batch_label_counts returns AGH_ERR_STATE after any other chain.
 *  8. Lifetimes and alignment are the masked batch's: host labels are copied by begin, depth labels repacked to one byte per
 *     pixel in point order; device points labels (_device) are read in place at any byte alignment; device depth labels are
 *     repacked by device-to-device copies queued at begin.
 *  9. A context's first labelled batch adds: one 32-bit word per word of the batch's bitmap slots, one 64-bit object set and
 *     one list entry per raw point of the batch, and L x ceil(n_max / 256) ints of group counts -- nothing that scales with L
 *     x a lattice, or with n_captures x 64.
 * 10. Not built: more than 64 lists per call; labels wider than a byte; a _stage call for labels; labelled, masked and unmasked
 *     captures mixed in one batch; sharded variants. */
int agh_localize_batch_labeled(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_batch_labeled_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_batch_labeled_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_batch_labeled_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_labeled(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out,
  int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_depth_batch_labeled_device(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out,
  int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_depth_batch_labeled_begin(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_labeled_begin_device(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures);
int agh_get_batch_label_counts(agh_ctx* ctx, int64_t* n_eligible, int32_t cap_lists);

/* The batch chains with one sample list per CONNECTED COMPONENT of every capture's own cloud: "grasps on each object, for every
 * rig of the cell", WITHOUT A SEGMENTER on any rig.  agh_localize_clustered once per capture pays the single chain and one
 * synchronisation per capture, one after the other, and a cluster stage that cannot fill the device from one capture.  Here the
 * batch is preprocessed once (agh_localize_batch*), ONE cluster stage runs for all captures (capture on blockIdx.y; the selection
 * one work-group per capture; no launch per capture or per list), and from the object sets on the call IS
 * agh_localize_batch_labeled: one compaction, one search over all lists, one batch tail, one synchronisation.
 * cp is an array of n_captures records, cp[k] capture k's own: rigs have their own planes.
 *  1. Lists.  K_k = cp[k].max_objects; list l = first_list[k] + j is object j of capture k, first_list being the exclusive prefix
 *     sum of the K_k; L = sum of K_k is the number of lists of the call, L <= 64 (the lists the batch tail holds; this is not
 *     lifted here).  lp[k].n_samples = S_k is the number of samples of EACH object of capture k and lp[k].sample_seed the seed of
 *     every object of capture k; sum of K_k x S_k <= 2^24.
 *  2. Objects per capture.  Rules 1 to 5 of agh_localize_clustered hold on capture k's own voxelised cloud with cp[k]: height,
 *     float32 adjacency, components, selection by size then smaller id, E_{k,j} ascending.  Voxel indices, ids and samples_out
 *     are CAPTURE-LOCAL.  No pair is ever formed across captures, whatever their coordinates: capture k's voxels are united only
 *     through capture k's own search grid, whose reach comes from its own grid descriptor and cp[k].tolerance.
 *  3. Equality, with AGH_NORMALS_DETERMINISTIC: the spans of lists first_list[k] .. first_list[k] + K_k - 1 and their
 *     results[l].r equal, bit for bit (epoch aside), what agh_localize_clustered returns on capture k alone with cp[k] and lp[k]
 *     (the depth form's twin is agh_localize_depth_clustered); capture k's counts, M_l, ids and label bytes equal the twin's
 *     agh_get_cluster_info / agh_get_cluster_labels; the whole call equals agh_localize_batch_labeled fed the label bytes the
 *     clusters imply.  With AGH_NORMALS_RAND50 the rand() stream runs through the whole sample list of the call: only list 0
 *     equals its twin.  No result depends on the order of an atomic operation.
 *  4. AGH_ERR_INVALID_ARGUMENT, nothing launched, the text naming the capture and the field: cp == NULL; any violation of rule 7
 *     of agh_localize_clustered by cp[k] (a non-finite field, the unit vector, the heights, tolerance, min_voxels, max_objects);
 *     L > 64; sum of K_k x S_k > 2^24; lp[k].sample_idx != NULL; and every validation of the unclustered batch twin: classify,
 *     cell_size, min_inliers, min_length and filters_boundaries equal across the batch, n_captures in 1..64, fewer than 2^30
 *     points, AGH_ERR_NO_SVM, a camera-origin table of n_captures rows -- origins are per CAPTURE, not per list -- and the
 *     per-image rules of the depth forms.
 *  5. Everything else is the labelled batch's: the output layout with L spans, results has L records; the 8192-hand limit per
 *     list (the error text says "capture k, object j"); AGH_ERR_CAPACITY with every results[l] filled; one synchronisation in
 *     the steady state, the first batch of a context takes the one for the lattice sizes; an outgrown-slot repeat re-enters
 *     with the cp records the chain holds (they are copied by begin), capacity-class and declined-walk repeats work on the
 *     lists already drawn; the cluster stage runs for S_k = 0 too; AGH_ERR_STATE while a chain of any kind is in flight, that
 *     chain untouched; a begin of host data never adopts a staged set and drops a pending one; after the call the voxelised
 *     batch is the context's bound batch of n_captures clouds.  The _begin forms are collected with agh_localize_batch_end; the
 *     blocking forms are begin + end.  The _device forms read device points (images) in place.
 *  6. agh_get_batch_cluster_info writes, for the last chain collected if it was a clustered batch, info[k] in capture order
 *     (cap_captures >= n_captures) and the M_l and capture-local ids in list order (cap_lists >= L; 0 and -1 for a list without
 *     an object); any of the three arrays may be NULL; AGH_ERR_CAPACITY if a cap is too small.  agh_get_batch_cluster_labels
 *     writes 0 or j + 1 per voxel of the bound batch, in agh_get_cloud's order, and returns the voxel count (AGH_ERR_CAPACITY if
 *     cap is below it).  Both return AGH_ERR_STATE after any other chain, with none collected, or while a chain is in flight.
 *     After a clustered batch agh_get_sample_mask_count, agh_get_label_counts, agh_get_cluster_info, agh_get_cluster_labels,
 *     agh_get_batch_mask_counts and agh_get_batch_label_counts return AGH_ERR_STATE.
 *  7. A context's first clustered batch adds, beside the labelled batch's object sets, list entries and group counts: two
 *     32-bit words and a byte per raw point of the batch; four 64-bit counters per capture; one record of cp per capture on the
 *     device and pinned; a pinned table of 4 words per capture plus 2 per list (counters, records and table are allocated once
 *     for 64 captures and lists, 10 KiB in all, and shared with the single clustered chain).  Nothing scales with L x a
 *     lattice, or with n_captures x 64.
 *  8. Not built: a _stage call; more than 64 lists per call; clustered captures mixed with labelled, masked or unmasked ones in
 *     one batch; sharded forms.  (These calls take every cp[k].plane from the caller: a fitted plane per capture is
 *     agh_localize_batch_clustered_fit* below.) */
int agh_localize_batch_clustered(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_batch_clustered_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_batch_clustered_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_batch_clustered_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_clustered(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_depth_batch_clustered_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results);
int agh_localize_depth_batch_clustered_begin(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_clustered_begin_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_get_batch_cluster_info(agh_ctx* ctx, agh_cluster_info* info /* n_captures */, int64_t* n_voxels /* L: M_l */,
  int32_t* ids /* L: capture-local */, int32_t cap_captures, int32_t cap_lists);
int agh_get_batch_cluster_labels(agh_ctx* ctx, uint8_t* labels_out, int64_t cap);  /* per voxel of the bound batch: 0 or j + 1 */

/* The clustered batch chains WITH EVERY CAPTURE'S SUPPORT PLANE FITTED ON THE DEVICE: a cell with several rigs and no calibration
 * on any of them.  agh_localize_clustered_fit takes one capture per call and pays the single chain each time;
 * agh_localize_batch_clustered* wants every cp[k].plane from the caller.  Here ONE fit stage (four launches, the capture on
 * blockIdx.y, whatever n_captures and the candidate counts are) runs behind the batch's preprocessing and in front of its one
 * cluster stage, writes capture k's plane into record k of the device table the cluster kernels read, and from there on the call
 * IS agh_localize_batch_clustered: nothing returns to the host, the chain keeps its one synchronisation.  The signatures are the
 * clustered batch's with one more argument, fp, in front of cp: an array of n_captures records, fp[k] capture k's own -- rigs
 * have their own noise, thresholds and seeds, as they have their own cp[k].
 *  1. Rules per capture.  Rules 1 to 6 of agh_localize_clustered_fit hold per capture, on capture k's own voxelised cloud: N_k its
 *     voxel count, voxel indices capture-local, fp[k] its parameters.  Rule 6 uses camera 0's origin in force for capture k: row
 *     k of an n_captures-row agh_set_cloud_cam_origins table, else agh_params::cam_origin[0].  No voxel of another capture is
 *     ever drawn, scored or summed for capture k, whatever the coordinates.
 *  2. Equality per capture.  result[k] (agh_get_batch_plane_fit) and capture k's candidates (agh_get_batch_plane_fit_candidates)
 *     equal, bit for bit, what agh_localize_clustered_fit reports on capture k alone with fp[k], cp[k], lp[k] and that origin
 *     (the depth forms' twin is agh_localize_depth_clustered_fit); capture k's lists, results[l], cluster info and label bytes
 *     equal that twin's (epoch aside, AGH_NORMALS_DETERMINISTIC as for the clustered batch).
 *  3. Equality of the whole call.  The whole call equals agh_localize_batch_clustered with cp[k].plane set to the reported plane
 *     for every found capture.  A capture without a plane has K_k empty lists, no foreground and a reported plane of zeros (its
 *     device record carries a NaN plane), and the other captures are unaffected; the return value is AGH_OK.
 *  4. Repeatability.  The same call twice gives the same bits, on one context and on a fresh one: counts and sums are integers,
 *     nothing depends on the order of an atomic operation.
 *  5. Refusals.  AGH_ERR_INVALID_ARGUMENT, nothing launched, the text naming the capture and the field: fp == NULL; any violation
 *     of agh_localize_clustered_fit's rule 10 by fp[k] (reported as "capture k: ..."); and every refusal of the clustered batch
 *     (its rule 4).  cp[k].plane is ignored and not validated.
 *  6. Repeats inside the call.  The chain holds a copy of the fp records beside the cp records: an outgrown-slot repeat re-enters
 *     with both, and fits again on the lattice that holds the captures.
 *  7. State.  After a fitted batch agh_get_batch_cluster_info and agh_get_batch_cluster_labels work as after a clustered batch;
 *     agh_get_plane_fit and agh_get_plane_fit_candidates (the single call's) return AGH_ERR_STATE, as every getter does that
 *     returns it after a clustered batch.  agh_get_batch_plane_fit writes result[k] in capture order and returns n_captures
 *     (AGH_ERR_CAPACITY if cap_captures is below it): the records arrive in pinned memory with the chain's one synchronisation.
 *     agh_get_batch_plane_fit_candidates is agh_get_plane_fit_candidates for one capture of the batch: capture-local indices,
 *     planes BEFORE refit and orientation, counts; any array may be NULL; it returns C_k = fp[capture].n_candidates
 *     (AGH_ERR_CAPACITY if cap is below it, AGH_ERR_INVALID_ARGUMENT for a capture outside the batch).  Both return AGH_ERR_STATE
 *     after any other chain, with none collected, or while one is in flight.
 *  8. Memory.  A context's first fitted batch adds 64 blocks of 256 candidates, counts and sums (about 0.8 MB on the device), 64
 *     parameter records on the device and pinned, and 64 pinned result records.  Nothing is allocated per point.
 *  9. Not built: a _stage call; fitted captures mixed with captures whose plane is given, in one batch; more than 256 candidates;
 *     sharded forms. */
int agh_localize_batch_clustered_fit(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_batch_clustered_fit_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_batch_clustered_fit_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_batch_clustered_fit_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes,
  const int64_t* n, const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_clustered_fit(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_depth_batch_clustered_fit_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results);
int agh_localize_depth_batch_clustered_fit_begin(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_localize_depth_batch_clustered_fit_begin_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures);
int agh_get_batch_plane_fit(agh_ctx* ctx, agh_plane_fit_result* out /* n_captures */, int32_t cap_captures);
int agh_get_batch_plane_fit_candidates(agh_ctx* ctx, int32_t capture, int32_t* idx /* 3 per candidate, capture-local */,
  double* planes /* 4 per candidate */, int64_t* counts, int32_t cap);

/* The context's current cloud: packed xyz (3 floats per point) and camera ids; returns the number of points. */
int agh_get_cloud(agh_ctx* ctx, float* xyz_out, int32_t* cam_out, int64_t cap);

/* Table-plane removal of Localization::localizeHands(..., uses_clustering = true) (localization.cpp:51-98):
 * pcl::SACSegmentation with SACMODEL_PLANE / SAC_RANSAC, then pcl::ExtractIndices with setNegative(true).
 * agh_remove_plane works on the context's current single cloud (agh_set_cloud* or agh_preprocess*) and replaces it with
 * the points that are not inliers of the plane, in their order (the grid build stays queued, as after agh_set_cloud).
 * The restated algorithm (candidate draws, scoring, termination, refit) is in DESIGN.md, "Table-plane removal".
 * AGH_ERR_STATE without a cloud, with a batch of several clouds bound, or between agh_localize_begin and _end.
 * Fewer than 3 points or no sample that passes: found = 0 and the cloud is left as it was (not an error). */
typedef struct agh_plane_params
{
  int32_t max_iterations;       /* 100 (setMaxIterations); 0 .. 1023 */
  int32_t optimize;             /* 1 (setOptimizeCoefficients): least-squares refit of the plane, then reselection */
  double distance_threshold;    /* 0.01 (setDistanceThreshold) */
  double probability;           /* 0.99 (PCL's default) */
  uint32_t seed;                /* 12345 (PCL's fixed seed of boost::mt19937) */
  int32_t cam_ids_by_position;  /* 1: the kept point i keeps the camera id of point i of the unsegmented cloud -- the
                                   reference's behaviour (it builds cluster_cam_source but searches with pts_cam_source);
                                   0: every kept point keeps its own camera id */
} agh_plane_params;
typedef struct agh_plane_result
{
  float coefficients[4];  /* a, b, c, d of a x + b y + c z + d = 0 (refined if optimize and >= 4 inliers) */
  int64_t n_inliers;      /* points removed (PCL's inliers->indices.size()) */
  int64_t n_remaining;    /* points kept: the new cloud's size */
  int32_t iterations;     /* RANSAC iterations (candidates scored) */
  int32_t found;          /* 1 if a model was chosen */
} agh_plane_result;
void agh_default_plane_params(agh_plane_params* p);
int agh_remove_plane(agh_ctx* ctx, const agh_plane_params* pp, agh_plane_result* result);
/* The inliers of the last agh_remove_plane (PCL's inliers->indices, ascending positions in the cloud it ran on); returns
 * their number (AGH_ERR_CAPACITY if it exceeds cap; idx may be NULL to ask for the number). */
int agh_get_plane_inliers(agh_ctx* ctx, int32_t* idx, int64_t cap);
/* Introspection for parity tests: the candidate planes the last agh_remove_plane drew (planes: 4 floats each, samples: 3
 * indices each, counts: points within the threshold), in drawing order; returns their number.  Candidates beyond the
 * ones the termination rule let RANSAC score are drawn and scored all the same (they cannot change the earlier ones). */
int agh_get_plane_candidates(agh_ctx* ctx, float* planes, int32_t* samples, int64_t* counts, int64_t cap);
/* RandomSampleConsensus::computeModel's termination rule replayed over the inlier counts of candidates 0 .. n - 1 of N
 * points: *best = the candidate chosen (-1 if none), *iterations = candidates scored.  Host-only, needs no device. */
void agh_plane_replay(const int64_t* counts, int64_t n, int64_t n_points, int32_t max_iterations, double probability,
  int32_t* best, int32_t* iterations);

/* HandSearch::findHands for explicit sample indices.  out receives <= 8*n_samples records, sample-major and
 * orientation-ascending (the reference's concatenation order, hand_search.cpp:194-200).  The host variant stages the sample
 * list in pinned memory of the context, the concatenation kernel writes count, flags and records into pinned memory as well,
 * and the call waits for ONE stream synchronisation (no read-back copies). */
int agh_find_hands(agh_ctx* ctx, const int32_t* sample_idx, int64_t n_samples, int calculates_antipodal,
  agh_hypothesis* out, int64_t cap, int64_t* n_out);
/* Same, everything device-resident and asynchronous on hip_stream (NULL = the context's stream):
 * d_out has room for cap records, *d_n_out (device int64) receives the count.  Device-side errors (capacity, a sample
 * index outside the cloud, AGH_ERR_RETRY) are reported by the next agh_synchronize.  A list longer than cap is
 * AGH_ERR_CAPACITY there; *d_n_out then holds its full length and d_out its first cap records.  The host variant
 * returns AGH_ERR_CAPACITY at once, with *n_out = the full length (cap = 0 and out = NULL ask for it). */
int agh_find_hands_device(agh_ctx* ctx, const int32_t* d_sample_idx, int64_t n_samples, int calculates_antipodal,
  agh_hypothesis* d_out, int64_t cap, int64_t* d_n_out, void* hip_stream);

/* Linear SVM (one weight vector of 3528 floats + rho) from memory, or any supported model (see agh_load_svm_model)
 * from an OpenCV YAML file. */
int agh_load_svm(agh_ctx* ctx, const float* weights, int32_t n_weights, double rho);
int agh_load_svm_file(agh_ctx* ctx, const char* path);
/* Learning::classify on the hypotheses of the last agh_find_hands* call: keep[i] = 1 iff kept.  Also sets
 * svm_keep in the device-side records; keep may be NULL for the device variant. */
int agh_classify(agh_ctx* ctx, uint8_t* keep, int64_t cap, int64_t* n_kept);
int agh_classify_device(agh_ctx* ctx, uint8_t* d_keep, void* hip_stream);
/* Stamp (agh_hypothesis::epoch) and hypothesis count of the last completed agh_find_hands* call of this context
 * (*n_hyp = -1 while the count of an asynchronous agh_find_hands_device call is not known to the host). */
int agh_get_epoch(agh_ctx* ctx, int32_t* epoch, int64_t* n_hyp);
/* The 80x100 occupancy images (Learning::convertToImage, learning.cpp:320-365) of the hypotheses of the last
 * agh_find_hands* call, packed (250 words each, layout below): what a hypothesis must carry to be classified later, by
 * any context, without the device state of its search.  Returns the number of images written. */
int agh_get_packed_images(agh_ctx* ctx, uint32_t* images, int64_t cap_hyp);
/* Learning::classify on n such images, independent of any earlier call (the reference's classify is stateless and takes
 * any list, learning.cpp:165-247): keep[i] = 1 iff CvSVM::predict == 1; sums (optional) receives the decision values. */
int agh_classify_images(agh_ctx* ctx, const uint32_t* images, int64_t n, uint8_t* keep, double* sums);

/* ---- training side: Learning::train / trainBalanced / convertData, learning.cpp:3-163, 249-318
 * The reference keeps, in every GraspHypothesis, the points of its hand box and their split by camera
 * (rotating_hand.cpp:143-151) so that Learning::train can later rasterise three instances per hand: all points, camera
 * 0's and camera 1's (createInstance, learning.cpp:375-400; same source_to_center for the three).  Here the three
 * 80x100 occupancy images are produced by the hand sweep itself and stand for the instance.
 * Packed image: 250 uint32 words, bit (b & 31) of word (b >> 5) is pixel b = row * 100 + col (set = 255). */
/* on != 0: every following agh_find_hands*(calculates_antipodal = 1) also rasterises the per-camera images. */
int agh_set_training_images(agh_ctx* ctx, int on);
/* The three images (cam = -1, 0, 1) of each hypothesis of the last such call: cap_hyp x 3 x 250 words.  Returns the
 * number of hypotheses written. */
int agh_get_training_images(agh_ctx* ctx, uint32_t* images, int64_t cap_hyp);
/* cv::HOGDescriptor(winSize 64x64).compute(image, winStride 32x32) as convertData calls it (learning.cpp:253-281):
 * n packed images -> n x 3528 floats. */
int agh_hog_images(agh_ctx* ctx, const uint32_t* images, int64_t n, float* desc);
/* convertData's CvSVM::train (C_SVC) on the images' descriptors.  kernel_type AGH_SVM_LINEAR is convertData's
 * uses_linear_kernel = true (the shipped model's shape): CvSVM::optimize_linear_svm compacts the result to one vector,
 * returned as sv_out[0..3527] with alpha_out[0] = 1 and *n_sv_out = 1.  AGH_SVM_POLY2 is uses_linear_kernel = false,
 * the default Learning::train* pass (learning.h:180-182): kernel (x.y)^2; sv_out receives the *n_sv_out support vectors
 * (3528 floats each, room for sv_cap of them: AGH_ERR_CAPACITY with *n_sv_out set if there are more), alpha_out their
 * signed coefficients.  labels[k] > 0 marks a positive (label 1), anything else label -1.  The reference's CvSVMParams
 * defaults are C = 1, max_iter = 1000, eps = FLT_EPSILON.  info_out (optional, 6 ints): solver steps taken, support
 * vectors of the solve, instances of label -1, instances of label +1, kernel rows computed, kernel rows served by the
 * row cache.
 * OpenCV's solver is third-party code restated from its published algorithm: see DESIGN.md for what is pinned. */
#define AGH_SVM_LINEAR 0
#define AGH_SVM_POLY2 1
int agh_train_svm(agh_ctx* ctx, const uint32_t* images, const int8_t* labels, int64_t n, int32_t kernel_type, double C,
  int32_t max_iter, double eps, float* sv_out, int64_t sv_cap, double* alpha_out, int32_t* n_sv_out, double* rho_out,
  int32_t* info_out);
/* CvSVM::save (learning.cpp:312) of such a model in OpenCV's YAML layout (what agh_load_svm_file and CvSVM::load read). */
int agh_save_svm_file(const char* path, int32_t kernel_type, const float* sv, int32_t n_sv, int32_t n_weights,
  const double* alpha, double rho);
/* The same with the training parameters the file's header records (C, term_criteria); agh_save_svm_file writes
 * CvSVMParams' defaults (C = 1, 1000 iterations, FLT_EPSILON), which is what Learning::convertData trains with. */
int agh_save_svm_file_ex(const char* path, int32_t kernel_type, const float* sv, int32_t n_sv, int32_t n_weights,
  const double* alpha, double rho, double C, int32_t max_iter, double eps);
/* Load a model for agh_classify from memory: the compacted linear vector (same as agh_load_svm) or support vectors +
 * alphas with either kernel (CvSVM::predict: sum = -rho + sum_k alpha[k] K(sv_k, x), kept iff sum <= 0). */
int agh_load_svm_model(agh_ctx* ctx, int32_t kernel_type, const float* sv, int32_t n_sv, int32_t n_weights,
  const double* alpha, double rho);

/* ---- multi-GPU: the sample set of ONE cloud sharded over the GPUs of a node --------------------------
 * The reference's two OpenMP loops run over independent samples (hand_search.cpp:77-80, 135-138); here rank g of G takes
 * the contiguous slice [g*S/G, (g+1)*S/G) of the sample list, so the concatenation of the ranks' results in rank order IS
 * the reference's sample-major list.  One process per GPU, one context per process; every rank sets the SAME cloud
 * (agh_set_cloud*) and passes the SAME sample list.  The only data-path communication is RCCL all-gathers over xGMI,
 * issued from this library on the search's stream:
 *   - the ranks' compacted hypothesis lists (one all-gather; fixed-size segments, see agh_find_hands_sharded_device);
 *   - with calculates_antipodal: the all-points normals pass is sharded by point range and cloud_normals_ (3 x N doubles,
 *     hand_search.cpp:13-26) is all-gathered before the hand search, and so are the samples' own normals
 *     (hand_search.cpp:102); with AGH_NORMALS_RAND50: the ranks' rand() draw counts (one int each).
 * The merged list is byte-identical to the single-GPU list apart from the per-call stamp.
 *
 * agh_comm_unique_id: ncclGetUniqueId; call on ONE rank and hand the 128 bytes to the others out of band (MPI, a
 * torch.distributed broadcast, a file).  agh_comm_init: ncclCommInitRank on the context's device (collective: every rank
 * calls it).  agh_comm_init_local: n contexts of THIS process (one host thread each; they may share a device) exchange
 * through device copies instead of RCCL -- RCCL refuses two ranks on one GPU, and this is how the sharded schedule is
 * validated on a single-GPU machine.  A context belongs to at most one communicator. */
#define AGH_COMM_ID_BYTES 128
int agh_comm_unique_id(uint8_t id[AGH_COMM_ID_BYTES]);
int agh_comm_init(agh_ctx* ctx, int32_t rank, int32_t n_ranks, const uint8_t id[AGH_COMM_ID_BYTES]);
int agh_comm_init_local(agh_ctx* const* ctxs, int32_t n_ranks);
int agh_comm_destroy(agh_ctx* ctx);
int agh_comm_rank(const agh_ctx* ctx, int32_t* rank, int32_t* n_ranks); /* 0 / 1 without a communicator */
/* Which RCCL image the library bound ("already mapped: <path>" -- the copy the process had loaded, e.g. PyTorch's --, or
 * "loaded: <name>"), or an error text if none was found.  Calling it BINDS RCCL if that has not happened yet (the same one-time
 * dlopen agh_comm_unique_id / agh_comm_init perform).  RCCL is bound at run time: building the library needs neither its headers
 * nor the library itself. */
const char* agh_comm_rccl_origin(void);
/* Length of the merged list of the last agh_find_hands_sharded (host variant) of this context; AGH_ERR_STATE if the context
 * has no communicator or has not run a sharded search. */
int agh_comm_last_count(const agh_ctx* ctx, int64_t* n_hyp);
/* What the hypothesis all-gather of the last agh_find_hands_sharded* call of this context moved: *segment_bytes = bytes every
 * rank contributed (header + record slots), *n_ranks = ranks of the communicator it ran on (so n_ranks x segment_bytes land in
 * every rank's exchange buffer), *via_rccl = 1 for ncclAllGather, 0 for the in-process communicator's device copies.  Any of
 * the three may be NULL.  AGH_ERR_STATE without a communicator or before the first sharded search. */
int agh_comm_last_exchange(const agh_ctx* ctx, int64_t* segment_bytes, int32_t* n_ranks, int32_t* via_rccl);
/* Testing aid (tests/test_gpu_sharding.py): make this rank fail ON ITS OWN at the named sites of its next sharded call, as an
 * out-of-memory or a launch error would -- 1: per-call buffers (device variant), 2: the Taubin launch, 4: growth of the exchange
 * buffer, 8: the HOG / SVM launch of agh_classify_sharded*, 16: per-call buffers (host variant); one shot per bit.  What the tests
 * then check is the contract of the sharded calls: such a rank still takes part in every collective (an empty segment whose header
 * says so), every rank returns an error for the call (the failing rank its own, the others AGH_ERR_STATE, or AGH_ERR_HIP together
 * when an exchange buffer could not grow), and the communicator stays usable. */
int agh_comm_inject_fault(agh_ctx* ctx, int32_t sites);

/* Tuning: record slots of one rank's exchange segment (0 = the default described at agh_find_hands_sharded_device; values
 * above 8 per sample are clipped).  Every rank must use the same value. */
int agh_comm_set_segment_records(agh_ctx* ctx, int64_t records);
/* The slice of an n-item list that rank `rank` of `n_ranks` takes: [*lo, *hi). */
void agh_shard_slice(int64_t n, int32_t rank, int32_t n_ranks, int64_t* lo, int64_t* hi);
/* HandSearch::findHands with the samples sharded over the communicator's ranks (collective).  Arguments as for
 * agh_find_hands_device; on return (asynchronously on hip_stream) every rank's d_out holds the complete list and
 * *d_n_out its length.  Each rank contributes a segment of max(2 ceil(S/G), 1024) records (never more than 8 ceil(S/G)): scenes
 * yield well under one hypothesis per sample, and xGMI all-gathers of this size are latency bound.  If a rank found more,
 * the call reports AGH_ERR_RETRY at the next agh_synchronize and switches the context to full-size segments (8 per
 * sample) for the following calls; the host variant retries by itself. */
int agh_find_hands_sharded_device(agh_ctx* ctx, const int32_t* d_sample_idx, int64_t n_samples, int calculates_antipodal,
  agh_hypothesis* d_out, int64_t cap, int64_t* d_n_out, void* hip_stream);
int agh_find_hands_sharded(agh_ctx* ctx, const int32_t* sample_idx, int64_t n_samples, int calculates_antipodal,
  agh_hypothesis* out, int64_t cap, int64_t* n_out);
/* Learning::classify after a sharded search (collective): every rank classifies the hypotheses of its own samples (their
 * images are local), the labels travel with a second all-gather of the segments; d_out of the search is updated in
 * place (svm_keep), d_keep (optional, room for the search's cap) receives the flags in list order. */
int agh_classify_sharded_device(agh_ctx* ctx, uint8_t* d_keep, void* hip_stream);
int agh_classify_sharded(agh_ctx* ctx, agh_hypothesis* out, uint8_t* keep, int64_t cap, int64_t* n_kept);

/* Introspection for parity tests / plotting (host buffers). */
int agh_get_frames(agh_ctx* ctx, agh_frame* out, int64_t cap);
/* Neighbour counts of the samples of the last call: n_taubin = points in the Taubin ball (hand_search.cpp:85), n_hands =
 * points radiusSearch(sample, nn_radius_hands) returns (hand_search.cpp:147).  Either may be NULL.  n_hands is counted
 * on demand (one extra kernel per call of this getter; the cloud of the search must still be set): the hand sweep itself
 * only visits the slab of that ball the hand can occupy. */
int agh_get_neighbor_counts(agh_ctx* ctx, int32_t* n_taubin, int32_t* n_hands, int64_t cap);
int agh_get_images(agh_ctx* ctx, uint8_t* images, int64_t cap_hyp); /* cap_hyp x 8000 bytes, 80 rows x 100 cols */
/* agh_get_hog recomputes the descriptors and SVM sums of every hypothesis of the last search on demand (a chain with
 * filters_boundaries computed none for the hypotheses it filtered; this getter does, unfiltered, and relabels svm_keep of the
 * device-side records as agh_classify does). */
int agh_get_hog(agh_ctx* ctx, float* desc, double* sums, int64_t cap_hyp); /* cap_hyp x 3528 floats (+ SVM sums) */
int agh_get_normals(agh_ctx* ctx, double* normals, int64_t cap_points);  /* cloud_normals_ (3 doubles per point) */
/* GraspHypothesis::getPointsForLearning and the split of its columns by camera (grasp_hypothesis.h:149-170; filled at
 * rotating_hand.cpp:125-157), recomputed on demand for hypothesis `hyp` of the last agh_find_hands* call: `points`
 * receives the 3 x n_b matrix column by column (Eigen's Matrix3Xd layout) in the reference's column order, cam_source[k]
 * the camera id of column k (indices_cam1 = the k with 0, indices_cam2 = the k with 1).  *n_out = n_b in any case;
 * AGH_ERR_CAPACITY if n_b > cap.  A lazy getter (one pass over the cloud per call), not part of the hot path. */
int agh_get_learning_points(agh_ctx* ctx, int64_t hyp, double* points, int32_t* cam_source, int64_t cap, int64_t* n_out);
int agh_get_timing(agh_ctx* ctx, agh_timing* out);
/* Timed launches behind ms[i] of the LAST agh_get_timing call of this context (profile 3 times a sample of the calls):
 * counts[0 .. min(cap, AGH_TIMING_SLOTS) - 1]. */
int agh_get_timing_counts(agh_ctx* ctx, int32_t* counts, int32_t cap);
/* Grid-build counters of the context: stats[0] = builds, [1] = cold builds (bounding box first: the context's first build, one
 * after a failed build or a change of the number of clouds, or every build under AGH_GRID_COLD=1), [2] = builds of a cloud with points
 * outside the grid descriptor the build kept from the previous one (a miss: still exact, only slower).  Writes min(cap, 3)
 * values and returns how many; synchronises the context's device. */
int agh_get_grid_stats(agh_ctx* ctx, int64_t* stats, int32_t cap);
/* The grid descriptor the LAST build used for cloud `cloud` of the context's batch (0 for a single cloud): the origin mn, the
 * cell size, the cells per axis and the open faces (bit 2a = low face of axis a, 2a + 1 = its high face: the cloud had points
 * beyond it).  Read-only: a copy of the device's descriptor after a synchronisation of the context's device; any of the four
 * outputs may be NULL.  AGH_ERR_INVALID_ARGUMENT for a cloud outside [0, n_clouds), AGH_ERR_NO_CLOUD before the first build. */
int agh_get_grid_desc(agh_ctx* ctx, int32_t cloud, double mn[3], double* cell, int32_t dim[3], uint32_t* open);
/* Change agh_params::profile of a live context (0 .. 3); pending timings are dropped. */
int agh_set_profile(agh_ctx* ctx, int32_t level);
int agh_synchronize(agh_ctx* ctx);
/* Device self-test of the IEEE assumptions the parity contract rests on (fp64 div/sqrt, fp32 div/sqrt correctly
 * rounded, no FMA contraction): returns the number of mismatches against host arithmetic on n random inputs. */
int64_t agh_selftest_math(agh_ctx* ctx, int64_t n, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* AGH_H */
