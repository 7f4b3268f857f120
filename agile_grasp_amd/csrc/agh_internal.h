// agh_internal.h -- shared declarations of the HIP implementation (gfx950 only, no CPU path).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "agh.h"

namespace agh
{

constexpr int kBboxBlocks = 128;   // work-groups of k_bbox per cloud (one slot of six extrema each)
constexpr int kCountBlocks = 2048; // most work-groups of k_cell_count per cloud (one slot of six extrema each)
constexpr int kGridMargin = 2;     // cells of padding on every face of a kept grid descriptor (grid.hip, desc_next)
constexpr int kCellCap = 1 << 21;  // cells in the uniform grid table (8 MiB of int32)
constexpr int kCellStride = kCellCap + 4;  // entries of one cloud's cell table (kCellCap + 1 used; 16-byte aligned tables)
constexpr int kMaxRows = 128;      // (y,z) cell rows one ball query may touch
constexpr int kNumSums = 37;       // distinct sequential sums behind M and N (quadric.cpp:40-131)
constexpr int kSumStride = 40;     // doubles per sample in the sums buffer
constexpr int kSlots = 8;          // hypothesis slots per sample = hand orientations (rotating_hand.cpp:13)
constexpr int kImageWords = 250;   // 80x100 occupancy bitmap, one bit per pixel
constexpr int kBigListGrid = 512;  // work-groups of the 4096-class Taubin launches, which walk the list of the samples beyond 1152 neighbours
constexpr int kSweepWg4MinSamples = 4096;  // k_hand_sweep launches beyond this many samples run four work-groups per CU (hand_sweep.hip, WG4)
constexpr int64_t kNormalsChunk = 16384;  // points per batch of the all-points normals pass

// Uniform grid over the cloud's bounding box (stands in for the kd-tree of hand_search.cpp:10-11).
struct GridDesc
{
  double mn[3];
  double cell;
  double inv_cell;
  int dim[3];
  int ncell;
  unsigned open;     // faces whose border layer holds points outside the box: bit 2a = low face of axis a, 2a + 1 = high face
  unsigned ticket;   // tile tickets of k_cell_scan (reset by the holder of the last one)
};

// Everything a search kernel needs to walk the grid.
// A context holds a BATCH of n_clouds >= 1 clouds laid end to end in one point array (cloud k = points [cloud_off[k],
// cloud_off[k + 1])); point and sample indices are positions in that array.  Every cloud has its own grid descriptor and
// its own cell table (kCellStride entries each, holding positions in the common cell-sorted array), so a ball query only
// sees its own cloud.  n_clouds == 1 is the plain HandSearch::findHands case.
constexpr int kMaxClouds = 64;
struct GridView
{
  const GridDesc* desc;    // n_clouds descriptors (or, after grid_of_*, the one of the query's cloud)
  const int* cell_start;   // n_clouds x kCellStride
  const float4* sorted;    // x, y, z, bits((idx << 1) | cam), cloud-major, then cell-major
  const int* cloud_off;    // n_clouds + 1
  int n_clouds;
};

struct HandGeom
{
  double finger_width, hand_outer_diameter, hand_depth, hand_height, init_bite;
  double cam_origin[2][3];
  double cos_a[8], sin_a[8];   // host libm cos/sin of the 8 hand angles (rotating_hand.cpp:13-15, 89-90)
  double fs[20];               // finger_spacing_ (finger_hand.cpp:8-15)
  double thr[40];              // sorted unique thresholds {fs_i, fs_i + fw}
  int n_thr;
  int lo_idx[20], hi_idx[20];  // index of fs_i and of fs_i + fw in thr
  double depths[16];           // init_bite, then += 0.005 while <= hand_depth (finger_hand.cpp:204)
  double backs[16];            // -1.0 * (hand_depth - depth_k)
  double boxy[16];             // backs[k] + hand_depth (rotating_hand.cpp:127)
  int n_depths;
  double cos_antipodal;        // cos(20 deg) (antipodal.cpp:16)
  // Uniform-cell look-up tables over the two sorted tables above: lut[cell(v)] = number of table entries in EARLIER
  // cells; the entries of v's own cell (at most kLutProbe of them, checked on the host) are compared explicitly, so
  // rank(v) = #{entries < v} (or <= v) is exact for every v.
  double xlut_lo, xlut_scale;
  double ylut_lo, ylut_scale;
  unsigned char xlut[1024];
  unsigned char ylut[64];
  int x_probes, y_probes;      // most entries any one cell holds: the probes a kernel instantiation must make
};
constexpr int kLutProbe = 4;

struct HogTablesDev
{
  // Gradient LUT for binary images: index = (sx+1)*3 + (sy+1), sx/sy = sign of dx/dy
  float mag0[9], mag1[9];
  int bin0[9], bin1[9];
  // coef[code][bin] = mag0 for bin0, mag1 for bin1, 0 elsewhere: a pixel's vote is hist[bin] += coef[code][bin] * w for
  // all nine bins (adding the +0.0f products is exact), i.e. 9 mul + 9 add instead of 18 compares and 18 selects
  alignas(16) float coef[9][12];
  // pixData of HOGCache::init in its accumulation order (count1 | count2 | count4 groups): position of entry k inside
  // the 16x16 block and its weight gradWeight * histWeights for each of the four cells (0 where it does not vote)
  int pix_x[256], pix_y[256];
  float pix_wcell[256][4];
};

enum SampleStatus : int
{
  kStatusOk = 0,
  kStatusOverflow = 1,    // neighbourhood larger than the kernel's LDS capacity
  kStatusDegenerate = 2,  // no frame (an empty neighbourhood; rank-deficient pencils DO get one since round 3): no hypotheses
  kStatusRows = 3,
  kStatusBadIndex = 4,    // sample index outside the cloud (device-resident sample lists are validated on the device)
  kStatusSkipped = 5      // kSampleSkip: an unused slot of a device-drawn sample list
};
constexpr int32_t kSampleSkip = INT32_MIN;
#ifdef __HIPCC__
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x)
{
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// Sample k of a device-drawn list of S over N points (include/agh.h, agh_localize): one per stratum [k N / S, (k + 1) N / S),
// offset splitmix64(seed ^ k * 0x9E3779B97F4A7C15) % width; with N < S every point, then kSampleSkip.  agh_localize and
// agh_localize_batch draw with this one function.
__device__ __forceinline__ int32_t draw_stratum(long long N, int S, long long k, unsigned long long seed)
{
  if (N >= S)
  {
    const long long lo = (k * N) / S, hi = ((k + 1) * N) / S;
    return (int32_t) (lo + (long long) (splitmix64(seed ^ ((unsigned long long) k * 0x9E3779B97F4A7C15ull)) % (unsigned long long) (hi - lo)));
  }
  return k < N ? (int32_t) k : kSampleSkip;
}
#endif
constexpr int kBigCap = 4096;    // per-sample neighbour-list scratch (and the largest LDS-resident class of K1a) without ...
constexpr int kHugeCap = 6144;   // ... and with the 6144 class (Ctx::huge_classes)
constexpr int64_t kHugeEntries = 1ll << 21;  // pool of the neighbourhoods beyond 4096 points of ONE launch: points in all (AGH_ERR_CAPACITY beyond)

// K-1 (voxelize.hip): per-camera voxel lattice of the preprocessing step
constexpr unsigned long long kVoxMaxWords = 1ull << 28;  // 1 GiB of bitmap (a 6 m x 6 m x 3 m lattice at 3 mm)
struct VoxDesc
{
  unsigned mn_enc[2][3], mx_enc[2][3];  // order-preserving encodings of the float minima / maxima per camera
  double mn[2][3];                      // the minima as the reference holds them (10000 if no smaller coordinate)
  int dim[2][3];
  unsigned long long bits[2], word_ofs[2], n_words;
  long long n_kept[2], n_vox[2];
  long long n_occupied[2], n_pruned[2];  // k_vox_prune (agh_set_voxel_filter): the bits k_vox_mark set, and those it took out
  int error;
};
struct VoxWorkspace
{
  double lo[3], hi[3];
};
// agh_localize_batch: one capture of a batched preprocessing pass (voxelize.hip, vox_batch)
struct VoxCapture
{
  const float* xyz;  // read in place
  int64_t stride;    // floats
  int64_t n, size_left;
  VoxWorkspace ws;
  int64_t blk_off;   // its first entry among the raw block counts
  int64_t code_off;  // its first point code
  int32_t dense, pad;
};
struct VoxBatch
{
  const VoxCapture* cap = nullptr;  // device table, one per blockIdx.y; nullptr: the single cloud of the kernel's own arguments
  VoxDesc* desc = nullptr;          // device descriptors, one per capture
  VoxDesc* host_desc = nullptr;     // pinned mirrors, one per capture
  int64_t slot_words = 0;           // bitmap words per capture (a multiple of the popcount block)
};

// one capture of a batch chain, as the device sees it (localize_batch.hip; sample_mask.hip draws a masked batch's lists with it)
struct BatchCapture
{
  int64_t soff;     // its first position in the batch's sample list
  int32_t S;        // its samples
  int32_t drawn;    // 1: drawn on the device (sample_idx NULL)
  uint64_t seed;
  double ws[6];     // its workspace (the boundary filter)
  int32_t capture;  // the capture the list belongs to (a labelled batch has a list per object; otherwise list k is capture k) ...
  int32_t object;   // ... and its object there (0 without labels)
};
// the list of the chain a position of its sample list belongs to: the last list whose span starts at or before it and is not
// empty (k_batch_samples' rule)
__device__ __forceinline__ int list_of_sample(const BatchCapture* __restrict__ tab, int n_lists, int64_t sample)
{
  int l = 0;
  for (int q = 1; q < n_lists; q++)
    if (tab[q].soff <= sample && tab[q].S > 0)
      l = q;
  return l;
}

struct Comm;  // shard.hip

// Host-buffer entry points: the concatenation kernel (K4) writes every record a second time, straight into pinned host
// memory of the context, and the count and the error word into a header there -- the list is on the host when the stream
// drains, with no read-back copies behind the kernels.  rec == nullptr: no mirror (device-resident callers).
struct HostMirror
{
  agh_hypothesis* rec;  // room for `cap` records (list positions beyond it stay on the device only)
  int64_t cap;
  int64_t* hdr;         // [0] hypotheses found, [1] flags[0] as the kernel saw it
};

// Localization::filterHands (localization.cpp:364-388) as a stage of the localize chain: a hypothesis whose grasp surface lies
// closer than MIN_DIST to a face of the workspace box is dropped before the classifier.  The box reaches the kernels by value;
// on = 0 is "no filter" (agh_classify*, the sharded calls, a chain without filters_boundaries).
constexpr double kBoundaryMinDist = 0.02;  // MIN_DIST (localization.cpp:366)
struct BoundaryBox
{
  double ws[6];  // {xmin, xmax, ymin, ymax, zmin, zmax}: the workspace the preprocessing cropped with
  int32_t on;
};
inline BoundaryBox boundary_box(const double* ws)  // ws == nullptr: off
{
  BoundaryBox b{};
  if (ws)
  {
    for (int k = 0; k < 6; k++)
      b.ws[k] = ws[k];
    b.on = 1;
  }
  return b;
}

// ---- the hand drop stage (hand_drop.hip; DESIGN.md, "Hand filter" and "Hand clearance"): the second drop decision between the
// search and the classifier, one byte per hypothesis (1: dropped), which k_hog_svm, k_svm_decide and compact_kept_records honour
// beside BoundaryBox; a null pointer is "no test set" (every chain without one, agh_classify*, the sharded calls).  hand_drop_stage
// provides the bytes and a list's counters and lets the two tests write them in turn, as peers: agh_set_hand_filter's k_hand_filter
// (hand_filter.hip), then agh_set_hand_clearance's k_hand_clearance (hand_clearance.hip), which skips what the first dropped. ----
// One depth image as the observed-space test reads it: the bytes where the chain's deprojection read them, the float64
// intrinsics and pose of the caller's record (DepthView holds their float32 roundings, which the contract does not use here).
struct HandView
{
  const uint8_t* data;  // row v at data + v * stride
  int64_t stride;       // bytes
  int32_t w, h, fmt;
  float scale;
  double fx, fy, cx, cy;
  double R[9], t[3];    // pose: row-major rotation, translation
};
constexpr int kMaxHandViews = 2 * kMaxClouds;
// a batch's view table: kMaxHandViews records, the captures' first views (kMaxClouds + 1) behind them
constexpr size_t kHandViewTableBytes = sizeof(HandView) * (size_t) kMaxHandViews + sizeof(int32_t) * (size_t) (kMaxClouds + 1);
struct HandViewPair  // a single capture's views, by value
{
  HandView v[2];
  int32_t n, pad;
};
struct HandFilterArgs
{
  agh_hand_filter_params p;
  double finger_off;   // hand_outer_diameter / 2 - finger_width / 2
  double hand_depth, hand_height;
  double step;         // hand_depth / probes_per_finger
  double depths[16];   // HandGeom::depths
  int32_t n_depths, pad;
};
struct HandClearanceArgs  // what k_hand_clearance needs beside the record
{
  agh_hand_clearance_params p;
  double hand_depth;
  double depths[16];   // HandGeom::depths
  int32_t n_depths, pad;
};
// a list's counters, the device's and the pinned copy the compaction writes: the hands each test dropped (k_hand_filter's reason
// for a drop is 1 + its slot)
enum HandDropSlot : int { kDropApproach = 0, kDropWidth, kDropUnobserved, kDropClearance, kHandDropCounters };
struct HandDropState
{
  // the two sticky settings, host-side (they travel as kernel arguments)
  bool filter_set = false, clearance_set = false;
  agh_hand_filter_params filter = {};
  agh_hand_clearance_params clearance = {};
  // the buffers, made by the first chain with a test set: the drop bytes, one per record of d_out_own, regrown with s_cap; the
  // counters, kMaxClouds lists, zeroed on the chain's stream in front of the tests, and their pinned copy; a batch's view table
  uint8_t* d_drop = nullptr;
  int64_t drop_cap = 0;
  unsigned* d_counts = nullptr;
  int* h_counts = nullptr;
  uint8_t *d_views = nullptr, *h_views = nullptr;  // kHandViewTableBytes
  // what the chain in flight (then the last one collected) left: its depth images' views (capture k's are view_first[k] ..
  // view_first[k + 1] - 1), kept for its repeats; the tests it queued; the lists it counted and their hypotheses
  std::vector<HandView> views;
  std::vector<int32_t> view_first;
  bool filter_ran = false, clearance_ran = false;
  int lists = 0;
  int64_t hyp[kMaxClouds] = {};
};
// agh_set_handle_ranking (handle_rank.hip): the sticky setting, host-side; the buffers of k_handle_rank, made by the first chain
// with a ranking set -- the kept hands' margins (device and pinned), the score records in list order (device) and in rank order
// (pinned), a list's three counts (pinned) -- and what the last chain collected left for the getters
struct HandleRankState
{
  bool set = false;
  agh_handle_ranking_params p = {};
  double* d_margin = nullptr;
  double* h_margin = nullptr;          // pinned
  agh_handle_score* d_scores = nullptr;
  agh_handle_score* h_scores = nullptr;  // pinned
  int* h_counts = nullptr;             // pinned: kMaxClouds x 4 (found, below, returned)
  int64_t dev_cap = 0, host_cap = 0;   // elements
  // the chain in flight: queued with a ranking, its lists' strides in the buffers above, and whether it has margins
  bool queued = false, with_margins = false;
  int64_t slot = 0, host_slot = 0;
  // the last chain collected
  bool ran = false;
  int lists = 0;
  std::vector<agh_handle_score> scores;
  std::vector<double> margins;
  agh_handle_ranking_counts counts[kMaxClouds] = {};
};
// agh_fuse_depth (depth_fuse.hip): a slot holds one fused image in a device buffer of its own, regrown when an image is larger, the
// record handed out for it, and the event behind its last kernel and the copy of its counters
constexpr int kFuseSlots = 128, kFuseMaxFrames = 16;
enum FuseCounter : int { kFuseEmpty = 0, kFuseUnsupported, kFuseInconsistent, kFuseFused, kFuseFilled, kFuseCounters };
// a slot's counters: kFuseRows rows of kFuseCounters, a row every 256 bytes (the kernel's waves spread their atomics over the rows,
// the getter adds the rows up)
constexpr int kFuseRows = 64, kFuseRowWords = 32, kFuseSlotWords = kFuseRows * kFuseRowWords;
struct DepthFuseSlot
{
  uint8_t* d = nullptr;
  int64_t cap = 0;
  bool fused = false;
  agh_depth_image rec = {};
  hipEvent_t done = nullptr;
};
struct DepthFuseState
{
  DepthFuseSlot slot[kFuseSlots];
  // host frames, rows packed, each at a 256-byte boundary; the kernel reads them from here
  uint8_t* d_stage = nullptr;
  int64_t stage_cap = 0;
  hipEvent_t staged = nullptr;  // behind the copies of page-locked frames
  // kFuseSlots x kFuseSlotWords: the device's, a slot's zeroed in front of its kernel, and the pinned copy queued behind it
  unsigned long long* d_counts = nullptr;
  int64_t* h_counts = nullptr;
};
struct HandDropView  // what the stage hands the classifier and the compaction, host-side: all null without a test
{
  int rc = AGH_OK;
  const uint8_t* drop = nullptr;
  const unsigned* d_counts = nullptr;
  int* h_counts = nullptr;
};
struct HandDropCounts  // a list's counters as the two counts getters report them
{
  int64_t hypotheses, approach, width, unobserved, clearance;
  int64_t past_filter() const { return hypotheses - (approach + width + unobserved); }  // kept by the filter = the clearance tested
};

// ---- what a localize chain draws its samples under (include/agh.h: agh_localize_masked*, _labeled*, _clustered*, _clustered_fit*
// and their batch forms), described once for the single chain and the batch chain ----
enum class SourceKind : int
{
  None = 0,        // the whole cloud (or an explicit list)
  Mask,            // a byte per raw point, non-zero: eligible
  Labels,          // a byte per raw point, 1 .. n_objects: a list per object
  Clusters,        // no bytes: a list per connected component above a support plane
  FittedClusters   // ... above a plane the chain fits itself (plane_fit.hip; the caller's plane is not read)
};
// As the entry points take it: arrays of one entry per capture.  The single chain is the view of one capture, its entry points
// pass pointers to their own scalars.  Host bytes and all image masks are copied into a buffer of the chain; device point bytes
// are read in place (sample_source_to_device).
struct SampleSource
{
  SourceKind kind = SourceKind::None;
  const uint8_t* const* points = nullptr;       // points form: capture k's bytes, one per raw point
  const agh_sample_mask* images = nullptr;      // depth form: one record per image, parallel to the DepthCaptures' flat array
  const int32_t* n_objects = nullptr;           // Labels: capture k's objects
  const agh_cluster_params* cluster = nullptr;  // Clusters, FittedClusters: capture k's record (max_objects lists)
  const agh_plane_fit_params* fit = nullptr;    // FittedClusters: capture k's record
  bool on_device = false;
  const char* who = nullptr;                    // the entry point, for the error texts
  bool has_bytes() const { return kind == SourceKind::Mask || kind == SourceKind::Labels; }
  bool per_object() const { return kind >= SourceKind::Labels; }  // (a list per (capture, object))
  bool clustered() const { return kind >= SourceKind::Clusters; }
  bool fitted() const { return kind == SourceKind::FittedClusters; }
  int32_t objects(int k) const { return clustered() ? cluster[k].max_objects : n_objects[k]; }
};
static_assert(sizeof(agh_label_image) == sizeof(agh_sample_mask) && offsetof(agh_label_image, data) == offsetof(agh_sample_mask, data) &&
                offsetof(agh_label_image, row_stride_bytes) == offsetof(agh_sample_mask, row_stride_bytes),
  "a label image is read as a sample mask whose bytes are labels");
inline SampleSource mask_source(const uint8_t* const* points, const agh_sample_mask* images, bool on_device, const char* who)
{
  return SampleSource{ SourceKind::Mask, points, images, nullptr, nullptr, nullptr, on_device, who };
}
inline SampleSource label_source(const uint8_t* const* points, const agh_label_image* images, const int32_t* n_objects, bool on_device,
  const char* who)
{
  return SampleSource{ SourceKind::Labels, points, reinterpret_cast<const agh_sample_mask*>(images), n_objects, nullptr, nullptr, on_device, who };
}
inline SampleSource cluster_source(const agh_cluster_params* cp, const agh_plane_fit_params* fp, bool fitted, const char* who)
{
  return SampleSource{ fitted ? SourceKind::FittedClusters : SourceKind::Clusters, nullptr, nullptr, nullptr, cp, fp, false, who };
}
// Captures given as depth images (include/agh.h, agh_localize_depth*, agh_localize_depth_batch*): the flat array in capture order,
// capture k's are the next n_images[k].  k_deproject* (depth.hip) fills the context's raw buffer; from there on a chain is the
// points chain's.
struct DepthCaptures
{
  const agh_depth_image* images;
  const int32_t* n_images;
  bool on_device;
  const char* who;  // the entry point, for the error texts
};
// A fitted chain finds the plane itself: the caller's is neither read nor validated, and the record the chain keeps (and uploads)
// carries this one until the fit's.
inline void placeholder_plane(agh_cluster_params* cp)
{
  cp->plane[0] = cp->plane[1] = cp->plane[3] = 0.0;
  cp->plane[2] = 1.0;
}
// The name of a chain in the texts of the errors found behind its synchronisation.
inline const char* chain_name(bool single, SourceKind kind)
{
  switch (kind)
  {
    case SourceKind::Labels: return single ? "agh_localize_labeled" : "agh_localize_batch_labeled";
    case SourceKind::Clusters: return single ? "agh_localize_clustered" : "agh_localize_batch_clustered";
    case SourceKind::FittedClusters: return single ? "agh_localize_clustered" : "agh_localize_batch_clustered_fit";
    default: return single ? "agh_localize" : "agh_localize_batch";
  }
}
// The device-resident form of a source, which a chain keeps for a repeat of the whole call: where each capture's bytes lie (the
// chain's own copy, or the caller's device memory) and copies of the caller's records.
struct StoredSource
{
  SourceKind kind = SourceKind::None;
  const char* who = "";                   // chain_name
  std::vector<const uint8_t*> d_bytes;    // has_bytes: per capture (sample_source_to_device)
  std::vector<int32_t> n_objects;         // per_object: per capture
  std::vector<agh_cluster_params> cluster;
  std::vector<agh_plane_fit_params> fit;
  bool per_object() const { return kind >= SourceKind::Labels; }
  bool clustered() const { return kind >= SourceKind::Clusters; }
  bool fitted() const { return kind == SourceKind::FittedClusters; }
  // (src: null for a chain without a source)
  void keep(const SampleSource* src, int C, bool single)
  {
    *this = StoredSource();
    kind = src ? src->kind : SourceKind::None;
    who = chain_name(single, kind);
    if (!src)
      return;
    for (int k = 0; k < C && src->per_object(); k++)
      n_objects.push_back(src->objects(k));
    if (src->clustered())
      cluster.assign(src->cluster, src->cluster + C);
    if (src->fitted())
    {
      fit.assign(src->fit, src->fit + C);
      for (agh_cluster_params& q : cluster)
        placeholder_plane(&q);
    }
  }
  // the source a repeat re-enters with
  SampleSource view() const
  {
    return SampleSource{ kind, d_bytes.data(), nullptr, n_objects.data(), cluster.data(), fit.data(), true, who };
  }
};

// agh_localize_begin / _stage / _end (api.hip): the one chain in flight and the capture staged for the next one
struct LocalizeState
{
  bool active = false;        // a chain is queued and agh_localize_end has not collected it
  bool repeated = false;      // inside the one repeat of a whole call (the voxel lattice outgrew the speculative bitmap)
  bool deferred = false;      // the voxel count is still on the device
  bool classify = false, with_sequential = false, explicit_samples = false;
  bool filters = false;       // filters_boundaries: Localization::filterHands between the search and the classifier
  int64_t S = 0, nv = 0;
  int32_t min_inliers = 0;
  double min_length = 0.0, x1 = 0.0, x2 = 0.0;
  agh_localize_params lp{};   // (sample_idx cleared: the list lives in the pinned staging)
  const float* d_raw = nullptr;  // where the chain read the raw capture (the context's raw buffer or the caller's device memory)
  int64_t dev_stride = 0, n_raw = 0;
  // What the samples are drawn under, as a repeat of the whole call re-enters with it: a mask (sample_mask.hip) in the context's
  // d_mask or in the caller's device memory; labels there (sample_labels.hip), S samples for each object; the cloud's own
  // components (sample_cluster.hip), above a given or a fitted plane (plane_fit.hip).  From the classifier on the tail of a chain
  // with a list per object is the batch chain's (localize_batch.hip).
  StoredSource source;
  int objects() const { return source.per_object() ? source.n_objects[0] : 0; }  // the lists of such a chain (0: the one list)
  // agh_localize_batch_begin / _stage / _end (localize_batch.hip) share the one chain and the one staged set of the context
  bool batch = false;         // the chain in flight is a batch's (agh_localize_batch_end collects it, not agh_localize_end)
  bool staged = false;        // stage_captures: a set of captures is (being) copied into d_stage_xyz, packed end to end,
  int staged_captures = 0;    // 0 = the one capture of agh_localize_stage; C = the C captures of agh_localize_batch_stage,
  std::vector<const float*> staged_src;  // with these sources, strides and counts (one entry for agh_localize_stage's)
  std::vector<int64_t> staged_stride, staged_n;
  // ... or, staged_depth, the depth images of agh_localize_depth_stage, rows packed, in d_depth_stage (depth.hip): one staged set
  // of any kind; a points begin never adopts images, a depth begin never adopts points
  bool staged_depth = false;
  std::vector<agh_depth_image> staged_images;  // (data, width, height, row_stride_bytes and format identify the set)
  bool staged_depth_is(const agh_depth_image* im, int count) const
  {
    if (!staged || !staged_depth || (int) staged_images.size() != count)
      return false;
    for (int k = 0; k < count; k++)
    {
      const agh_depth_image& s = staged_images[k];
      if (s.data != im[k].data || s.width != im[k].width || s.height != im[k].height ||
          s.row_stride_bytes != im[k].row_stride_bytes || s.format != im[k].format)
        return false;
    }
    return true;
  }
  // the begin that may adopt the staged set: is it these `count` captures (as_batch: of a batch), by pointer, stride and count?
  bool staged_is(const float* const* xyz, const int64_t* stride_bytes, const int64_t* n, int count, bool as_batch) const
  {
    if (!staged || staged_depth || staged_captures != (as_batch ? count : 0) || (int) staged_src.size() != count)
      return false;
    for (int k = 0; k < count; k++)
      if (staged_src[k] != xyz[k] || staged_stride[k] != stride_bytes[k] || staged_n[k] != n[k])
        return false;
    return true;
  }
};

struct PlaneState;
struct LocalizeBatchState;

// What the last chain a context collected left for the getters of the chains (agh_get_sample_mask_count, _label_counts,
// _cluster_info, _cluster_labels, _plane_fit*, and the agh_get_batch_* ones).  Value-initialised: no chain, or one that left
// nothing.  agh_localize_end and agh_localize_batch_end start with `results = ChainResults{}` and fill it behind their
// synchronisation; a getter answers for exactly one (kind, batch) -- a single getter refuses after a batch of its kind, and the
// reverse.
struct ChainResults
{
  SourceKind kind = SourceKind::None;
  bool batch = false;
  int32_t captures = 0;                   // a batch's captures (the single chain: 1)
  int32_t lists = 0;                      // the entries of counts: 1 (a single mask), the captures (a masked batch), else the lists
  int64_t counts[kMaxClouds] = {};        // eligible voxels: M, M_k, or per list M_j / M_{k,j} (a clustered chain: the objects' sizes)
  int64_t nv = 0;                         // clustered: the voxels of the bound cloud (batch), which agh_get_*cluster_labels copies
  int64_t cluster_info[kMaxClouds][4] = {};  // clustered, per capture: foreground, components, objects, qualifying
  int32_t cluster_ids[kMaxClouds] = {};      // ... per list: the smallest (capture-local) voxel index of the object, -1: none
  int32_t fit_candidates[kMaxClouds] = {};   // fitted, per capture: n_candidates
  agh_plane_fit_result fit_results[kMaxClouds] = {};  // ... and the result record
  bool is(SourceKind k, bool of_batch) const { return kind == k && batch == of_batch; }
  bool is_clustered(bool of_batch) const { return kind >= SourceKind::Clusters && batch == of_batch; }
};

struct Ctx
{
  agh_params p;
  HandGeom geom;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t copy_done = nullptr;
  hipEvent_t copy_gate = nullptr;   // recorded on the build's stream before its kernels: the camera-id copy waits for earlier work only
  hipEvent_t xyz_copied = nullptr;  // host-buffer agh_set_cloud from PINNED memory: recorded behind the coordinates' copy
  bool cam_copy_on_copy_stream = false;  // the last grid_build put the camera ids on copy_stream (copy_done was recorded)
  hipStream_t copy_stream = nullptr;  // host-buffer agh_set_cloud: the camera ids go up here while the grid build's first kernels run
  bool copy_stream_failed = false;    // its creation failed once: not retried (the ids go up on the build's stream)
  std::string err;

  // cloud
  int64_t n = 0;
  const float* d_xyz = nullptr;  // borrowed or owned
  int64_t stride_floats = 3;
  const int32_t* d_cam = nullptr;
  float* own_xyz = nullptr;
  int32_t* own_cam = nullptr;
  int64_t own_cap = 0;
  int64_t own_cap_floats = 0;
  int32_t* d_idx_own = nullptr;  // device copy of a host sample list
  int64_t idx_cap = 0;
  // pinned staging of the host-buffer entry points (hipHostMalloc, device-visible): [256-byte header | sample indices |
  // records]; the caller's pageable buffers are copied from / to it by the CPU, the GPU reads and writes it directly
  uint8_t* h_pin = nullptr;
  int64_t h_pin_samples = 0, h_pin_records = 0;
  HostMirror mirror{ nullptr, 0, nullptr };  // set by agh_find_hands around its device call
  uint8_t* h_pin_handles = nullptr;  // agh_find_handles: [256-byte header | hands in | handles out | inlier indices out]
  int64_t h_pin_handles_cap = 0;     // in hands
  bool handles_sequential = false;   // the previous handle search needed k_handle_greedy (a row longer than kMaxRow, two waves' worth): launch it along
  uint8_t* h_pin_keep = nullptr;     // agh_classify: the keep flags, written by K3 itself
  int64_t h_pin_keep_cap = 0;

  // preprocessing (K-1)
  VoxDesc* d_vox_desc = nullptr;
  uint8_t* d_vox_code = nullptr;   // per raw point: 0 dropped, 1 | cam << 1 kept
  int* d_vox_blk = nullptr;        // finite-point counts per 1024 raw points
  int* d_vox_blk2 = nullptr;       // popcounts per 4096 bitmap words
  long long* d_vox_total = nullptr;
  unsigned* d_vox_bitmap = nullptr;
  int64_t vox_bitmap_cap = 0;      // words (a multiple of the popcount block)
  int64_t vox_last_words = 0;   // lattice words of the last preprocessed cloud (a much larger kept bitmap is dropped)
  // agh_set_voxel_filter (voxelize.hip, k_vox_prune): the sticky filter every voxelisation of this context applies, host-side (the
  // kernel takes the two ints as arguments); d_vox_pruned: the second bitmap, of d_vox_bitmap's capacity, made by the first filtered
  // voxelisation -- k_vox_prune writes it and the two pointers are swapped, so that d_vox_bitmap is the pruned one to all later
  // code; vox_filter_captures: the captures of the LAST voxelisation if it ran filtered (their counts are in the pinned descriptor
  // mirrors at vox_filter_mirror: h_vox_desc, or the batch's), else 0
  bool voxel_filter_set = false;
  agh_voxel_filter_params voxel_filter = {};
  unsigned* d_vox_pruned = nullptr;
  int64_t vox_pruned_cap = 0;
  int vox_filter_captures = 0;
  const VoxDesc* vox_filter_mirror = nullptr;
  VoxDesc* h_vox_desc = nullptr;   // pinned host mirror of the descriptor, written by k_vox_lattice / k_vox_totals
  float* d_vox_xyz = nullptr;      // voxelised cloud (packed xyz) and camera ids
  int32_t* d_vox_cam = nullptr;
  int64_t vox_cap = 0;
  float* d_raw_xyz = nullptr;      // device copy of a raw host cloud
  float* d_stage_xyz = nullptr;    // ... and of the NEXT one (agh_localize_stage); the two change places when it is adopted
  int64_t stage_cap = 0;           // floats
  hipStream_t stage_stream = nullptr;
  hipEvent_t stage_done = nullptr;
  hipEvent_t raw_read = nullptr, stage_read = nullptr;  // recorded on `stream` behind the last batch chain that read d_raw_xyz /
  bool raw_read_set = false, stage_read_set = false;    // d_stage_xyz (they change places with the buffers)
  LocalizeState loc;
  int64_t raw_cap = 0;             // floats
  // sample masks (sample_mask.hip), allocated by the first masked call
  uint8_t* d_mask = nullptr;       // the chain's copy of a host mask (depth masks: rows packed, image after image)
  int64_t mask_cap = 0;            // bytes
  unsigned* d_mask_bitmap = nullptr;  // eligibility bitmap: the voxel bitmap's layout, grown with it
  int64_t mask_bitmap_cap = 0;     // words
  int* d_mask_blk = nullptr;       // eligible bits per 4096 bitmap words, then their exclusive scan
  long long* d_mask_total = nullptr;  // M, the eligible voxels
  int32_t* d_mask_list = nullptr;  // E: the eligible voxel indices, ascending
  int64_t mask_list_cap = 0;
  // label images (sample_labels.hip), allocated by the first labelled call; the lists E_j share d_mask_list
  unsigned* d_label_rank = nullptr;   // per bitmap word: the voxel bits in front of it inside its 4096-word block
  int64_t label_rank_cap = 0;         // words
  unsigned long long* d_label_set = nullptr;  // per voxel: the set of the objects eligible there
  int64_t label_set_cap = 0;
  int* d_label_groups = nullptr;      // per object and work-group of 256 voxels: eligible voxels, then their exclusive scan
  int64_t label_group_cap = 0;
  long long* d_label_totals = nullptr;  // kMaxClouds: the M_j
  long long* h_label_counts = nullptr;  // pinned: the M_j, written by the chain
  // clusters as the label source (sample_cluster.hip), allocated by the first clustered call
  int* d_cluster_parent = nullptr;    // per voxel: the union-find's parent, then its root (-1: background)
  int* d_cluster_size = nullptr;      // per voxel: a root's size, then -1 - rank for the roots that are objects
  uint8_t* d_cluster_label = nullptr; // per voxel: 0 or object + 1 (agh_get_cluster_labels)
  int64_t cluster_cap = 0;
  unsigned long long* d_cluster_counts = nullptr;  // foreground voxels, components
  long long* h_cluster_table = nullptr;  // pinned: counts, M_j and ids, written by the chain (k_cluster_select)
  // a fitted plane for the clustered chain (plane_fit.hip), allocated by the first fitted call: nothing per point
  void* d_fit = nullptr;                       // candidates' indices and planes, counts, sums and the ClusterDev record (PlaneFitBuffers)
  agh_plane_fit_result* h_fit_result = nullptr;  // pinned: written by the chain (k_fit_finish)
  ChainResults results;               // what the last chain collected left for the agh_get_* getters of the chains
  // agh_localize_depth* (depth.hip): a host capture's depth images, rows packed, image k at depth_image_offset(k); the NEXT
  // capture's (agh_localize_depth_stage) in the second buffer; the two change places when a staged set is adopted
  uint8_t* d_depth = nullptr;
  uint8_t* d_depth_stage = nullptr;
  int64_t depth_cap = 0, depth_stage_cap = 0;  // bytes
  hipEvent_t depth_read = nullptr;  // recorded on `stream` behind the last k_deproject that read one of the two
  // agh_localize_depth_batch* (depth.hip): the view table of k_deproject_batch, kMaxDepthViews records, filled in the pinned copy
  // and uploaded on `stream` in front of the launch (a batch's host images lie in d_depth too, each at a 256-byte boundary)
  uint8_t* d_depth_views = nullptr;
  uint8_t* h_depth_views = nullptr;  // pinned
  // agh_set_depth_filter (depth.hip): the sticky filter every deprojection of this context applies, host-side (the kernels take it
  // as arguments); the per-view counters of k_deproject_filtered*, kMaxDepthViews x 4, zeroed on the launch's stream in front of
  // it; filter_views: the views of the LAST deprojection if it ran with a filter, else 0, and the stream it ran on
  bool depth_filter_set = false;
  agh_depth_filter_params depth_filter = {};
  int64_t* d_filter_counts = nullptr;
  int filter_views = 0;
  hipStream_t filter_stream = nullptr;
  HandDropState hand_drop;         // the hand drop stage (hand_drop.hip): agh_set_hand_filter, agh_set_hand_clearance
  HandleRankState handle_rank;     // agh_set_handle_ranking (handle_rank.hip)
  DepthFuseState* fuse = nullptr;  // agh_fuse_depth's slots, staging buffer and counters (depth_fuse.hip), made by its first call
  PlaneState* plane = nullptr;     // agh_remove_plane's buffers and last result (plane.hip), made by its first call
  LocalizeBatchState* lbatch = nullptr;  // agh_localize_batch's buffers (localize_batch.hip), made by its first call
  bool batch_active = false;       // inside agh_localize_batch (agh_localize_begin refuses)

  // handle search (K5)
  agh_hypothesis* d_h_hands = nullptr;
  unsigned long long* d_h_bits = nullptr;
  int* d_h_rowcnt = nullptr;
  int* d_h_first = nullptr;
  int* d_h_n = nullptr;
  int* d_h_idx = nullptr;
  int* d_h_counts = nullptr;  // HandleCounts
  int* d_h_tmp = nullptr;     // h_cap: scratch of k_handle_batch (inlier lists in commit order)
  agh_handle* d_h_handles = nullptr;
  int64_t h_cap = 0;

  // grid (per cloud of the batch)
  int n_clouds = 1;
  int clouds_cap = 0;               // clouds the tables below are allocated for
  std::vector<int64_t> cloud_off;   // host copy, n_clouds + 1
  std::vector<int32_t> cloud_off_i32;
  bool cloud_off_on_device = false;
  bool defer_cloud_count = false;  // set by the deferred preprocessing for the agh_set_cloud_device call it makes next
  bool n_is_bound = false;  // agh_localize, between its launches and its synchronisation: `n` is the RAW point count, an upper bound of
                            // the voxelised cloud's; the true count is d_cloud_off[1], written by the voxeliser
  int* d_cloud_off = nullptr;       // kMaxClouds + 1
  int32_t* d_scloud = nullptr;      // s_cap: cloud of every sample of the last call (written by k_taubin_moments)
  GridDesc* d_desc = nullptr;       // clouds_cap: the descriptors of the last build (what the searches read)
  GridDesc* d_desc_next = nullptr;  // clouds_cap: the descriptors the next build keeps (decided on the device by k_cell_scan)
  float* d_bbox_part = nullptr;     // clouds_cap x kBboxBlocks x 6 partial extrema of k_bbox
  float* d_count_part = nullptr;    // clouds_cap x kCountBlocks x 6 partial extrema of k_cell_count
  unsigned* d_grid_miss = nullptr;  // builds of a cloud that had points outside its kept descriptor
  bool grid_miss_zeroed = false;
  bool grid_force_cold = false;     // AGH_GRID_COLD=1: every build takes the k_bbox path (A/B measurement)
  int grid_key_clouds = 0;          // clouds of the last build: another number of them means a cold build
  int64_t grid_builds = 0, grid_cold_builds = 0;
  int* d_cell_start = nullptr;      // clouds_cap x kCellStride
  int* d_cell_count = nullptr;      // clouds_cap x kCellCap
  int* d_block_sums = nullptr;
  unsigned long long* d_tile_state = nullptr;  // clouds_cap x kCellCap / 1024 look-back descriptors of k_cell_scan, tagged with the build number
  unsigned build_gen = 0;
  bool grid_clean = false;      // cell counts, bbox and counters are in their reset state (self-cleaning kernels)
  int* d_cell_of = nullptr;     // n
  int* d_rank_of = nullptr;     // n: rank of a point inside its cell
  float4* d_sorted = nullptr;   // n
  int64_t grid_cap = 0;
  bool has_cloud = false;
  const int32_t* pending_cam_host = nullptr;  // host-buffer agh_set_cloud: camera ids still to upload (grid_build does it while
  int64_t pending_cam_n = 0;                  // its first three kernels run: only k_scatter reads them)
  bool cloud_async = false;     // agh_set_cloud (host buffers) left the grid build running on `stream`; a search on ANOTHER
                                // stream must first wait for it (order_after_cloud)

  // agh_set_cloud_cam_origins: camera origins per cloud of the bound batch, in place of p.cam_origin (sticky; 0 rows = none)
  int cam_tab_rows = 0;
  double* d_cam_tab = nullptr;      // kMaxClouds x 6 doubles
  double* h_cam_tab = nullptr;      // pinned staging of the upload, and what agh_get_cloud_cam_origins reads
  hipEvent_t cam_tab_up = nullptr;  // recorded behind the upload on `stream`
  bool cam_tab_async = false;       // the upload may still be running on `stream`: a search on ANOTHER stream waits for the event

  // per-call buffers (sized for s_cap samples)
  int64_t s_cap = 0;
  int32_t* d_samples = nullptr;
  double* d_sums = nullptr;        // s_cap * kSumStride
  int32_t* d_nt = nullptr;         // n_taubin
  int32_t* d_ovf = nullptr;        // {count, samples...}: the samples k_taubin_moments<1152> hands on to the 4096 class (s_cap + 16)
  int32_t* d_nh = nullptr;         // n_hands
  int32_t* d_status = nullptr;
  int* d_weight = nullptr;         // candidate count of each sample's hand-search ball (scheduling weight)
  uint8_t* d_vmask = nullptr;      // per sample: orientations with a hypothesis (k_hand_sweep -> concatenation)
  int* d_order = nullptr;          // samples by descending n_t: blockIdx -> sample of k_taubin_frame
  int* d_order_sweep = nullptr;    // blocks of 32 samples, heaviest first: blockIdx -> sample of k_hand_sweep (made by K1b)
  int order_frame_s = 0;           // ... and the same for k_taubin_frame's longest-first order (d_order)
  const int32_t* order_frame_samples = nullptr;
  int order_sweep_s = 0;           // the sample count / list that order was made for (0: none)
  const int32_t* order_sweep_samples = nullptr;
  float4* d_nbr = nullptr;         // s_cap * nbr_stride sorted neighbour lists
  int64_t nbr_stride = 0;
  double* d_eig = nullptr;         // s_cap * 12 : params[10], eigenvalue, valid
  agh_frame* d_frames = nullptr;
  agh_hypothesis* d_slots = nullptr;   // s_cap * 8
  uint32_t* d_images = nullptr;        // s_cap * 8 * kImageWords
  int32_t* d_slot_index = nullptr;     // compacted position of each slot (or -1)
  int32_t* d_scan_tmp = nullptr;
  agh_hypothesis* d_out_own = nullptr;  // compacted hypotheses when the caller gave host memory
  int64_t* d_nout = nullptr;
  uint32_t* d_out_images = nullptr;     // compacted images (s_cap * 8 * kImageWords)
  uint32_t* d_images_cam = nullptr;     // training side: per slot the camera-0 and camera-1 images (s_cap * 16 * kImageWords)
  int64_t images_cam_cap = 0;           // in samples
  bool training_images = false;         // agh_set_training_images
  bool last_has_cam_images = false;     // the last hand sweep filled d_images_cam
  int32_t* d_draw_ofs = nullptr;        // RAND50: offset of each sample's 50 draws
  int32_t* d_draws = nullptr;
  int64_t draws_cap = 0;
  int64_t last_s = 0;
  int32_t epoch = 0;         // stamp of the last agh_find_hands* call (agh_hypothesis::epoch; process-wide counter)
  int64_t last_nout = -1;
  int64_t last_cap = 0;
  agh_hypothesis* d_out_last = nullptr;  // where the last call's compacted records live
  int64_t* d_nout_last = nullptr;
  int32_t* d_flags = nullptr;  // [0] any overflow, [1] ...
  bool huge_classes = false;  // ... and the 6144 class behind those (K1a through global scratch, K1c in LDS): neighbourhoods of up to
                              // kHugeCap points; enabled like big_classes, by the first call that needs it (AGH_ERR_RETRY once)
  float4* d_huge_stage = nullptr;            // kHugeEntries points of the neighbourhoods beyond 4096, unsorted
  unsigned long long* d_huge_key = nullptr;  // ... their (d2, index) keys
  float4* d_huge_sorted = nullptr;           // ... the sorted lists of those beyond the per-sample scratch (> kHugeCap)
  double* d_huge_normals = nullptr;          // ... and their normals (3 x kHugeEntries: x | y | z), K1c beyond the LDS classes
  long long* d_huge_base = nullptr;          // per sample: first pool entry of its neighbourhood (s_cap)
  unsigned long long* d_huge_count = nullptr;  // entries handed out in this launch
  bool big_classes = false;  // launch the larger capacity classes of K1a / K1c too (sticky; set by the first call that
                             // met a neighbourhood beyond the first class, see AGH_ERR_RETRY)
  bool zero_flags_pending = false;  // the next k_taubin_moments launch clears d_flags first

  // normals for the antipodal test (cloud_normals_, hand_search.cpp:13-14)
  double* d_normals = nullptr;  // 3 * n
  int64_t normals_cap = 0;
  bool has_normals = false;

  // svm / hog
  float* d_svm_w = nullptr;
  double svm_rho = 0.0;
  bool has_svm = false;
  // a model that is not the compacted linear vector (several support vectors and/or the POLY degree-2 kernel)
  bool svm_general = false;
  int svm_kernel = 0;               // AGH_SVM_*
  int svm_n_sv = 1;
  float* d_svm_svT = nullptr;       // support vectors, tiles of 64 (train.hip: xt_index)
  double* d_svm_alpha = nullptr;
  float* d_cls_desc = nullptr;      // descriptors of the hypotheses being classified (general models)
  int64_t cls_desc_cap = 0;         // in hypotheses
  float* d_cls_kbuf = nullptr;      // kernel values, hypotheses x support vectors
  int64_t cls_kbuf_cap = 0;         // in floats
  HogTablesDev* d_hog = nullptr;
  HandGeom* d_geom = nullptr;
  float* d_desc_out = nullptr;  // optional descriptor dump
  double* d_svm_sums = nullptr;
  uint8_t* d_keep = nullptr;
  int64_t keep_cap = 0;
  uint32_t* d_cls_images = nullptr;  // agh_classify_images: uploaded packed images, keep flags, decision values
  uint8_t* d_cls_keep = nullptr;
  double* d_cls_sums = nullptr;
  int64_t cls_images_cap = 0;

  // multi-GPU: the sample set of one cloud sharded over the ranks of a communicator (shard.hip)
  Comm* comm = nullptr;
  uint8_t* d_xbuf = nullptr;      // n_ranks segments of [160-byte header | seg_records records], all-gathered in place
  int64_t xbuf_bytes = 0;
  double* d_nbuf = nullptr;       // n_ranks segments of per-sample normals (antipodal mode), all-gathered in place
  int64_t nbuf_doubles = 0;
  int64_t* d_xcnt = nullptr;      // n_ranks RAND50 draw counts + scratch (kXcntWords; shard.hip)
  bool shard_symmetric_error = false;  // the last sharded device call failed on something every rank saw alike, after the ranks
                                       // had met in a collective: nobody is left waiting, the communicator stays usable
  int64_t shard_seg_override = 0;    // agh_comm_set_segment_records
  int shard_inject = 0;              // agh_comm_inject_fault (testing aid): sites that fail on this rank, one shot each
  bool shard_full_exchange = false;  // exchange all 8 slots per sample instead of the 2-per-sample prefix
  int64_t shard_seg_records = 0, shard_seg_bytes = 0, shard_S = 0;
  agh_hypothesis* shard_out = nullptr;  // the caller's merged list of the last sharded search
  int64_t shard_cap = 0;
  int64_t* shard_nout = nullptr;
  int64_t shard_last_n = -1;            // length of the merged list, once a host entry point has read it
  bool shard_host_list = false;         // the last sharded search was agh_find_hands_sharded (the list is d_out_own)
  int shard_hdr_search = 0;             // kHdrRank* bits the last sharded search left in this rank's own segment header
  int shard_hdr_bits = 0;               // ... and the kHdrRank* bits that header carries now (a failed classification adds one)

  long long* d_dbg = nullptr;  // AGH_DEBUG_CLOCKS: per-sample phase timestamps of k_hand_sweep (dumped to a file)
  int debug_stop_sweep = 0;    // AGH_DEBUG_STOP_SWEEP: phase-timing aid, see k_hand_sweep
  int debug_stop_moments = 0;  // AGH_DEBUG_STOP_MOMENTS
  int debug_stop_frame = 0;    // AGH_DEBUG_STOP_FRAME
  int debug_stop_hog = 0;      // AGH_DEBUG_STOP_HOG  (all four only in builds with -DAGH_DEBUG_HOOKS)

  // timing
  std::vector<hipEvent_t> ev;
  std::vector<const char*> ev_name;
  int ev_used = 0;
  unsigned prof_calls = 0;     // profile 3: calls seen; every fourth one is timed
  agh_timing timing;
  int32_t timing_counts[AGH_TIMING_SLOTS] = { 0 };  // timed launches per slot of the last agh_get_timing (agh_get_timing_counts)
};

inline int class_level(const Ctx* c) { return c->huge_classes ? 2 : (c->big_classes ? 1 : 0); }

// A HIP call that failed leaves its own text and HIP's in the context's error string, and the function returns AGH_ERR_HIP -- or
// on_fail, evaluated after the string is set: whatever first undoes what the function has queued (chain_fail, stage_captures).
inline bool hip_failed(Ctx* c, hipError_t e, const char* expr)
{
  if (e != hipSuccess)
    c->err = std::string(expr) + ": " + hipGetErrorString(e);
  return e != hipSuccess;
}
#define AGH_HIPCHK(c, expr) do { if (agh::hip_failed((c), (expr), #expr)) return AGH_ERR_HIP; } while (0)
#define AGH_HIPCHK_OR(c, expr, on_fail) do { if (agh::hip_failed((c), (expr), #expr)) return (on_fail); } while (0)

// ---- the localize chains' plumbing (localize.hip, localize_batch.hip; the uploads and the label buffers: api.hip, hog_svm.hip,
// shard.hip too) ----
// A chain failed between its launches and its synchronisation, while the host only knows a BOUND of the cloud's size: the context
// must not be left believing the bound is the cloud.
inline void drop_bound_cloud(Ctx* c)
{
  if (!c->n_is_bound)
    return;
  c->n_is_bound = false;
  c->has_cloud = false;
  c->n = 0;
  c->cloud_off_on_device = false;
}
// ... and every such error return first drains the stream: a pinned source may still be in flight, and the caller may free it as
// soon as the call returns.
inline int chain_fail(Ctx* c, int code)
{
  (void) hipStreamSynchronize(c->stream);
  drop_bound_cloud(c);
  return code;
}
// a raw capture as the entry points take it: n points of stride_bytes each, x y z first
inline bool bad_capture(const float* xyz, int64_t stride_bytes, int64_t n)
{
  return n < 0 || n >= (1ll << 30) || stride_bytes < 12 || (stride_bytes % 4) != 0 || (n > 0 && !xyz);
}
// the output arguments of agh_localize* and agh_localize_batch*, as the entry points take them
struct ChainOutputs
{
  agh_handle* handles;
  int64_t handle_cap;
  int32_t* inlier_idx;
  int64_t idx_cap;
  agh_hypothesis* hands;
  int64_t hands_cap;
  int32_t* samples;
  bool bad() const
  {
    return handle_cap < 0 || idx_cap < 0 || hands_cap < 0 || (handle_cap > 0 && !handles) || (idx_cap > 0 && !inlier_idx) ||
           (hands_cap > 0 && !hands);
  }
};
// A host capture goes up as it lies in host memory -- one contiguous copy: a strided 2-D copy of 12 of every 32 bytes runs at a
// fraction of the PCIe rate -- and the kernels read it with the caller's stride; strides above 32 bytes are repacked to 12.
inline int64_t device_stride(int64_t stride_bytes) { return stride_bytes <= 32 ? stride_bytes : 12; }
inline hipError_t upload_capture(float* dst, const float* xyz, int64_t stride_bytes, int64_t n, hipStream_t st)
{
  if (n <= 0)
    return hipSuccess;
  if (device_stride(stride_bytes) == stride_bytes)  // (all but the last point's padding, which may lie outside the caller's buffer)
    return hipMemcpyAsync(dst, xyz, (size_t) (n * stride_bytes - (stride_bytes - 12)), hipMemcpyHostToDevice, st);
  return hipMemcpy2DAsync(dst, 12, xyz, (size_t) stride_bytes, 12, (size_t) n, hipMemcpyHostToDevice, st);
}
// The classifier's labels and decision sums for `count` hypotheses.  Growing drops the old pair first and counts nothing as held
// until both allocations have succeeded.
inline hipError_t ensure_keep_buffers(Ctx* c, int64_t count)
{
  if (count <= c->keep_cap)
    return hipSuccess;
  if (c->d_keep)
    (void) hipFree(c->d_keep);
  if (c->d_svm_sums)
    (void) hipFree(c->d_svm_sums);
  c->d_keep = nullptr;
  c->d_svm_sums = nullptr;
  c->keep_cap = 0;
  hipError_t e = hipMalloc((void**) &c->d_keep, (size_t) count);
  if (e == hipSuccess)
    e = hipMalloc((void**) &c->d_svm_sums, (size_t) count * sizeof(double));
  if (e == hipSuccess)
    c->keep_cap = count;
  return e;
}
// the slices of h_pin_handles (ensure_handle_buffers: room for h_pin_handles_cap of each)
struct HandlePins
{
  int* counts;            // the 256-byte header: [0..3] the handle search's (HandleMirror::counts), [4..6] k_compact_kept's
  agh_hypothesis* hands;
  agh_handle* handles;
  int32_t* idx;
};
inline HandlePins handle_pins(const Ctx* c)
{
  HandlePins p;
  p.counts = reinterpret_cast<int*>(c->h_pin_handles);
  p.hands = reinterpret_cast<agh_hypothesis*>(c->h_pin_handles + 256);
  p.handles = reinterpret_cast<agh_handle*>(p.hands + c->h_pin_handles_cap);
  p.idx = reinterpret_cast<int32_t*>(p.handles + c->h_pin_handles_cap);
  return p;
}

// include/agh.h: between agh_localize_begin and agh_localize_end only agh_localize_stage and the calls listed there may run on a
// context.  The others refuse here, before they touch a buffer: the chain in flight owns the per-call buffers (d_out_own, d_flags,
// d_idx_own, the pinned mirrors) and the cloud, whose size may still be only a bound (n_is_bound).
inline bool refuse_mid_chain(Ctx* c, const char* fn)
{
  if (!c->loc.active)
    return false;
  c->err = std::string(fn) + ": a localize chain is in flight on this context (agh_localize_end first)";
  return true;
}

// Page-locked host memory (hipHostMalloc / hipHostRegister)?  A copy from it is truly asynchronous: it returns before the
// source has been read, where a pageable copy returns after.
inline bool is_pinned_host(const void* p)
{
  if (!p)
    return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess)
  {
    (void) hipGetLastError();  // (an unregistered pointer is an error on older runtimes, hipMemoryTypeUnregistered on newer ones)
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// The stage stream and its events, made by the first agh_localize_stage / agh_localize_batch_stage of a context.
inline int ensure_stage_stream(Ctx* c, const char* fn)
{
  if (c->stage_stream)
    return AGH_OK;
  hipStream_t s = nullptr;
  hipEvent_t e[3] = { nullptr, nullptr, nullptr };
  bool ok = hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
  for (int k = 0; k < 3 && ok; k++)
    ok = hipEventCreateWithFlags(&e[k], hipEventDisableTiming) == hipSuccess;
  if (!ok)
  {
    for (hipEvent_t q : e)
      if (q)
        (void) hipEventDestroy(q);
    if (s)
      (void) hipStreamDestroy(s);
    c->err = std::string(fn) + ": no stream or event";
    return AGH_ERR_HIP;
  }
  c->stage_stream = s;
  c->stage_done = e[0];
  c->raw_read = e[1];
  c->stage_read = e[2];
  return AGH_OK;
}
// A staged capture (or batch) is adopted: the two raw buffers change places, and so do the events behind their last readers.
inline void swap_raw_buffers(Ctx* c)
{
  std::swap(c->d_raw_xyz, c->d_stage_xyz);
  std::swap(c->raw_cap, c->stage_cap);
  std::swap(c->raw_read, c->stage_read);
  std::swap(c->raw_read_set, c->stage_read_set);
}

// The table K1c and K2 take in place of the context's origins (null: none set).
inline const double* cloud_cam_table(const Ctx* c) { return c->cam_tab_rows > 0 ? c->d_cam_tab : nullptr; }
// A call about to use the origins on a batch of n_clouds clouds: a table must have exactly that many rows (include/agh.h).
inline bool cam_table_mismatch(Ctx* c, const char* fn, int n_clouds)
{
  if (c->cam_tab_rows == 0 || c->cam_tab_rows == n_clouds)
    return false;
  c->err = std::string(fn) + ": the camera-origin table (agh_set_cloud_cam_origins) holds " + std::to_string(c->cam_tab_rows) +
           " rows, the batch " + std::to_string(n_clouds) + " clouds; set a table of that many rows or clear it";
  return true;
}
// ... and the upload of the table is in front of that call's kernels: a search on the context's own stream is in order behind
// it; one on another stream waits for the event ON THE DEVICE (no host stall; a wait on a completed event costs next to nothing).
// The flag comes down where the host is known to have waited for the context's stream: the next setter, agh_synchronize.
inline hipError_t order_after_cam_table(Ctx* c, hipStream_t st)
{
  if (!c->cam_tab_async || st == c->stream)
    return hipSuccess;
  return hipStreamWaitEvent(st, c->cam_tab_up, 0);
}

// a search about to run on `st`: if the host-buffer agh_set_cloud left its grid build running on the context's stream and `st`
// is another stream, wait for the build first (streams the caller brings may be non-blocking ones)
inline hipError_t order_after_cloud(Ctx* c, hipStream_t st)
{
  if (!c->cloud_async || st == c->stream)
    return hipSuccess;  // (in order behind the build on the context's own stream: the flag stays up for a LATER search on another
                        // stream, which is not -- ADVICE r4)
  c->cloud_async = false;
  return hipStreamSynchronize(c->stream);
}

// Bits of d_flags[0]: 1 = a Taubin neighbourhood beyond the capacity classes this context launched, 2 = output buffer too small,
// 4 = a sample index outside the cloud, 16 = a rank's exchange segment overflowed (sharded search).  The sharded search decides
// on what EVERY rank reported, never on a rank's own state -- two ranks that disagreed would part ways before the next collective,
// and raw RCCL has no watchdog -- so a rank's findings travel in word 1 of its segment header and the merge kernel turns the
// gathered headers into three more bits, identical on every rank: kFlagShardRetry (some rank that had NOT launched the larger
// classes needs them), kFlagShardHard (some rank that had launched them still overflowed), kFlagSharded (a merge ran: the
// decision comes from these bits, the rank's own bit 0 is ignored).
constexpr int kFlagShardRetry = 32, kFlagShardHard = 64, kFlagSharded = 128, kFlagShardRetryHuge = 256;
// ... and two for a rank that took part in the call's collectives without doing its share (shard.hip, "no rank leaves alone"):
// kFlagShardPeerFailed (a rank's own failure: memory, a launch), kFlagShardPeerNoCloud (a rank holds no cloud) -- from the header
// bits kHdrRankFailed / kHdrRankNoCloud of its segment
constexpr int kFlagShardPeerFailed = 512, kFlagShardPeerNoCloud = 1024;
constexpr int kHdrRankFailed = 32, kHdrRankNoCloud = 64;
// word 1 of a segment header: an overflow of the capacity classes the rank had launched -- 1 with the larger classes off (level
// 0: a retry with them helps), 8 with them on (level 1: a retry with the 6144 class helps), 16 with that on too (level 2: hard)
// -- and 4 = bad sample index
__host__ __device__ inline int shard_header_word(int flags0, int class_level)
{
  return ((flags0 & 1) ? (class_level >= 2 ? 16 : (class_level == 1 ? 8 : 1)) : 0) | (flags0 & 4);
}

// ---- kernel launchers (defined in the .hip files) ----
int vox_stage1(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, int64_t size_left, int dense,
  const double workspace[6], double cell, hipStream_t st, int64_t cap_words, VoxDesc* host_desc, bool with_lattice);
int vox_stage2(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, double cell, int64_t n_words, hipStream_t st,
  VoxDesc* host_desc, bool with_lattice, int* cloud_off_out = nullptr);
// voxelize.hip's block popcount and one-block scan on a bitmap of the voxel bitmap's layout (sample_mask.hip: the eligibility
// bitmap): counts per 4096 words into blk, then their exclusive scan in place and the total
int vox_count_blocks(const unsigned* d_bitmap, int64_t n_blocks, int* d_blk, long long* d_total, hipStream_t st);
// sample_mask.hip: the masked sample list of a chain whose voxelisation is queued on st (include/agh.h, agh_localize_masked)
int sample_mask_stage(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, const uint8_t* d_mask, double cell, int64_t S,
  unsigned long long seed, int32_t* d_out, int32_t* h_out, long long* h_count, hipStream_t st);
// sample_labels.hip: the K sample lists of a labelled chain, S each, object after object (include/agh.h, agh_localize_labeled);
// the M_j go to c->h_label_counts
int sample_label_stage(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, const uint8_t* d_labels, int K, double cell,
  int64_t S, unsigned long long seed, int32_t* d_out, int32_t* h_out, hipStream_t st);
// ... in two parts, so that another source of the object sets shares the second: the label buffers (a bitmap of `words` words, n
// raw points, `groups` group counts), and the compaction of c->d_label_set into the K lists with their draw
constexpr int kLabelGroup = 256;  // voxels per work-group of the compaction: four waves
int ensure_label_buffers(Ctx* c, int64_t words, int64_t n, int64_t groups);
int label_compact_stage(Ctx* c, int64_t n, int K, bool any, int64_t S, unsigned long long seed, int32_t* d_out, int32_t* h_out,
  hipStream_t st);
// sample_cluster.hip: the same K lists with the object sets taken from the cloud itself (include/agh.h, agh_localize_clustered):
// the connected components of the voxels above a support plane; the parameters as the kernels take them
struct ClusterDev
{
  double plane[4], min_height, max_height, tolerance;
  float tol2;          // (float) (tolerance * tolerance): the bound of the float32 adjacency rule
  int32_t min_voxels;
};
// (d_cp: the record in device memory that a fitted chain's k_fit_finish writes -- the kernels read plane and bounds there, the
// host's cp serves min_voxels alone; nullptr: the record goes by value, as agh_localize_clustered*)
int sample_cluster_stage(Ctx* c, int64_t n, const ClusterDev& cp, int K, int64_t S, unsigned long long seed, int32_t* d_out,
  int32_t* h_out, hipStream_t st, const ClusterDev* d_cp = nullptr);
// plane_fit.hip: the support plane of a fitted chain (include/agh.h, agh_localize_clustered_fit), found on the voxelised cloud
// whose preprocessing is queued on st; *d_cp_out: the device record the cluster stage reads.  origin: camera 0's, in force
struct PlaneFitDev
{
  int32_t C, refine, min_inliers, pad;
  double threshold;
  unsigned long long seed;
  double origin[3];
};
constexpr int kPlaneFitMaxCandidates = 256;
struct PlaneFitBuffers  // the one device block of a context's fitted calls
{
  double planes[kPlaneFitMaxCandidates][4];
  int32_t idx[kPlaneFitMaxCandidates][3];
  unsigned counts[kPlaneFitMaxCandidates];
  unsigned long long sums[16];  // [0] n_refit, [1 .. 3] Sx Sy Sz, [4 .. 9] Sxx Sxy Sxz Syy Syz Szz
  ClusterDev record;
};
std::string plane_fit_params_fault(const agh_plane_fit_params& fp);
int plane_fit_stage(Ctx* c, int64_t n, const agh_plane_fit_params& fp, const ClusterDev& cp, hipStream_t st, const ClusterDev** d_cp_out);
inline ClusterDev cluster_dev(const agh_cluster_params& q)
{
  return ClusterDev{ { q.plane[0], q.plane[1], q.plane[2], q.plane[3] }, q.min_height, q.max_height, q.tolerance,
    (float) (q.tolerance * q.tolerance), q.min_voxels };
}
// the rules of one agh_cluster_params record (include/agh.h, agh_localize_clustered, 7): what is wrong with it, naming the field,
// or "" -- the single call's text as it is, a batch's behind "capture k: " (localize.hip)
std::string cluster_params_fault(const agh_cluster_params& cp);
// ... and on the C slots of a batch's bitmap (vb.slot_words words each): slot k's counts at blk + k * slot_words / 4096, not scanned
int vox_count_blocks_batch(const VoxBatch& vb, int C, const unsigned* d_bitmap, int* d_blk, hipStream_t st);
// What every sample stage of a batch chain is given (localize_batch.hip, batch_pass fills it once, behind the queued preprocessing
// vox_batch and grid build); the stages' own records below add what only they read.
struct BatchStageCommon
{
  VoxBatch vb;                      // the batch's capture table, descriptors and slot size
  int C = 0, L = 0;                 // captures; lists (C without a list per object)
  int64_t n_max = 0, n_tot = 0, S_tot = 0;  // the largest capture's raw points; all captures'; the samples of all lists
  double cell = 0.0;
  const uint8_t* code = nullptr;    // the per-point codes of all captures (VoxCapture::code_off)
  const unsigned* bitmap = nullptr; // the voxel bitmap slots
  const int* blk2 = nullptr;        // ... and their capture-local block prefixes
  const int* cloud_off = nullptr;   // the batch's device-side cloud offsets
  const BatchCapture* tab = nullptr;  // the chain's list table (soff, S, seed, capture, object)
  int32_t* d_out = nullptr;         // S_tot indices into the common voxel array (or kSampleSkip), for the search
  int32_t* h_out = nullptr;         // pinned: S_tot capture-local indices
};
// sample_mask.hip: the masked sample list of a batch chain (include/agh.h, agh_localize_batch_masked)
struct BatchMaskStage : BatchStageCommon
{
  const uint8_t* const* mask = nullptr;  // device table: capture k's mask, one byte per raw point, at any byte alignment
  unsigned* elig = nullptr;         // C eligibility slots of the voxel slots' layout
  int* eblk = nullptr;              // their block counts, then capture-local prefixes
  long long* total = nullptr;       // C: the M_k
  int32_t* list = nullptr;          // the E_k, capture k's at its code_off
  long long* h_total = nullptr;     // pinned: C counts M_k
};
int sample_mask_stage_batch(Ctx* c, const BatchMaskStage& m, hipStream_t st);
// sample_labels.hip: the sample lists of a labelled batch chain (include/agh.h, agh_localize_batch_labeled), one list per (capture,
// object); the label buffers are the context's (the single labelled chain's, grown); the M_l go to c->h_label_counts
struct LabelCapture  // the lists of a labelled batch, per capture: its objects and its first list among the call's
{
  int32_t K, first_list;
};
struct BatchLabelStage : BatchStageCommon
{
  const uint8_t* const* labels = nullptr;  // device table: capture k's labels, one byte per raw point, at any byte alignment
  const LabelCapture* lists = nullptr;     // device table, one per capture
};
int sample_label_stage_batch(Ctx* c, const BatchLabelStage& m, hipStream_t st);
// ... in two parts, as the single chain's: the compaction of c->d_label_set into the L lists with their draw, shared with
// sample_cluster.hip's batch stage, which fills the object sets from the clouds with one ClusterDev record per capture (and reads
// neither labels, codes nor bitmaps)
int label_compact_stage_batch(Ctx* c, const BatchLabelStage& m, bool any, hipStream_t st);
int sample_cluster_stage_batch(Ctx* c, const BatchLabelStage& m, const ClusterDev* cps, hipStream_t st);
// plane_fit.hip's batch stage (include/agh.h, agh_localize_batch_clustered_fit), queued behind the upload of the ClusterDev table
// and in front of sample_cluster_stage_batch: capture k's plane, found on its own voxels with fps[k], goes into cps[k].plane
struct BatchFitStage : BatchStageCommon
{
  const PlaneFitDev* fps = nullptr; // device table: capture k's parameters and camera 0's origin in force for it
  PlaneFitBuffers* fbs = nullptr;   // device: a block per capture
  ClusterDev* cps = nullptr;        // device table of the cluster stage: the plane of record k is written
  agh_plane_fit_result* h_results = nullptr;  // pinned: C records
};
int plane_fit_stage_batch(Ctx* c, const BatchFitStage& m, hipStream_t st);
int vox_batch(const VoxBatch& vb, int C, int64_t nb_max, int64_t n_max, bool any_finite_scan, double cell, bool probe,
  unsigned* bitmap, int* blk, int* blk2, uint8_t* code, float* out_xyz, int32_t* out_cam, int* cloud_off, hipStream_t st,
  unsigned* pruned = nullptr, const agh_voxel_filter_params* filter = nullptr);
// host mirror of the handle search's results (pinned memory of the context; all nullptr / 0: none)
struct HandleMirror
{
  agh_handle* handles;
  int handle_cap;
  int* idx;
  int idx_cap;
  int* counts;  // [0] handles, [1] inlier indices, [2] error, [3] the batched walk declined and no sequential kernel was launched
};
int handle_search(Ctx* c, int64_t H, double x1, double x2, int min_inliers, double min_length, hipStream_t st,
  const HandleMirror& hm, bool with_sequential, const int* d_H = nullptr);
// the handle search's device buffers (the context's, or agh_localize_batch's slices of n_lists lists)
struct HandleBufs
{
  agh_hypothesis* hands;
  unsigned long long* bits;
  int* rowcnt;
  int* first;
  int* n;
  int* idx;
  int* counts;  // HandleCounts (four ints) per list
  int* tmp;
  agh_handle* handles;
};
// agh_localize_batch: n_lists lists of at most H hands each, list k in slot k of `slot` hands of every buffer (the pair matrix:
// slot x ceil(slot / 64) words per list); d_H[k] its count on the device.  The host mirror: list k's handles and inlier indices at
// k x hm.handle_cap (hm.idx_cap must equal it), its counts at k x host_counts_stride ints.
int handle_search_batch(const HandleBufs& b, int n_lists, int64_t slot, int64_t H, double x1, double x2, int min_inliers,
  double min_length, hipStream_t st, const HandleMirror& hm, int host_counts_stride, bool with_sequential, const int* d_H);
// agh_localize_batch: the hand lists of several captures side by side, one per blockIdx.y, each in a slice of every buffer at these
// element strides (all 0 and a grid of one row: the single list of agh_find_handles / agh_localize).  counts and d_H are arrays
// with one entry per capture.  (handles.hip's kernels and handle_rank.hip's)
struct HandleSlots
{
  int64_t hands;     // hands, rowcnt, h_first, h_n, inlier_idx, tmp, the device-side handles
  int64_t bits;      // the pair matrix
  int64_t host;      // host_idx and the host-side handles
  int host_counts;   // host_counts
};
#define AGH_HANDLE_SLICE(p, stride)      \
  do                                     \
  {                                      \
    if (p)                               \
      p += (int64_t) blockIdx.y * (stride); \
  } while (0)
struct HandleCounts
{
  int n_handles, n_idx, error;
  int sequential;  // set by k_handle_batch when it declines (a row longer than kMaxRow, two waves' worth): k_handle_greedy runs
};
// ---- agh_set_handle_ranking (handle_rank.hip; DESIGN.md, "Handle ranking") ----
// What a chain's compaction writes beside the kept hands when a ranking is set: for output position k the margin -sums[src[k]]
// (0.0 without a classifier: sums null), to a device array and to its pinned mirror.  out null: nothing (every chain without one).
struct MarginOut
{
  const double* sums;
  double* out;
  double* host;
  int64_t stride, host_stride;  // a batch's lists: list l at l x stride (the handle search's slots)
};
// the chain's lists for k_handle_rank, queued behind k_handle_build on st: no-op unless handle_rank_prepare saw a ranking set
int handle_rank_stage(Ctx* c, const HandleBufs& b, int n_lists, int64_t slot, const HandleMirror& hm, int host_counts_stride,
  hipStream_t st);
// the buffers for n_lists lists of at most `slot` hands (host mirror: host_slot), made or regrown if a ranking is set; *m = what the
// compaction writes (out null if none is set).  Called where a chain queues its compaction.
int handle_rank_prepare(Ctx* c, int n_lists, int64_t slot, int64_t host_slot, bool classify, MarginOut* m);
// a chain's end: lists = 0 forgets the last chain's; else list l's n_kept[l] hands, for the three getters
void handle_rank_collect(Ctx* c, int lists, const int64_t* n_kept);
// the rule a set ranking adds to a chain's arguments: w_margin != 0 needs the classifier
int handle_rank_check(Ctx* c, const char* who, bool classify);
void handle_rank_release(Ctx* c);
int grid_build(Ctx* c, hipStream_t st);
int taubin_frames(Ctx* c, const int32_t* d_samples, int64_t S, double radius, agh_frame* d_frames, int32_t* d_nt,
  bool write_normals, hipStream_t st);
int taubin_moments_eigen(Ctx* c, const int32_t* d_samples, int64_t S, double radius, int32_t* d_nt, hipStream_t st,
  bool with_draw_offsets = false);
int taubin_frame_stage(Ctx* c, const int32_t* d_samples, int64_t S, double radius, agh_frame* d_frames, int32_t* d_nt,
  bool write_normals, hipStream_t st, bool draw_offsets_done = false);
int hand_sweep(Ctx* c, const int32_t* d_samples, int64_t S, bool use_normals, hipStream_t st);
int ball_counts(Ctx* c, int64_t S, hipStream_t st);  // d_nh of the last call's samples (agh_get_neighbor_counts)
int compact_hypotheses(Ctx* c, int64_t S, agh_hypothesis* d_out, int64_t cap, int64_t* d_nout, hipStream_t st,
  int64_t* d_hdr_flags = nullptr);  // d_hdr_flags: sharded search, slices of at most 65536 samples (see shard.hip)
// ws: the workspace of a chain with filters_boundaries (the hypotheses near its faces are labelled 0 and not classified), or null
// drop: the hand drop stage's bytes, or null: a dropped hypothesis is labelled 0 and not classified either
int hog_svm(Ctx* c, int64_t n_hyp_cap, uint8_t* d_keep, hipStream_t st, const double* ws = nullptr, const uint8_t* drop = nullptr);
// hand_drop.hip: the set tests queued on st behind the search (the records of d_out_own, *d_nout of them, at most `bound`); without
// one nothing is allocated or launched.  tab / n_lists: the batch chain's list table (null: the one list of the single chain).
HandDropView hand_drop_stage(Ctx* c, int64_t bound, const BatchCapture* tab, int n_lists, hipStream_t st);
// a chain's end: its lists and their hypotheses, for the two counts getters (0 lists: nothing collected)
void hand_drop_collect(Ctx* c, int lists, const int64_t* hyp);
HandDropCounts hand_drop_counts(const Ctx* c, int k);
void hand_drop_release(Ctx* c);
void depth_fuse_release(Ctx* c);
// the two tests, each launched only if its own setting is set.  has_drop: the bytes are written already (the kernel skips the
// dropped hands); else it writes every byte itself
int hand_filter_launch(Ctx* c, int64_t bound, const BatchCapture* tab, int n_lists, hipStream_t st);
int hand_clearance_launch(Ctx* c, int64_t bound, const BatchCapture* tab, int n_lists, hipStream_t st, bool has_drop);
// the views of a depth chain's images, as the chain's deprojection read them (depth.hip), kept while a filter with view_on is set
void hand_filter_keep_views(Ctx* c, const agh_depth_image* images, const int32_t* n_images, int C, const uint8_t* const* data,
  const int64_t* stride);
// the rules a set filter adds to a chain's arguments: view_on needs depth images with orthonormal poses (C captures, capture k's
// images the next n_images[k] of the flat array; the text names the image, and for C > 1 its capture)
int hand_filter_check(Ctx* c, const char* who, const agh_depth_image* images, const int32_t* n_images, int C, bool has_depth);
int hog_images(Ctx* c, const uint32_t* d_images, const int32_t* d_order, int64_t n, float* d_desc, hipStream_t st);
int svm_predict_general(Ctx* c, const float* d_desc, int64_t cap, uint8_t* d_keep, hipStream_t st,
  const BoundaryBox& box = BoundaryBox{}, const uint8_t* drop = nullptr);
int svm_predict_images(Ctx* c, const float* d_desc, int64_t n, uint8_t* d_keep, double* d_sums, hipStream_t st);
int svm_predict_desc(Ctx* c, const float* d_desc, int64_t cap, const int64_t* d_nhyp, agh_hypothesis* d_out, uint8_t* d_keep,
  double* d_sums, hipStream_t st, const BoundaryBox& box = BoundaryBox{}, const uint8_t* drop = nullptr);
int svm_load_general(Ctx* c, int kernel_type, const float* sv, int n_sv, const double* alpha, double rho);
void hog_tables_host(HogTablesDev* t);
int64_t selftest_math(Ctx* c, int64_t n, uint64_t seed);

void timing_mark(Ctx* c, const char* name, hipStream_t st);
hipEvent_t timing_next_event(Ctx* c, const char* name);
bool timing_launch_events(Ctx* c, const char* name, hipEvent_t* start, hipEvent_t* stop);
void timing_begin(Ctx* c, hipStream_t st);
int32_t next_epoch();
int ensure_call_buffers(Ctx* c, int64_t S);
int ensure_host_staging(Ctx* c, int64_t samples, int64_t records);
constexpr int64_t kPinHeaderBytes = 256;  // pinned staging of the host-buffer entry points: [header | sample indices | records]
constexpr int kPinMaskCount = 8;  // int64 word of that header that a masked chain writes M into (words 0 and 1: HostMirror::hdr)
// (re)allocation of one of the context's device buffers
template <typename T>
inline int dev_alloc(Ctx* c, T** p, size_t count)
{
  if (*p)
  {
    (void) hipFree(*p);
    *p = nullptr;
  }
  const hipError_t e = hipMalloc((void**) p, (count > 0 ? count : 1) * sizeof(T));
  if (e != hipSuccess)
  {
    c->err = std::string("hipMalloc: ") + hipGetErrorString(e);
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}
// the voxel bitmap of the context, and the voxel filter's second one with it (the next voxelisation sizes new ones)
inline void drop_vox_bitmaps(Ctx* c)
{
  (void) hipFree(c->d_vox_bitmap);
  (void) hipFree(c->d_vox_pruned);
  c->d_vox_bitmap = c->d_vox_pruned = nullptr;
  c->vox_bitmap_cap = c->vox_pruned_cap = 0;
}
int ensure_clouds(Ctx* c, int C);
int ensure_draws(Ctx* c, int64_t count, hipStream_t st);
int normals_pass(Ctx* c, int64_t p0, int64_t p1, hipStream_t st);
void comm_release(Ctx* c);
void plane_release(Ctx* c);
void localize_batch_release(Ctx* c);

// ---- device helpers ----
#if defined(__HIPCC__)

// Localization::filterHands' test (localization.cpp:374-378) on a record's own doubles: true iff some face k of the box is
// closer than MIN_DIST, |surface[k / 2] - ws[k]| < 0.02, strictly.  Exact IEEE (no contraction, no fast math: the build's
// flags), so it agrees with the host filterHands bit for bit; a NaN surface compares false everywhere and is kept, as there.
__device__ __forceinline__ bool near_workspace_boundary(const double* surface, const double* ws)
{
  bool near = false;
#pragma unroll
  for (int k = 0; k < 6; k++)
    near |= fabs(surface[k >> 1] - ws[k]) < kBoundaryMinDist;
  return near;
}

// The body of k_compact_kept (localize.hip) and k_compact_kept_batch (localize_batch.hip), one work-group of 1024 threads: the
// records of in[r0, r1) that are kept -- svm_keep if use_keep; not near a face of ws if filters; not dropped by the hand filter if
// drop (its bytes, indexed as `in`; null: none) -- leave in list order (an ordered
// compaction is a scan: a ballot, sixteen wave sums, a carry), each as one 160-byte run, ten threads of sixteen bytes, to out and,
// below host_cap, to host_out (pinned; null: none), `sample` less sample_base.  dev_cap bounds what is written, not what is
// counted; the count is returned.  LDS of the caller: src[kCompactList] (position in the output -> position in the input),
// wsum[16], carry.  marg (agh_set_handle_ranking; null: none): for output position k the value -sums[src[k]], to marg and, below
// host_cap, to marg_host.
constexpr int kCompactList = 8192;  // (the handle search takes no more)
__device__ __forceinline__ int compact_kept_records(const agh_hypothesis* __restrict__ in, int64_t r0, int64_t r1, int use_keep,
  int filters, const double* ws, int* src, int* wsum, int* carry, agh_hypothesis* __restrict__ out, int dev_cap,
  agh_hypothesis* __restrict__ host_out, int host_cap, int sample_base, const uint8_t* __restrict__ drop,
  const double* __restrict__ sums = nullptr, double* __restrict__ marg = nullptr, double* __restrict__ marg_host = nullptr)
{
  static_assert(sizeof(agh_hypothesis) == 160 && offsetof(agh_hypothesis, sample) == 8 * 16,
    "ten 16-byte parts; sample is the first word of the ninth");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0)
    *carry = 0;
  __syncthreads();
  for (int64_t b0 = r0; b0 < r1; b0 += 1024)
  {
    const int64_t i = b0 + tid;
    const bool keep = i < r1 && (!use_keep || in[i].svm_keep != 0) && !(filters && near_workspace_boundary(in[i].surface, ws)) &&
                      !(drop && drop[i]);
    const unsigned long long m = __ballot(keep);
    if (lane == 0)
      wsum[wave] = __popcll(m);
    __syncthreads();
    int base = *carry, tot = 0;
    for (int w = 0; w < 16; w++)
    {
      base += w < wave ? wsum[w] : 0;
      tot += wsum[w];
    }
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && pos < kCompactList)
      src[pos] = (int) i;
    __syncthreads();
    if (tid == 0)
      *carry += tot;
    __syncthreads();
  }
  const int K = *carry, kw = min(K, min(dev_cap, kCompactList));
  for (int t = tid; t < kw * 10; t += 1024)
  {
    const int k = t / 10, part = t - 10 * k;
    const uint4 raw = reinterpret_cast<const uint4*>(in + src[k])[part];
    const uint4 v = make_uint4(part == 8 ? (unsigned) ((int) raw.x - sample_base) : raw.x, raw.y, raw.z, raw.w);
    reinterpret_cast<uint4*>(out + k)[part] = v;
    if (host_out && k < host_cap)
      reinterpret_cast<uint4*>(host_out + k)[part] = v;
  }
  // agh_set_handle_ranking: the kept hands' margins, minus the classifier's decision sums (0.0 without a classifier)
  if (marg)
    for (int k = tid; k < kw; k += 1024)
    {
      const double g = sums ? -sums[src[k]] : 0.0;
      marg[k] = g;
      if (marg_host && k < host_cap)
        marg_host[k] = g;
    }
  return K;
}

__device__ __forceinline__ unsigned enc_float(float f)
{
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_float(unsigned u)
{
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// Voxel index along one axis exactly as localization.cpp:288: floor((double(p) - min) / cell).
__device__ __forceinline__ long long vox_index(float p, double mn, double cell)
{
  return (long long) floor(((double) p - mn) / cell);
}
// ... and the bit of a kept point of camera c in the lattice of its camera: x-major, z-fastest (voxelize.hip)
__device__ __forceinline__ unsigned long long vox_bit(const VoxDesc* d, int c, const float* p, double cell)
{
  const unsigned long long ix = (unsigned long long) vox_index(p[0], d->mn[c][0], cell);
  const unsigned long long iy = (unsigned long long) vox_index(p[1], d->mn[c][1], cell);
  const unsigned long long iz = (unsigned long long) vox_index(p[2], d->mn[c][2], cell);
  return (ix * (unsigned long long) d->dim[c][1] + iy) * (unsigned long long) d->dim[c][2] + iz;
}

// The voxels of the cloud (device side; none after a voxeliser's error, whose repeat runs the stage again): n = the raw points.
__device__ __forceinline__ int64_t label_voxels(const VoxDesc* d, int64_t n)
{
  return d->error ? 0 : min((int64_t) (d->n_vox[0] + d->n_vox[1]), n);
}

__device__ __forceinline__ int cell_coord(const GridDesc& g, double v, int a)
{
  // clamped in double, BEFORE the conversion: a finite point 1e30 m outside a kept descriptor is 5e31 cells away, which no int
  // holds (the conversion of such a value is undefined).  A NaN ends in cell 0 (fmax returns its other argument).
  const double f = floor((v - g.mn[a]) * g.inv_cell);
  return (int) fmin(fmax(f, 0.0), (double) (g.dim[a] - 1));
}

// The view of the grid of cloud k / of the cloud that holds point p (uniform per work-group: scalar loads).
__device__ __forceinline__ GridView grid_of_cloud(GridView gv, int k)
{
  gv.desc += k;
  gv.cell_start += (int64_t) k * kCellStride;
  return gv;
}
__device__ __forceinline__ int cloud_of_point(const GridView& gv, int p)
{
  // (p wave-uniform; the offsets of the <= 64 clouds are compared a lane each: one load and a ballot, where a loop over the clouds
  // was a chain of dependent scalar loads -- 0.6 us per work-group with a batch of eight)
  if (gv.n_clouds == 1)
    return 0;
  const int lane = threadIdx.x & 63;
  const int off = (lane >= 1 && lane < gv.n_clouds) ? gv.cloud_off[lane] : 0x7fffffff;
  return __popcll(__ballot(p >= off));
}

// Squared distance exactly as FLANN's L2_Simple<float> accumulates it (see oracle a2): ((0+dx*dx)+dy*dy)+dz*dz.
__device__ __forceinline__ float flann_d2(float qx, float qy, float qz, float px, float py, float pz)
{
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  float d2 = __fmul_rn(dx, dx);
  d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
  d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
  return d2;
}

// Inclusive sum scan over the 64 lanes of a wave by DPP: row_shr 1, 2, 4, 8 inside each 16-lane row (a lane without a source
// adds zero), then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3 -- six v_add_u32_dpp, where a
// __shfl_up loop is six dependent ds_bpermute round trips through the LDS crossbar.
__device__ __forceinline__ int wave_incl_scan_i32(int v)
{
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}

// The value lane (l ^ O) holds, for a double, without the LDS crossbar: v_permlane32_swap / v_permlane16_swap (gfx950) for
// O = 32 / 16, DPP moves inside a 16-lane row for O = 8 (row_ror:8), 4 (row_shl:4 into banks 0 and 2, row_shr:4 into banks 1 and
// 3), 2 and 1 (quad_perm).  A __shfl_xor of a double is two ds_bpermute round trips (~130 cycles of latency in a dependent
// butterfly); these are two to four VALU moves.
template <int O>
__device__ __forceinline__ int xor_partner_i32(int x)
{
  static_assert(O == 32 || O == 16 || O == 8 || O == 4 || O == 2 || O == 1, "a single bit of the lane index");
  if (O == 32)
  {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);  // r[0] = {x[0..31], x[0..31]}, r[1] = {x[32..63], x[32..63]}
    return (threadIdx.x & 32) ? (int) r[0] : (int) r[1];
  }
  if (O == 16)
  {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);  // r[0] = rows {0, 0, 2, 2}, r[1] = rows {1, 1, 3, 3}
    return (threadIdx.x & 16) ? (int) r[0] : (int) r[1];
  }
  if (O == 8)
    return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false);  // row_ror:8
  if (O == 4)
  {
    const int t = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xf, 0x5, false);  // row_shl:4 -> lanes 0-3, 8-11 of a row take l + 4
    return __builtin_amdgcn_update_dpp(t, x, 0x114, 0xf, 0xa, false);         // row_shr:4 -> lanes 4-7, 12-15 take l - 4
  }
  if (O == 2)
    return __builtin_amdgcn_update_dpp(0, x, 0x4e, 0xf, 0xf, false);  // quad_perm [2, 3, 0, 1]
  return __builtin_amdgcn_update_dpp(0, x, 0xb1, 0xf, 0xf, false);    // quad_perm [1, 0, 3, 2]
}
template <int O>
__device__ __forceinline__ double xor_partner_f64(double x)
{
  return __hiloint2double(xor_partner_i32<O>(__double2hiint(x)), xor_partner_i32<O>(__double2loint(x)));
}
// The butterfly of the oracle's LaneSum64: v + v(l ^ 32), then ^ 16, 8, 4, 2, 1; every lane ends with the same total.
__device__ __forceinline__ double wave_allsum_f64(double v)
{
  v = v + xor_partner_f64<32>(v);
  v = v + xor_partner_f64<16>(v);
  v = v + xor_partner_f64<8>(v);
  v = v + xor_partner_f64<4>(v);
  v = v + xor_partner_f64<2>(v);
  v = v + xor_partner_f64<1>(v);
  return v;
}

// Wave-wide integer sum, the same on every lane.
__device__ __forceinline__ int wave_allsum_i32(int v)
{
  v += xor_partner_i32<32>(v);
  v += xor_partner_i32<16>(v);
  v += xor_partner_i32<8>(v);
  v += xor_partner_i32<4>(v);
  v += xor_partner_i32<2>(v);
  v += xor_partner_i32<1>(v);
  return v;
}

// Row table of one ball query, built cooperatively in LDS.
struct RowTable
{
  int begin[kMaxRows];
  int prefix[kMaxRows + 1];
  int seg_row[64];  // the row that holds flat candidate 128 j, for the first 64 segments of 128 candidates (FlatRows)
  int nrows;
  int total;
  int bad;
};

// Fill rt for the ball (q, rpad).  Must be called by all threads of the block; ends with a barrier.
// SLAB: the caller only wants the points p of the ball with |a . (p - q)| < hh (the hand sweep's crop along the hand axis,
// rotating_hand.cpp:37-51, keeps a 2 hh thick slab of a 2 r ball: about a fifth of its points).  Every row is then clipped
// to the part of its chord that can hold such a point -- by interval arithmetic over the row's (y, z) cell, widened by
// kSlabMargin, which is orders of magnitude above the rounding of the caller's own test (the float32 subtraction it
// starts from is off by < 1e-8 m) -- and rows the slab misses are dropped: half the candidates and half the row segments
// of the plain ball at C2.  The caller's exact test still decides every point; this only prunes what it never accepts.
constexpr double kSlabMargin = 1e-6;
// `gpre`: the query's grid descriptor if the caller has loaded it already (so that the load could be issued before other
// loads the caller had to wait for).
template <bool SLAB = false>
__device__ __forceinline__ void build_rows(const GridView& gv, float qx, float qy, float qz, double rpad, RowTable& rt,
  const double* slab_axis = nullptr, double slab_hh = 0.0, const GridDesc* gpre = nullptr)
{
  const GridDesc& g = gpre ? *gpre : *gv.desc;
  const int tid = threadIdx.x;
  const int lx = cell_coord(g, (double) qx - rpad, 0), hx = cell_coord(g, (double) qx + rpad, 0);
  const int ly = cell_coord(g, (double) qy - rpad, 1), hy = cell_coord(g, (double) qy + rpad, 1);
  const int lz = cell_coord(g, (double) qz - rpad, 2), hz = cell_coord(g, (double) qz + rpad, 2);
  const int ny = hy - ly + 1, nz = hz - lz + 1;
  const int nrows = ny * nz;
  if (tid == 0)
  {
    rt.nrows = nrows;
    rt.bad = nrows > kMaxRows;
  }
  if (nrows <= kMaxRows)
  {
    for (int t = tid; t < nrows; t += blockDim.x)
    {
      // (t / ny for ny <= 9, t < 128, without the ~40-instruction integer division: exact in float)
      const int tq = (int) (((float) t + 0.5f) * (1.0f / (float) ny));
      const int cy = ly + (t - tq * ny), cz = lz + tq;
      // distance from q to the row's (y,z) slab; rows that cannot touch the ball are skipped.  A border row or layer whose
      // face is open (points outside the descriptor's box, clamped into it: a kept descriptor that missed the cloud) reaches
      // to infinity on its outer side.
      const double y0 = g.mn[1] + cy * g.cell, z0 = g.mn[2] + cz * g.cell;
      double ylo = y0, yhi = y0 + g.cell, zlo = z0, zhi = z0 + g.cell;
      bool open_row = false;
      if (g.open)  // (uniform: only after a build that missed)
      {
        const bool oy0 = cy == 0 && (g.open & 4u), oy1 = cy == g.dim[1] - 1 && (g.open & 8u);
        const bool oz0 = cz == 0 && (g.open & 16u), oz1 = cz == g.dim[2] - 1 && (g.open & 32u);
        ylo = oy0 ? -INFINITY : ylo;
        yhi = oy1 ? INFINITY : yhi;
        zlo = oz0 ? -INFINITY : zlo;
        zhi = oz1 ? INFINITY : zhi;
        open_row = oy0 | oy1 | oz0 | oz1;
      }
      const double dy = fmax(fmax(ylo - (double) qy, (double) qy - yhi), 0.0);
      const double dz = fmax(fmax(zlo - (double) qz, (double) qz - zhi), 0.0);
      int b = 0, len = 0;
      const double rem = rpad * rpad - (dy * dy + dz * dz);
      if (rem >= 0.0)
      {
        // the ball's chord along x at this row: a point of the row within rpad of q has |x - qx| <= sqrt(rem)
        // (dy, dz are the smallest possible offsets), so only the cells under the chord are candidates -- about a
        // third fewer than the bounding box's
        const double xr = sqrt(rem);
        double xlo = (double) qx - xr, xhi = (double) qx + xr;
        bool keep = true;
        if (SLAB && !open_row)  // (an open row is not clipped to the slab: its (y, z) extent is unbounded)
        {
          // a_y (y - qy) + a_z (z - qz) over the row's cell lies in [L, U]; a point passes only if a_x (x - qx) + that is
          // inside (-hh, hh), i.e. a_x (x - qx) in (-hh - U, hh - L)
          const double ya = (y0 - kSlabMargin) - (double) qy, yb = (y0 + g.cell + kSlabMargin) - (double) qy;
          const double za = (z0 - kSlabMargin) - (double) qz, zb = (z0 + g.cell + kSlabMargin) - (double) qz;
          const double ey0 = slab_axis[1] * ya, ey1 = slab_axis[1] * yb, ez0 = slab_axis[2] * za, ez1 = slab_axis[2] * zb;
          const double L = fmin(ey0, ey1) + fmin(ez0, ez1), U = fmax(ey0, ey1) + fmax(ez0, ez1);
          const double lo_n = (-1.0 * (slab_hh + kSlabMargin)) - U, hi_n = (slab_hh + kSlabMargin) - L;
          const double ax = slab_axis[0];
          if (fabs(ax) > 1e-9)
          {
            const double inv_ax = 1.0 / ax;  // (one division instead of two: these bounds only prune, with kSlabMargin to spare)
            const double b1 = lo_n * inv_ax, b2 = hi_n * inv_ax;
            xlo = fmax(xlo, ((double) qx + fmin(b1, b2)) - kSlabMargin);
            xhi = fmin(xhi, ((double) qx + fmax(b1, b2)) + kSlabMargin);
            keep = xlo <= xhi;
          }
          else  // the slab contains the x direction (|a_x (x - qx)| < 1e-9 * 2 r): the row is inside or outside as a whole
            keep = (lo_n < 0.0) & (hi_n > 0.0);
          keep = keep | !(L == L && U == U);  // a NaN axis prunes nothing
        }
        if (keep)
        {
          const int lxr = max(lx, cell_coord(g, xlo, 0)), hxr = min(hx, cell_coord(g, xhi, 0));
          const int base = (cz * g.dim[1] + cy) * g.dim[0];
          b = gv.cell_start[base + lxr];
          len = hxr >= lxr ? gv.cell_start[base + hxr + 1] - b : 0;
        }
      }
      rt.begin[t] = b;
      rt.prefix[t + 1] = len;
    }
  }
  __syncthreads();
  if (tid < 64)  // wave 0: inclusive scan of the (<= 128) row lengths, two per lane -- and the rows without candidates are
  {              // squeezed out of the table (the walks then never meet an empty row): a second scan, of the non-empty flags
    const int nr = rt.bad ? 0 : nrows;
    const int v0 = tid < nr ? rt.prefix[tid + 1] : 0;
    const int v1 = (64 + tid) < nr ? rt.prefix[64 + tid + 1] : 0;
    const int b0 = tid < nr ? rt.begin[tid] : 0;
    const int b1 = (64 + tid) < nr ? rt.begin[64 + tid] : 0;
    const int f0 = v0 > 0 ? 1 : 0, f1 = v1 > 0 ? 1 : 0;
    int i0 = wave_incl_scan_i32(v0), i1 = wave_incl_scan_i32(v1), c0 = wave_incl_scan_i32(f0), c1 = wave_incl_scan_i32(f1);
    i1 += __builtin_amdgcn_readlane(i0, 63);  // (a v_readlane, where __shfl is a ds_bpermute round trip)
    c1 += __builtin_amdgcn_readlane(c0, 63);
    // (all reads of the table above precede these writes in the wave's program order; a row only moves down)
    if (f0)
    {
      rt.begin[c0 - 1] = b0;
      rt.prefix[c0] = i0;
      for (int jj = (i0 - v0 + 127) >> 7; (jj << 7) < i0 && jj < 64; jj++)  // the segment starts inside this row (mostly none or one)
        rt.seg_row[jj] = c0 - 1;
    }
    if (f1)
    {
      rt.begin[c1 - 1] = b1;
      rt.prefix[c1] = i1;
      for (int jj = (i1 - v1 + 127) >> 7; (jj << 7) < i1 && jj < 64; jj++)
        rt.seg_row[jj] = c1 - 1;
    }
    const int tot = __builtin_amdgcn_readlane(i1, 63), nkept = __builtin_amdgcn_readlane(c1, 63);  // lanes past nr hold zeros, so lane 63 of the second half has the totals
    if (tid == 0)
    {
      rt.prefix[0] = 0;
      rt.total = tot;
      rt.nrows = nkept;
    }
  }
  __syncthreads();
}

// Candidate j of the query -> position in the sorted array, for a thread whose j only grows: r is its row cursor.
__device__ __forceinline__ int row_advance(const RowTable& rt, int j, int& r)
{
  while (r + 1 < rt.nrows && j >= rt.prefix[r + 1])  // (bounded: a cursor can never leave the table)
    r++;
  return rt.begin[r] + (j - rt.prefix[r]);
}

// Candidate j of the query -> position in the sorted array (binary search).
__device__ __forceinline__ int row_lookup(const RowTable& rt, int j)
{
  int lo = 0, hi = rt.nrows;  // find the largest r with prefix[r] <= j
  while (hi - lo > 1)
  {
    const int mid = (lo + hi) >> 1;
    if (rt.prefix[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  return rt.begin[lo] + (j - rt.prefix[lo]);
}

// The candidates of a ball query as ONE run of `total` flat indices, walked in segments of 128 (lane: flat index
// 128 j + lane and 128 j + 64 + lane).  A row-per-wave walk leaves a third of the lanes without a candidate (a slab row of
// the hand search holds 87 candidates on average, a Taubin row 83) and gives the waves unequal numbers of rows; flat
// segments are full except the last, and wave w takes segments w, w + 4, ... .  The row table lives in lane registers
// (lane k: rows k and k + 64) and is read with v_readlane at wave-uniform indices, so finding a segment's rows costs no LDS
// round trip: a scalar loop over the row boundaries inside the segment and two selects per boundary and lane.
struct FlatRows
{
  int pre_lo, pre_hi;  // prefix[k + 1], prefix[k + 65]: the flat index at which row k (k + 64) ENDS
  int adj_lo, adj_hi;  // begin[k] - prefix[k] (rows k, k + 64): position in the sorted array = flat index + adj
  int seg_v;           // lane j: the first row of segment j (j < 64)
  int nrows, total;

  __device__ __forceinline__ void init(const RowTable& rt, int lane)
  {
    nrows = rt.nrows;
    total = rt.total;
    pre_lo = lane < nrows ? rt.prefix[lane + 1] : total;
    pre_hi = lane + 64 < nrows ? rt.prefix[lane + 65] : total;
    adj_lo = lane < nrows ? rt.begin[lane] - rt.prefix[lane] : 0;
    adj_hi = lane + 64 < nrows ? rt.begin[lane + 64] - rt.prefix[lane + 64] : 0;
    seg_v = (lane << 7) < total ? rt.seg_row[lane] : 0;
  }
  __device__ __forceinline__ int row_end(int r) const  // r wave-uniform; (two reads and a scalar select: no branch)
  {
    const int a = __builtin_amdgcn_readlane(pre_lo, r & 63), b = __builtin_amdgcn_readlane(pre_hi, r & 63);
    return r < 64 ? a : b;
  }
  __device__ __forceinline__ int row_adj(int r) const
  {
    const int a = __builtin_amdgcn_readlane(adj_lo, r & 63), b = __builtin_amdgcn_readlane(adj_hi, r & 63);
    return r < 64 ? a : b;
  }
  __device__ __forceinline__ int segments() const { return (total + 127) >> 7; }
  // Segment j (wave-uniform; r0 = the wave's row cursor, which only grows with j): positions of the lane's two candidates
  // in the sorted array and whether it has them.
  __device__ __forceinline__ void locate(int j, int& r0, int lane, int& a0, int& a1, bool& h0, bool& h1) const
  {
    // (j and r0 derive from the wave's index, i.e. from threadIdx: tell the compiler they are wave-uniform, or the two
    // loops below become exec-masked vector loops)
    j = __builtin_amdgcn_readfirstlane(j);
    r0 = __builtin_amdgcn_readfirstlane(r0);
    const int tot = __builtin_amdgcn_readfirstlane(total), nrows = __builtin_amdgcn_readfirstlane(this->nrows);
    const int start = j << 7, end = min(start + 128, tot);
    const int i0 = start + lane, i1 = i0 + 64;
    h0 = i0 < tot;
    h1 = i1 < tot;
    if (start >= tot)  // (the read-ahead past the last segment)
    {
      a0 = a1 = 0;
      return;
    }
    if (j < 64)  // the segment's first row comes from the table build_rows left; later segments walk on from the cursor
      r0 = __builtin_amdgcn_readlane(seg_v, j);
    else
      while (r0 + 1 < nrows && row_end(r0) <= start)
        r0++;
    int adj = row_adj(r0);
    a0 = adj;
    a1 = adj;
    for (int r = r0; r + 1 < nrows;)  // the row boundaries inside the segment (build_rows leaves no empty rows)
    {
      const int b = row_end(r);
      if (b >= end)
        break;
      r++;
      adj = row_adj(r);
      a0 = i0 >= b ? adj : a0;
      a1 = i1 >= b ? adj : a1;
    }
    a0 += i0;
    a1 += i1;
  }
};

// Cyclic Jacobi of a symmetric 3x3 (oracle jacobi_sym<3>): one lane, the oracle's operation order.
__device__ inline void jacobi3_serial(double A[3][3], double V[3][3], double d[3])
{
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++)
  {
    double off = 0.0;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++)
        off += A[p][q] * A[p][q];
    if (off == 0.0)
      break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++)
      {
        const double apq = A[p][q];
        if (apq == 0.0)
          continue;
        const double app = A[p][p], aqq = A[q][q];
        const double aabs = fabs(apq);
        if (sweep > 3 && (fabs(app) + aabs == fabs(app)) && (fabs(aqq) + aabs == fabs(aqq)))
        {
          A[p][q] = 0.0;
          A[q][p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0)
          t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        A[p][p] = app - t * apq;
        A[q][q] = aqq + t * apq;
        A[p][q] = 0.0;
        A[q][p] = 0.0;
        for (int k = 0; k < 3; k++)
        {
          if (k == p || k == q)
            continue;
          const double akp = A[k][p], akq = A[k][q];
          const double np_ = c * akp - s * akq;
          const double nq_ = s * akp + c * akq;
          A[k][p] = np_;
          A[p][k] = np_;
          A[k][q] = nq_;
          A[q][k] = nq_;
        }
        for (int k = 0; k < 3; k++)
        {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < 3; i++)
    d[i] = A[i][i];
}

#endif  // __HIPCC__

}  // namespace agh

struct agh_ctx
{
  agh::Ctx c;
};

// api.hip's stages as localize.hip queues them
int preprocess_device_impl(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, int64_t size_left, int dense,
  const double workspace[6], double cell_size, int64_t* n_voxels_out, void* hip_stream, bool defer_count, bool* deferred);
bool handle_thresholds(double* x1, double* x2);
int ensure_handle_buffers(agh::Ctx* c, int64_t n_hands);
int flags_to_status(agh::Ctx* c, const int32_t* flags);
// localize.hip's pieces that localize_batch.hip runs too: the staging of the next chain's captures, and the end of a chain behind
// its synchronisation (the capacity-class repeat, the sequential-walk repeat, the limits)
int stage_captures(agh_ctx* ctx, const char* who, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n, int C,
  bool as_batch);
// depth.hip: the third source kind of the localize chain.  depth_check: the argument rules of include/agh.h (the error text names
// the image and the field).  depth_to_raw: the images (host: uploaded into d_depth on `st`, or adopted from a staged set when
// use_staged; device: read in place) back-projected by k_deproject on `st` into d_raw_xyz, packed, stride 12.
// capture >= 0: the images are capture `capture`'s of a batch, and the error text names it too ("capture 3, image 1: ...").
// With a depth filter set (agh_set_depth_filter) depth_to_raw and depth_batch_to_raw launch k_deproject_filtered /
// k_deproject_filtered_batch in the plain kernels' place, behind a memset of the views' counters on `st`; without one they launch
// what they always launched.
int depth_check(agh::Ctx* c, const char* who, const agh_depth_image* images, int32_t n_images, bool on_device, int64_t* n_points,
  int capture = -1);
int depth_to_raw(agh_ctx* ctx, const char* who, const agh_depth_image* images, int n_images, bool on_device, bool use_staged,
  hipStream_t st);
// The fourth source kind, a batch of captures as depth images (agh_localize_depth_batch*): `images` is the flat array in capture
// order, capture k's are the next n_images[k].  depth_batch_check: 1 <= C <= 64, every n_images[k] 1 or 2, fewer than 2^30 points
// in all, depth_check's rules per image; first[k] (C + 1 entries) = capture k's first point among the batch's, left0[k] = W0 x H0
// of its image 0.  depth_batch_to_raw: every image of the batch back-projected by ONE k_deproject_batch on `st` into d_raw_xyz,
// capture after capture, packed, stride 12 (host images uploaded into d_depth on `st`; drop_staged: a pending staged set of any
// kind is dropped and `st` waits for its copies); a failure has drained `st`.
int depth_batch_check(agh::Ctx* c, const char* who, const agh_depth_image* images, const int32_t* n_images, int32_t C, bool on_device,
  std::vector<int64_t>* first, std::vector<int64_t>* left0);
int depth_batch_to_raw(agh_ctx* ctx, const char* who, const agh_depth_image* images, const int32_t* n_images, int C, bool on_device,
  bool drop_staged, hipStream_t st);
// The rules a source adds to a chain's arguments (include/agh.h; C captures with lp[k], single: the single chain's texts, which name
// no capture), and its bytes to where the chain reads them, queued on st: device point bytes are read in place; host bytes and
// all image masks go, packed in point order, into *buf (grown to n_tot bytes, *cap its capacity), capture k's n[k] bytes at
// byte_off[k]; (*d_bytes)[k] says where capture k's lie.  The single chain owns c->d_mask, the batch chain its state's.
int sample_source_check(agh::Ctx* c, const agh::SampleSource& src, const agh::DepthCaptures* depth, const agh_localize_params* lp, int C,
  bool single);
int sample_source_to_device(agh::Ctx* c, const agh::SampleSource& src, const agh::DepthCaptures* depth, int C, const int64_t* n,
  const int64_t* byte_off, int64_t n_tot, uint8_t** buf, int64_t* cap, hipStream_t st, std::vector<const uint8_t*>* d_bytes);
// (unit: what the chain's C lists are, "capture" or "object", for the error texts; nullptr: the one list of a single chain)
// (names: what list k is called when it is no plain "unit k" -- "capture 2, object 5" of a labelled batch)
int chain_collect(agh_ctx* ctx, const char* who, const char* unit, int C, const int* counts, int count_stride, int64_t S_tot,
  const int* bad, int (*requeue)(agh_ctx*, bool handles_only), const std::vector<std::string>* names = nullptr);
// localize_batch.hip's tail as the labelled chain of localize.hip runs it, one list per OBJECT of the one capture.
// labeled_tail_prepare: the batch state's table of K spans of S samples (soff = j * S, the one workspace), its handle-search slots
// and its pinned sample mirror (*h_samples), everything queued on the context's stream.  batch_queue: search -> classification ->
// kept hands per list -> handle search.  batch_collect: chain_collect over the lists, results[k] (nv[k]: list k's voxel count)
// and the outputs' assembly, spans in list order.
int labeled_tail_prepare(agh_ctx* ctx, int K, int64_t S, const agh_localize_params* lp, double x1, double x2, int32_t** h_samples);
int batch_queue(agh_ctx* ctx, bool handles_only);
int batch_collect(agh_ctx* ctx, const char* who, const char* unit, const int64_t* nv, const agh::ChainOutputs& out,
  agh_localize_batch_result* results);
