// localize.hip -- the online chain of the reference's only online caller as one call (or two halves of one):
// GraspLocalizer::localizeGrasps, grasp_localizer.cpp:95-103 = localizeHands -> predictAntipodalHands -> findHandles per capture.
// agh_localize / agh_localize_device / agh_localize_begin / agh_localize_stage / agh_localize_end, agh_localize_depth* and the
// masked forms of both (agh_localize_masked*, agh_localize_depth_masked*) and the labelled ones (agh_localize_labeled*,
// agh_localize_depth_labeled*) and the clustered ones (agh_localize_clustered*, agh_localize_depth_clustered*) of include/agh.h
// (the back-projection of depth images: depth.hip; the sample list under a mask: sample_mask.hip; one list per object of a label
// image: sample_labels.hip, or per connected component of the cloud: sample_cluster.hip, with localize_batch.hip's tail); the stages
// themselves (preprocessing, search, classification, handle search) are api.hip's, voxelize.hip's, hog_svm.hip's and handles.hip's.
#include "agh_internal.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

using namespace agh;

namespace
{
// (the two kernels keep C names: the traces under profiles/ know them by these)
// One sample per stratum of the cloud (include/agh.h, agh_localize); the point count is read on the device.
extern "C" __global__ void k_draw_samples(const int* __restrict__ cloud_off, int n_clouds, int S, unsigned long long seed,
  int32_t* __restrict__ out, int32_t* __restrict__ host_out)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= S)
    return;
  const long long N = cloud_off[n_clouds];
  const int32_t v = draw_stratum(N, S, k, seed);
  out[k] = v;
  if (host_out)
    host_out[k] = v;
}
// The hands Learning::classify kept (svm_keep; all of them if !use_keep), in list order (learning.cpp:236-243), as the handle
// search's input -- and a second time into pinned host memory.  One work-group around compact_kept_records (agh_internal.h).
// box.on (a chain with filters_boundaries and no classifier): the hands Localization::filterHands drops are left out too (with
// the classifier their svm_keep is 0 already).
// host_counts: [4] hypotheses, [5] kept, [6] the search's error word.
// drop (null: none): the hand drop stage's bytes -- a dropped hand is left out -- and its counters, which go to the pinned hf_host
// with the counts.
extern "C" __global__ __launch_bounds__(1024) void k_compact_kept(const agh_hypothesis* __restrict__ in, const int64_t* __restrict__ n_in,
  int64_t cap_in, int use_keep, BoundaryBox box, agh_hypothesis* __restrict__ out, int out_cap, int* __restrict__ n_out,
  agh_hypothesis* __restrict__ host_out, int host_cap, int* __restrict__ host_counts, const int32_t* __restrict__ flags,
  const uint8_t* __restrict__ drop, const unsigned* __restrict__ hf_counts, int* __restrict__ hf_host, MarginOut mg)
{
  __shared__ int src[kCompactList];
  __shared__ int wsum[16];
  __shared__ int carry;
  const int64_t n = min(*n_in, cap_in);
  const int K = compact_kept_records(in, 0, n, use_keep, box.on, box.ws, src, wsum, &carry, out, out_cap, host_out, host_cap, 0, drop,
    mg.sums, mg.out, mg.host);
  if (drop && threadIdx.x < kHandDropCounters)
    hf_host[threadIdx.x] = (int) hf_counts[threadIdx.x];
  if (threadIdx.x == 0)
  {
    *n_out = K;
    if (host_counts)
    {
      host_counts[4] = (int) n;
      host_counts[5] = K;
      host_counts[6] = flags[0] | (*n_in > cap_in ? 2 : 0);
    }
  }
}
}  // namespace

// ---- shared with localize_batch.hip (declared in agh_internal.h) ----

// The NEXT chain's captures up, beside whatever runs on the context's stream: packed end to end (device_stride's rule) into the
// context's second raw buffer, on a stream of its own.  A pageable source makes the call last as long as its copies (the kernels of
// the chain in flight run meanwhile: that is the overlap); a pinned one is read asynchronously and must stay valid until the copy
// is done: until the begin that adopts (or drops) the set has returned for agh_localize_stage, until the matching end for
// agh_localize_batch_stage (include/agh.h).  The callers have checked the arguments.
int stage_captures(agh_ctx* ctx, const char* who, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n, int C,
  bool as_batch)
{
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  AGH_HIPCHK(c, hipSetDevice(c->device));
  if (int rc = ensure_stage_stream(c, who))
    return rc;
  // A failure from here on leaves nothing staged -- and an earlier set's copies may still be reading their (pinned) sources, with no
  // begin left to wait for stage_done: the stage stream is drained before the flag comes down.
  auto stage_fail = [c](int code) {
    (void) hipStreamSynchronize(c->stage_stream);
    c->loc.staged = false;
    return code;
  };
  int64_t need = 0;
  for (int k = 0; k < C; k++)
    need += n[k] * (device_stride(stride_bytes[k]) / 4);
  if (need > c->stage_cap || !c->d_stage_xyz)
  {
    // (nobody reads this buffer now: the chain in flight reads d_raw_xyz)
    if (int rc = dev_alloc(c, &c->d_stage_xyz, (size_t) std::max<int64_t>(need, 1)))
      return stage_fail(rc);
    c->stage_cap = need;
    c->stage_read_set = false;
  }
  if (c->stage_read_set)  // the last batch chain that read the buffer these copies overwrite (it has ended: see DESIGN.md)
  {
    AGH_HIPCHK_OR(c, hipStreamWaitEvent(c->stage_stream, c->stage_read, 0), stage_fail(AGH_ERR_HIP));
  }
  // (whatever was staged before is replaced: its copies are ahead of these on the stage stream, so stage_done covers them too)
  int64_t off = 0;
  for (int k = 0; k < C; k++)
  {
    AGH_HIPCHK_OR(c, upload_capture(c->d_stage_xyz + off, xyz[k], stride_bytes[k], n[k], c->stage_stream), stage_fail(AGH_ERR_HIP));
    off += n[k] * (device_stride(stride_bytes[k]) / 4);
  }
  AGH_HIPCHK_OR(c, hipEventRecord(c->stage_done, c->stage_stream), stage_fail(AGH_ERR_HIP));
  L.staged_src.assign(xyz, xyz + C);
  L.staged_stride.assign(stride_bytes, stride_bytes + C);
  L.staged_n.assign(n, n + C);
  L.staged_captures = as_batch ? C : 0;
  L.staged_depth = false;
  L.staged = true;
  return AGH_OK;
}

// The end of a chain over C captures, after its one synchronisation: attempt 0 is on the host (capture k's counts at
// counts + k * count_stride: [0..3] the handle search's, [4..6] the compaction's).  The search once more for a capacity class
// (on the cloud that is already there), the handle search once more for a walk the batched kernel declined -- requeue queues
// either on the context's stream -- then the limits.  Errors are `who`'s, and `unit` k's ("capture 3", "object 3") if the chain
// has several lists; bad: a batch's per-capture flags of a sample index outside the capture (null: flags_to_status' text stands).
int chain_collect(agh_ctx* ctx, const char* who, const char* unit, int C, const int* counts, int count_stride, int64_t S_tot,
  const int* bad, int (*requeue)(agh_ctx*, bool handles_only), const std::vector<std::string>* names)
{
  Ctx* c = &ctx->c;
  auto of = [&](int k) {
    if (names)
      return std::string(who) + ": " + (*names)[(size_t) k] + ": ";
    return std::string(who) + (unit ? ": " + std::string(unit) + " " + std::to_string(k) : std::string()) + ": ";
  };
  bool handles_only = false;
  int rc;
  for (int attempt = 0;; attempt++)
  {
    if (attempt > 0)
    {
      if ((rc = requeue(ctx, handles_only)) != AGH_OK)
        return chain_fail(c, rc);
      AGH_HIPCHK_OR(c, hipStreamSynchronize(c->stream), chain_fail(c, AGH_ERR_HIP));
    }
    if (!handles_only)
    {
      int32_t flags[1] = { counts[6] };
      rc = flags_to_status(c, flags);
      if (rc == AGH_ERR_RETRY && attempt < 3)
      {
        // (the larger capacity classes are on now)
        if ((rc = ensure_call_buffers(c, std::max<int64_t>(S_tot, 1))) != AGH_OK)
          return rc;
        continue;
      }
      if (rc == AGH_ERR_INVALID_ARGUMENT && (flags[0] & 4) && bad)
        for (int k = 0; k < C; k++)
          if (bad[k])
          {
            c->err = std::string(who) + ": a sample index of capture " + std::to_string(k) + " is outside its voxelised cloud";
            break;
          }
      if (rc != AGH_OK)
        return rc;
    }
    bool declined = false;
    for (int k = 0; k < C; k++)
    {
      const int* h = counts + k * count_stride;
      if (h[2] == 2 || h[5] > 8192)  // ([5]: the hands that survived the classifier and the boundary filter)
      {
        c->err = of(k) + "more than 8192 hands for the handle search (classify first, or search fewer samples)";
        return AGH_ERR_CAPACITY;
      }
      declined |= h[3] != 0;  // a row of the pair matrix longer than kMaxRow (two waves' worth; see agh_find_handles)
    }
    c->handles_sequential = declined;
    if (declined && !c->loc.with_sequential && attempt < 3)
    {
      handles_only = true;
      continue;
    }
    break;
  }
  for (int k = 0; k < C; k++)
    if (counts[k * count_stride + 2])
    {
      c->err = of(k) + "a seed hand has more than 2048 inliers";
      return AGH_ERR_CAPACITY;
    }
  return AGH_OK;
}

// ---- agh_localize = agh_localize_begin (everything queued) + agh_localize_end (the one synchronisation, the results, the rare
// repeats).  Between the two the caller may stage the NEXT capture (agh_localize_stage: upload on a second stream into a second
// raw buffer, under this cloud's kernels), which the next begin adopts instead of uploading.  One chain is in flight at a time:
// the context's device buffers, pinned mirrors and host-side cloud state are single. ----

// search -> classification -> kept hands -> handle search, queued on the context's stream (handles_only: the handle search alone,
// once more, on the hands that are already there)
static int localize_queue(agh_ctx* ctx, bool handles_only)
{
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  hipStream_t st = c->stream;
  const HandlePins pin = handle_pins(c);
  const HandleMirror hm{ pin.handles, (int) c->h_pin_handles_cap, pin.idx, (int) c->h_pin_handles_cap, pin.counts };
  int* d_hcount = c->d_h_counts + 4;  // (behind the HandleCounts record)
  const int64_t hand_bound = std::min<int64_t>(8 * L.S, 8192);
  int rc;
  for (int k = 0; k < (handles_only ? 4 : 8); k++)  // ([4..6], the search's counts, outlive a repeat of the handle search alone)
    pin.counts[k] = 0;
  L.with_sequential = c->handles_sequential;
  if (!handles_only)
  {
    c->mirror = HostMirror{ nullptr, 0, nullptr };
    if ((rc = agh_find_hands_device(ctx, c->d_idx_own, L.S, 0, c->d_out_own, c->s_cap * 8, c->d_nout, st)) != AGH_OK)
      return rc;
    // (filters_boundaries: the classifier labels the hands near the workspace's faces 0 without classifying them; without it,
    // the compaction drops them)
    const double* ws = L.filters ? L.lp.workspace : nullptr;
    // (the hand drop stage's bytes, which the classifier and the compaction honour beside the box; null and nothing launched
    // without a test set)
    const int64_t hyp_bound = std::min<int64_t>(c->last_s * 8, c->last_cap);
    const HandDropView hd = hand_drop_stage(c, hyp_bound, nullptr, 1, st);
    if (hd.rc != AGH_OK)
      return hd.rc;
    if (L.classify && (rc = hog_svm(c, hyp_bound, c->d_keep, st, ws, hd.drop)) != AGH_OK)
      return rc;
    // (agh_set_handle_ranking: the kept hands' margins leave with them; nothing without one)
    MarginOut mg;
    if ((rc = handle_rank_prepare(c, 1, hand_bound, hand_bound, L.classify, &mg)) != AGH_OK)
      return rc;
    hipLaunchKernelGGL(k_compact_kept, dim3(1), dim3(1024), 0, st, (const agh_hypothesis*) c->d_out_own, (const int64_t*) c->d_nout,
      c->s_cap * 8, L.classify ? 1 : 0, boundary_box(L.classify ? nullptr : ws), c->d_h_hands, (int) hand_bound, d_hcount, pin.hands,
      (int) c->h_pin_handles_cap, pin.counts, (const int32_t*) c->d_flags, hd.drop, hd.d_counts, hd.h_counts, mg);
    if (hipGetLastError() != hipSuccess)
    {
      c->err = "k_compact_kept launch failed";
      return AGH_ERR_HIP;
    }
  }
  timing_begin(c, st);
  rc = handle_search(c, hand_bound, L.x1, L.x2, L.min_inliers, L.min_length, st, hm, L.with_sequential, d_hcount);
  timing_mark(c, "handle_search", st);
  if (rc != AGH_OK)
  {
    c->err = "handle search launch failed";
    return rc;
  }
  const HandleBufs hb{ c->d_h_hands, c->d_h_bits, c->d_h_rowcnt, c->d_h_first, c->d_h_n, c->d_h_idx, c->d_h_counts, c->d_h_tmp,
    c->d_h_handles };
  return handle_rank_stage(c, hb, 1, 0, hm, 0, st);
}

std::string agh::cluster_params_fault(const agh_cluster_params& cp)
{
  const double* q = cp.plane;
  const char* field[7] = { "plane[0]", "plane[1]", "plane[2]", "plane[3]", "min_height", "max_height", "tolerance" };
  const double value[7] = { q[0], q[1], q[2], q[3], cp.min_height, cp.max_height, cp.tolerance };
  for (int k = 0; k < 7; k++)
    if (!std::isfinite(value[k]))
      return std::string(field[k]) + " is not finite";
  if (std::fabs(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) - 1.0) > 1e-6)
    return "plane: (a, b, c) must be a unit vector (|a^2 + b^2 + c^2 - 1| <= 1e-6)";
  if (cp.min_height >= cp.max_height)
    return "min_height must be below max_height";
  if (!(cp.tolerance > 0.0) || cp.tolerance > 0.05)
    return "tolerance must be in (0, 0.05]";
  if (cp.min_voxels < 1)
    return "min_voxels must be >= 1";
  if (cp.max_objects < 1 || cp.max_objects > kMaxClouds)
    return "max_objects must be 1 .. 64";
  return std::string();
}

// The texts of sample_source_check, where the single and the batch chains word a rule differently.  The single labelled chain
// speaks of its labels as a mask; a batch's texts name the capture (and the image) in front.
namespace
{
struct SourceWording
{
  const char* array_null;       // no array of the captures' bytes (or no image records) at all
  const char* bytes_null;       // one capture's bytes
  const char* with_sample_idx;
  const char* image;            // what a batch calls an image's record, in front of "row_stride_bytes is below the image's width"
  const char* all_null;         // no image of a capture has bytes
};
const SourceWording& source_wording(bool single, SourceKind kind)
{
  static const SourceWording mask{ "masks is NULL", "the mask is NULL", "a mask together with sample_idx (an explicit list needs no mask)",
    "", "every mask's data is NULL (no pixel would be eligible)" };
  static const SourceWording batch_mask{ "masks is NULL (every capture of a masked batch has a mask)", mask.bytes_null,
    mask.with_sample_idx, "the mask's ", mask.all_null };
  static const SourceWording batch_labels{ "labels is NULL (every capture of a labelled batch has labels)", "the label array is NULL",
    "labels together with sample_idx (an explicit list needs no labels)", "the label image's ",
    "every label image's data is NULL (no pixel would belong to an object)" };
  static const SourceWording clusters{ "", "", "sample_idx must be NULL (the lists are drawn on the objects the call finds)", "", "" };
  if (kind >= SourceKind::Clusters)
    return clusters;
  return single ? mask : (kind == SourceKind::Labels ? batch_labels : batch_mask);
}
}  // namespace

// (the order of the rules decides which of two faults a call reports: it is part of the contract)
int sample_source_check(Ctx* c, const SampleSource& src, const DepthCaptures* depth, const agh_localize_params* lp, int C, bool single)
{
  const SourceWording& w = source_wording(single, src.kind);
  const std::string objects = src.clustered() ? "max_objects" : "n_objects";
  auto bad = [&](const std::string& what) {
    c->err = std::string(src.who) + ": " + what;
    return AGH_ERR_INVALID_ARGUMENT;
  };
  if (!single)  // (the single entry points pass pointers to their own scalars; their image records are tested behind sample_idx)
  {
    if (src.fitted() && !src.fit)
      return bad("fp is NULL (every capture of a fitted batch has its agh_plane_fit_params record)");
    if (src.clustered() && !src.cluster)
      return bad("cp is NULL (every capture of a clustered batch has its agh_cluster_params record)");
    if (src.kind == SourceKind::Labels && !src.n_objects)
      return bad("n_objects is NULL");
    if (src.has_bytes() && (depth ? !src.images : !src.points))
      return bad(w.array_null);
  }
  int64_t lists = 0, samples = 0;
  for (int k = 0, i0 = 0; k < C; k++)
  {
    const std::string cap = "capture " + std::to_string(k);
    const std::string at = single ? std::string() : cap + ": ";
    if (src.clustered())
    {
      agh_cluster_params q = src.cluster[k];
      if (src.fitted())
      {
        const std::string fit_fault = plane_fit_params_fault(src.fit[k]);
        if (!fit_fault.empty())
          return bad(at + fit_fault);
        placeholder_plane(&q);
      }
      const std::string fault = cluster_params_fault(q);
      if (!fault.empty())
        return bad(at + fault);
    }
    else if (src.kind == SourceKind::Labels && (src.n_objects[k] < 1 || src.n_objects[k] > kMaxClouds))
      return bad(at + "n_objects must be 1 .. 64");
    if (src.per_object())
    {
      lists += src.objects(k);
      samples += (int64_t) src.objects(k) * lp[k].n_samples;
      if (lists > kMaxClouds)
        return bad(at + "more than 64 lists in all (the sum of " + objects + " up to this capture)");
      if (samples > (1 << 24))
        return bad(single ? objects + " x n_samples exceeds 2^24"
                          : at + "more than 2^24 samples in all (the sum of " + objects + " x n_samples up to this capture)");
    }
    if (lp[k].sample_idx)
      return bad(at + w.with_sample_idx);
    if (!src.has_bytes())
      continue;
    if (!depth)
    {
      if (!src.points[k])
        return bad(at + w.bytes_null);
      continue;
    }
    if (!src.images)
      return bad(w.array_null);
    bool any = false;
    for (int j = 0; j < depth->n_images[k]; j++)
    {
      const agh_sample_mask& m = src.images[i0 + j];
      if (!m.data)
        continue;
      any = true;
      if (m.row_stride_bytes < depth->images[i0 + j].width)
        return bad((single ? "mask " + std::to_string(j) + ": " : cap + ", image " + std::to_string(j) + ": " + w.image) +
                   "row_stride_bytes is below the image's width");
    }
    if (!any)
      return bad(at + w.all_null);
    i0 += depth->n_images[k];
  }
  return AGH_OK;
}

int sample_source_to_device(Ctx* c, const SampleSource& src, const DepthCaptures* depth, int C, const int64_t* n, const int64_t* byte_off,
  int64_t n_tot, uint8_t** buf, int64_t* cap, hipStream_t st, std::vector<const uint8_t*>* d_bytes)
{
  d_bytes->resize((size_t) C);
  if (!depth && src.on_device)
  {
    std::copy(src.points, src.points + C, d_bytes->begin());
    return AGH_OK;
  }
  if (n_tot > *cap || !*buf)
  {
    *cap = 0;
    if (int rc = dev_alloc(c, buf, (size_t) std::max<int64_t>(n_tot, 1)))
      return rc;
    *cap = std::max<int64_t>(n_tot, 1);
  }
  const hipMemcpyKind kind = src.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  for (int k = 0, i0 = 0; k < C; k++)
  {
    uint8_t* dst = *buf + byte_off[k];
    (*d_bytes)[k] = dst;
    if (!depth)
    {
      if (n[k] > 0)
        AGH_HIPCHK(c, hipMemcpyAsync(dst, src.points[k], (size_t) n[k], kind, st));
      continue;
    }
    for (int j = 0; j < depth->n_images[k]; j++)
    {
      const size_t W = (size_t) depth->images[i0 + j].width, H = (size_t) depth->images[i0 + j].height;
      const agh_sample_mask& m = src.images[i0 + j];
      if (!m.data)
        AGH_HIPCHK(c, hipMemsetAsync(dst, 0, W * H, st));
      else
        AGH_HIPCHK(c, hipMemcpy2DAsync(dst, W, m.data, (size_t) m.row_stride_bytes, W, H, kind, st));
      dst += W * H;
    }
    i0 += depth->n_images[k];
  }
  return AGH_OK;
}

static int localize_begin_impl(agh_ctx* ctx, const float* xyz, bool xyz_on_device, int64_t stride_bytes, int64_t n,
  const agh_localize_params* lp, const DepthCaptures* depth = nullptr, const SampleSource* src = nullptr)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  const char* who = src ? src->who : (depth ? depth->who : "agh_localize_begin");
  if (L.active)
  {
    c->err = std::string(who) + ": a chain is in flight (agh_localize_end first)";
    return AGH_ERR_STATE;
  }
  if (c->batch_active)
  {
    c->err = std::string(who) + ": an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  agh_localize_params lp_depth;
  if (depth && lp)
  {
    // (the arguments of the images first: their sizes are the capture's; then size_left and dense as include/agh.h fixes them)
    if (int rc = depth_check(c, depth->who, depth->images, depth->n_images[0], depth->on_device, &n))
      return rc;
    lp_depth = *lp;
    lp_depth.size_left = (int64_t) depth->images[0].width * depth->images[0].height;
    lp_depth.dense = 1;
    lp = &lp_depth;
    stride_bytes = 12;
  }
  if (!lp || (!depth && bad_capture(xyz, stride_bytes, n)) || !(lp->cell_size > 0.0) || lp->size_left < 0 || lp->n_samples < 0 ||
      lp->n_samples > (1 << 24) || lp->min_inliers < 1)
  {
    c->err = "agh_localize: bad arguments (see include/agh.h)";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (lp->filters_boundaries != 0 && lp->filters_boundaries != 1)
  {
    c->err = "agh_localize: filters_boundaries must be 0 or 1";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (lp->classify && !c->has_svm)
  {
    c->err = "agh_localize: classify needs a loaded SVM (agh_load_svm*)";
    return AGH_ERR_NO_SVM;
  }
  if (cam_table_mismatch(c, "agh_localize", 1))  // (the chain's cloud is a batch of one; the table stays the context's for the
    return AGH_ERR_INVALID_ARGUMENT;              // whole chain -- the setter refuses mid-chain -- so its repeats search with it too)
  if (!handle_thresholds(&L.x1, &L.x2))
  {
    c->err = "agh_localize: this libm's acos is not monotone around the 0.34 rad thresholds";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (src)
    if (int rc = sample_source_check(c, *src, depth, lp, 1, true))
      return rc;
  // (agh_set_hand_filter's observed-space criterion reads the chain's depth images; the repeat of a whole call re-enters with the
  // points its first pass made of them, and with the views that pass kept)
  if (!L.repeated)
    if (int rc = hand_filter_check(c, who, depth ? depth->images : nullptr, depth ? depth->n_images : nullptr, depth ? 1 : 0, depth != nullptr))
      return rc;
  if (int rc = handle_rank_check(c, who, lp->classify != 0))
    return rc;
  AGH_HIPCHK(c, hipSetDevice(c->device));
  const int64_t S = lp->n_samples;
  const int K = src && src->per_object() ? src->objects(0) : 0;  // (a chain with a list per object: K lists of S samples)
  const int64_t S_all = K ? K * S : S;
  hipStream_t st = c->stream;
  int rc;
  // ---- 1. raw cloud up (unless it is on the device already: agh_localize_device, which reads it in place with the caller's
  // stride -- or was staged: agh_localize_stage), voxelisation and grid build queued; the voxel count stays on the device when it
  // can ----
  const int64_t dev_stride = xyz_on_device ? stride_bytes : device_stride(stride_bytes);
  const float* d_raw = xyz;
  // (a masked begin of host data never adopts a staged set: it drops a pending one as a begin of another kind does)
  const bool adopts = !src;
  if (depth)
  {
    if (!adopts && !depth->on_device)
    {
      if (L.staged)
        AGH_HIPCHK(c, hipStreamWaitEvent(st, c->stage_done, 0));
      L.staged = false;
    }
    if ((rc = depth_to_raw(ctx, depth->who, depth->images, depth->n_images[0], depth->on_device, adopts, st)) != AGH_OK)
      return rc;
    d_raw = c->d_raw_xyz;
  }
  else if (!xyz_on_device)
  {
    if (adopts && L.staged_is(&xyz, &stride_bytes, &n, 1, false) && c->d_stage_xyz)
    {
      // the capture is (or is about to be) in the second raw buffer: the two buffers change places, the chain waits for the copy
      swap_raw_buffers(c);
      L.staged = false;
      AGH_HIPCHK(c, hipStreamWaitEvent(st, c->stage_done, 0));
    }
    else
    {
      // (a staged set that is not this capture is dropped -- its copy may still be reading the caller's source: the chain waits
      // for it too, so that agh_localize_end's synchronisation covers it, as include/agh.h promises)
      if (L.staged)
        AGH_HIPCHK(c, hipStreamWaitEvent(st, c->stage_done, 0));
      L.staged = false;
      const int64_t need = n * (dev_stride / 4);
      if (need > c->raw_cap || !c->d_raw_xyz)
      {
        if ((rc = dev_alloc(c, &c->d_raw_xyz, (size_t) need)))
          return rc;
        c->raw_cap = need;
      }
      AGH_HIPCHK(c, upload_capture(c->d_raw_xyz, xyz, stride_bytes, n, st));
    }
    d_raw = c->d_raw_xyz;
  }
  L.source.keep(src, 1, true);
  const int64_t byte_off = 0;
  if (src && src->has_bytes() &&
      (rc = sample_source_to_device(c, *src, depth, 1, &n, &byte_off, n, &c->d_mask, &c->mask_cap, st, &L.source.d_bytes)) != AGH_OK)
    return chain_fail(c, rc);  // (the capture's copy may be in flight)
  const uint8_t* d_mask = L.source.d_bytes.empty() ? nullptr : L.source.d_bytes[0];
  L.S = S;
  L.classify = lp->classify != 0;
  L.filters = lp->filters_boundaries != 0;
  L.min_inliers = lp->min_inliers;
  L.min_length = lp->min_length;
  L.lp = *lp;
  L.lp.sample_idx = nullptr;  // (the list is copied below; a repeat of the whole call reads it from the pinned copy)
  L.explicit_samples = lp->sample_idx != nullptr;
  L.d_raw = d_raw;
  L.dev_stride = dev_stride;
  L.n_raw = n;
  L.deferred = false;
  L.nv = 0;
  rc = preprocess_device_impl(ctx, d_raw, dev_stride, n, lp->size_left, lp->dense, lp->workspace, lp->cell_size, &L.nv, nullptr,
    true, &L.deferred);
  if (rc != AGH_OK)
    return rc;
  c->cloud_async = false;  // (everything below is queued on the context's own stream, and the call ends with its synchronisation)
  // (every error return from here on is a chain_fail: the host may only know a BOUND of the cloud's size)
  // ---- 2. buffers for the bounds ----
  if ((rc = ensure_call_buffers(c, std::max<int64_t>(S_all, 1))) != AGH_OK)  // (S = 0: the later stages still want their buffers)
    return chain_fail(c, rc);
  if (S_all > c->idx_cap || !c->d_idx_own)
  {
    if ((rc = dev_alloc(c, &c->d_idx_own, (size_t) std::max<int64_t>(S_all, 1024))))
      return chain_fail(c, rc);
    c->idx_cap = std::max<int64_t>(S_all, 1024);
  }
  if ((rc = ensure_host_staging(c, S, 1024)) != AGH_OK)
    return chain_fail(c, rc);
  int32_t* h_idx = reinterpret_cast<int32_t*>(c->h_pin + kPinHeaderBytes);
  int32_t* h_idx_labeled = nullptr;  // (a labelled chain: the batch tail's slots, table and pinned sample mirror)
  if ((rc = K ? labeled_tail_prepare(ctx, K, S, lp, L.x1, L.x2, &h_idx_labeled) : ensure_handle_buffers(c, std::min<int64_t>(8 * S, 8192))) != AGH_OK)
    return chain_fail(c, rc);
  if (lp->classify)
  {
    AGH_HIPCHK_OR(c, ensure_keep_buffers(c, c->s_cap * 8), chain_fail(c, AGH_ERR_HIP));
  }
  // ---- 3. the sample list ----
  if (L.source.clustered())  // (the grid build is queued: the preprocessing above bound the voxelised cloud)
  {
    // (a fitted chain: the plane is found first, on the same stream, and the cluster kernels read the record it leaves on the device)
    const ClusterDev* d_cp = nullptr;
    const ClusterDev cp = cluster_dev(L.source.cluster[0]);
    if (L.source.fitted() && (rc = plane_fit_stage(c, n, L.source.fit[0], cp, st, &d_cp)) != AGH_OK)
      return chain_fail(c, rc);
    if ((rc = sample_cluster_stage(c, n, cp, K, S, (unsigned long long) lp->sample_seed, c->d_idx_own, h_idx_labeled, st, d_cp)) != AGH_OK)
      return chain_fail(c, rc);
  }
  else if (K)  // (for S = 0 too, as the mask's)
  {
    if ((rc = sample_label_stage(c, d_raw, dev_stride / 4, n, d_mask, K, lp->cell_size, S, (unsigned long long) lp->sample_seed,
           c->d_idx_own, h_idx_labeled, st)) != AGH_OK)
      return chain_fail(c, rc);
  }
  else if (src)  // (for S = 0 too: the count of eligible voxels is what a caller sizes S with)
  {
    if ((rc = sample_mask_stage(c, d_raw, dev_stride / 4, n, d_mask, lp->cell_size, S, (unsigned long long) lp->sample_seed,
           c->d_idx_own, h_idx, reinterpret_cast<long long*>(c->h_pin) + kPinMaskCount, st)) != AGH_OK)
      return chain_fail(c, rc);
  }
  else if (S > 0)
  {
    if (lp->sample_idx)
    {
      if (lp->sample_idx != h_idx)  // (a repeat of the whole call hands the pinned copy back in)
        std::memcpy(h_idx, lp->sample_idx, sizeof(int32_t) * (size_t) S);
      AGH_HIPCHK_OR(c, hipMemcpyAsync(c->d_idx_own, h_idx, sizeof(int32_t) * S, hipMemcpyHostToDevice, st), chain_fail(c, AGH_ERR_HIP));
    }
    else
    {
      hipLaunchKernelGGL(k_draw_samples, dim3((unsigned) ((S + 255) / 256)), dim3(256), 0, st, (const int*) c->d_cloud_off, 1, (int) S,
        (unsigned long long) lp->sample_seed, c->d_idx_own, h_idx);
      AGH_HIPCHK_OR(c, hipGetLastError(), chain_fail(c, AGH_ERR_HIP));
    }
  }
  // ---- 4. search -> classification -> kept hands -> handle search: queued; agh_localize_end waits ----
  if ((rc = K ? batch_queue(ctx, false) : localize_queue(ctx, false)) != AGH_OK)
    return chain_fail(c, rc);
  L.active = true;
  return AGH_OK;
}

// (results: a labelled chain's, one record per object, where a chain of another kind has *result)
static int localize_end_impl(agh_ctx* ctx, const ChainOutputs& out, agh_localize_result* result, agh_localize_batch_result* results = nullptr)
{
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  L.active = false;
  c->results = ChainResults{};
  hand_drop_collect(c, 0, nullptr);
  handle_rank_collect(c, 0, nullptr);
  const int64_t S = L.S;
  const HandlePins pin = handle_pins(c);
  const int* h_counts = pin.counts;
  int32_t* h_idx = reinterpret_cast<int32_t*>(c->h_pin + kPinHeaderBytes);
  int rc;
  if (hipStreamSynchronize(c->stream) != hipSuccess)
  {
    drop_bound_cloud(c);
    c->err = "agh_localize: hipStreamSynchronize failed";
    return AGH_ERR_HIP;
  }
  if (L.deferred)  // the descriptor of the speculative voxelisation, now on the host
  {
    L.deferred = false;
    const VoxDesc h = *c->h_vox_desc;
    L.nv = (int64_t) (h.n_vox[0] + h.n_vox[1]);
    if (h.error)
    {
      // error 2: the lattice outgrew the bitmap kept from the previous cloud -- the whole call once more, sized from this
      // cloud's lattice (the context then has no bitmap to speculate with: the preprocessing takes its own round trips).  The
      // raw capture is still where the chain read it: in the context's raw buffer, or in the caller's device memory.
      drop_bound_cloud(c);
      if (h.error == 2 && !L.repeated)
      {
        drop_vox_bitmaps(c);
        agh_localize_params lp = L.lp;
        lp.sample_idx = L.explicit_samples ? h_idx : nullptr;
        L.repeated = true;
        // (the source is where the chain read it, as the capture is: in the context's buffer, or in the caller's device memory; the
        // begin stores it anew, so it re-enters with a copy)
        const StoredSource kept = L.source;
        const SampleSource again = kept.view();
        rc = localize_begin_impl(ctx, L.d_raw, true, L.dev_stride, L.n_raw, &lp, nullptr, kept.kind != SourceKind::None ? &again : nullptr);
        if (rc == AGH_OK)
          rc = localize_end_impl(ctx, out, result, results);
        c->loc.repeated = false;
        return rc;
      }
      c->err = "the voxel lattice of the kept points exceeds 2^33 cells (1 GiB bitmap): set a workspace "
               "(Localization::setWorkspace) that bounds the scene";
      return AGH_ERR_CAPACITY;
    }
    // the bound cloud is now the true one
    c->n_is_bound = false;
    c->vox_last_words = (int64_t) h.n_words;
    c->n = L.nv;
    c->cloud_off.assign({ (int64_t) 0, L.nv });
    c->cloud_off_on_device = true;  // ({0, nv}: what the voxeliser wrote)
    c->n_clouds = 1;
  }
  ChainResults& R = c->results;
  R.kind = L.source.kind;
  R.captures = 1;
  if (const int K = L.objects())
  {
    // the tail of the batch chain: one list per object, every object on the one cloud
    R.lists = K;
    if (L.source.clustered())
    {
      // (the table of k_cluster_select: counts, then the M_j and the ids; the M_j equal the compaction's h_label_counts)
      const long long* t = c->h_cluster_table;
      R.nv = L.nv;
      std::copy(t, t + 4, R.cluster_info[0]);
      for (int j = 0; j < K; j++)
      {
        R.counts[j] = (int64_t) t[8 + j];
        R.cluster_ids[j] = (int32_t) t[8 + kMaxClouds + j];
      }
      if (L.source.fitted())  // (the record k_fit_finish wrote into pinned memory: here with the chain's one synchronisation)
      {
        R.fit_candidates[0] = L.source.fit[0].n_candidates;
        R.fit_results[0] = *c->h_fit_result;
      }
    }
    else
      for (int j = 0; j < K; j++)
        R.counts[j] = (int64_t) c->h_label_counts[j];
    const std::vector<int64_t> nv((size_t) K, L.nv);
    return batch_collect(ctx, L.source.who, "object", nv.data(), out, results);
  }
  if (R.kind == SourceKind::Mask)
  {
    R.lists = 1;
    R.counts[0] = (int64_t) reinterpret_cast<const long long*>(c->h_pin)[kPinMaskCount];
  }
  if ((rc = chain_collect(ctx, "agh_localize", nullptr, 1, h_counts, 0, S, nullptr, localize_queue)) != AGH_OK)
    return rc;
  const int64_t n_hyp = h_counts[4], n_kept = h_counts[5];
  hand_drop_collect(c, 1, &n_hyp);  // (the counters are in pinned memory if the chain ran a test)
  handle_rank_collect(c, 1, &n_kept);
  c->last_nout = std::min<int64_t>(n_hyp, c->s_cap * 8);
  if (result)
    *result = agh_localize_result{ L.nv, n_hyp, n_kept, h_counts[0], h_counts[1] };
  if (out.samples && S > 0)
    std::memcpy(out.samples, h_idx, sizeof(int32_t) * (size_t) S);
  if (h_counts[0] > out.handle_cap || h_counts[1] > out.idx_cap || (out.hands && n_kept > out.hands_cap))
  {
    c->err = "agh_localize: output buffers too small (the counts are in *result)";
    return AGH_ERR_CAPACITY;
  }
  if (h_counts[0] > 0)
  {
    std::memcpy(out.handles, pin.handles, sizeof(agh_handle) * (size_t) h_counts[0]);
    std::memcpy(out.inlier_idx, pin.idx, sizeof(int32_t) * (size_t) h_counts[1]);
  }
  if (out.hands && n_kept > 0)
    std::memcpy(out.hands, pin.hands, sizeof(agh_hypothesis) * (size_t) n_kept);
  return AGH_OK;
}

// agh_localize[_device] = begin + end
static int localize_call(agh_ctx* ctx, const float* xyz, bool xyz_on_device, int64_t stride_bytes, int64_t n,
  const agh_localize_params* lp, const ChainOutputs& out, agh_localize_result* result, const DepthCaptures* depth = nullptr,
  const SampleSource* src = nullptr)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  if (result)
    *result = agh_localize_result{ 0, 0, 0, 0, 0 };
  if (out.bad())
  {
    ctx->c.err = "agh_localize: bad arguments (see include/agh.h)";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  const int rc = localize_begin_impl(ctx, xyz, xyz_on_device, stride_bytes, n, lp, depth, src);
  if (rc != AGH_OK)
    return rc;
  return localize_end_impl(ctx, out, result);
}

// the forms with a list per object (labelled, clustered, fitted) = begin + end; K: the objects, as far as the arguments say
static int per_object_call(agh_ctx* ctx, const float* xyz, bool on_device, int64_t stride_bytes, int64_t n, const DepthCaptures* depth,
  const SampleSource& src, int K, const agh_localize_params* lp, const ChainOutputs& out, agh_localize_batch_result* results)
{
  if (results && K >= 1 && K <= kMaxClouds)
    for (int j = 0; j < K; j++)
      results[j] = agh_localize_batch_result{ { 0, 0, 0, 0, 0 }, 0, 0, 0, 0 };
  if (out.bad())
  {
    ctx->c.err = "agh_localize: bad arguments (see include/agh.h)";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  const int rc = localize_begin_impl(ctx, xyz, depth ? false : on_device, stride_bytes, n, lp, depth, &src);
  if (rc != AGH_OK)
    return rc;
  return localize_end_impl(ctx, out, nullptr, results);
}

extern "C" {

int agh_localize(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap,
  int32_t* samples_out, agh_localize_result* result)
{
  return localize_call(ctx, xyz, false, stride_bytes, n, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result);
}

int agh_localize_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap,
  int32_t* samples_out, agh_localize_result* result)
{
  return localize_call(ctx, d_xyz, true, stride_bytes, n, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result);
}

int agh_localize_begin(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_localize_params* lp)
{
  return localize_begin_impl(ctx, xyz, false, stride_bytes, n, lp);
}

int agh_localize_depth(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap,
  int32_t* samples_out, agh_localize_result* result)
{
  const DepthCaptures depth{ images, &n_images, false, "agh_localize_depth" };
  return localize_call(ctx, nullptr, false, 12, 0, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result, &depth);
}

int agh_localize_depth_device(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_localize_params* lp,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap,
  int32_t* samples_out, agh_localize_result* result)
{
  const DepthCaptures depth{ images, &n_images, true, "agh_localize_depth_device" };
  return localize_call(ctx, nullptr, false, 12, 0, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result, &depth);
}

int agh_localize_depth_begin(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_localize_params* lp)
{
  const DepthCaptures depth{ images, &n_images, false, "agh_localize_depth_begin" };
  return localize_begin_impl(ctx, nullptr, false, 12, 0, lp, &depth);
}

int agh_localize_end(agh_ctx* ctx, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  if (result)
    *result = agh_localize_result{ 0, 0, 0, 0, 0 };
  Ctx* c = &ctx->c;
  if (!c->loc.active)
  {
    c->err = "agh_localize_end: no agh_localize_begin in flight";
    return AGH_ERR_STATE;
  }
  if (c->loc.batch)
  {
    c->err = "agh_localize_end: the chain in flight is a batch's (agh_localize_batch_end collects it)";
    return AGH_ERR_STATE;
  }
  const ChainOutputs out{ handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out };
  if (out.bad())
  {
    // (the chain is queued: drain it, leave the context as a failed call does)
    c->loc.active = false;
    c->err = "agh_localize: bad arguments (see include/agh.h)";
    return chain_fail(c, AGH_ERR_INVALID_ARGUMENT);
  }
  return localize_end_impl(ctx, out, result);
}

// ---- the masked forms (include/agh.h): the chain with its samples drawn among the eligible voxels of a mask ----

int agh_localize_masked(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const uint8_t* mask,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result)
{
  const SampleSource src = mask_source(&mask, nullptr, false, "agh_localize_masked");
  return localize_call(ctx, xyz, false, stride_bytes, n, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result, nullptr, &src);
}

int agh_localize_masked_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const uint8_t* d_mask,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result)
{
  const SampleSource src = mask_source(&d_mask, nullptr, true, "agh_localize_masked_device");
  return localize_call(ctx, d_xyz, true, stride_bytes, n, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result, nullptr, &src);
}

int agh_localize_masked_begin(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const uint8_t* mask,
  const agh_localize_params* lp)
{
  const SampleSource src = mask_source(&mask, nullptr, false, "agh_localize_masked_begin");
  return localize_begin_impl(ctx, xyz, false, stride_bytes, n, lp, nullptr, &src);
}

int agh_localize_depth_masked(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, int32_t n_images,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result)
{
  const DepthCaptures depth{ images, &n_images, false, "agh_localize_depth_masked" };
  const SampleSource src = mask_source(nullptr, masks, false, depth.who);
  return localize_call(ctx, nullptr, false, 12, 0, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result, &depth, &src);
}

int agh_localize_depth_masked_device(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, int32_t n_images,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_result* result)
{
  const DepthCaptures depth{ images, &n_images, true, "agh_localize_depth_masked_device" };
  const SampleSource src = mask_source(nullptr, masks, true, depth.who);
  return localize_call(ctx, nullptr, false, 12, 0, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, result, &depth, &src);
}

int agh_localize_depth_masked_begin(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, int32_t n_images,
  const agh_localize_params* lp)
{
  const DepthCaptures depth{ images, &n_images, false, "agh_localize_depth_masked_begin" };
  const SampleSource src = mask_source(nullptr, masks, false, depth.who);
  return localize_begin_impl(ctx, nullptr, false, 12, 0, lp, &depth, &src);
}

// ---- the labelled forms (include/agh.h): one capture, one list of samples per object of a label image ----

int agh_localize_labeled(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const uint8_t* labels, int32_t n_objects,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  return per_object_call(ctx, xyz, false, stride_bytes, n, nullptr, label_source(&labels, nullptr, &n_objects, false, "agh_localize_labeled"),
    n_objects, lp, { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_labeled_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const uint8_t* d_labels,
  int32_t n_objects, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  return per_object_call(ctx, d_xyz, true, stride_bytes, n, nullptr,
    label_source(&d_labels, nullptr, &n_objects, true, "agh_localize_labeled_device"), n_objects, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_depth_labeled(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels, int32_t n_images,
  int32_t n_objects, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  const DepthCaptures depth{ images, &n_images, false, "agh_localize_depth_labeled" };
  return per_object_call(ctx, nullptr, false, 12, 0, &depth, label_source(nullptr, labels, &n_objects, false, depth.who), n_objects, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_depth_labeled_device(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels, int32_t n_images,
  int32_t n_objects, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  const DepthCaptures depth{ images, &n_images, true, "agh_localize_depth_labeled_device" };
  return per_object_call(ctx, nullptr, true, 12, 0, &depth, label_source(nullptr, labels, &n_objects, true, depth.who), n_objects, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

// ---- the clustered forms (include/agh.h): the labelled chain with the cloud's own connected components as its objects; the
// fitted forms (agh_localize_clustered_fit*): with the plane found by plane_fit.hip ----

static int clustered_call(agh_ctx* ctx, const float* xyz, bool on_device, int64_t stride_bytes, int64_t n, const DepthCaptures* depth,
  const char* who, const agh_cluster_params* cp, const agh_localize_params* lp, const ChainOutputs& out,
  agh_localize_batch_result* results, const agh_plane_fit_params* fp = nullptr, bool fitted = false)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  if (fitted && !fp)
  {
    ctx->c.err = std::string(who) + ": fp is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (!cp)
  {
    ctx->c.err = std::string(who) + ": cp is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  return per_object_call(ctx, xyz, on_device, stride_bytes, n, depth, cluster_source(cp, fp, fitted, who), cp->max_objects, lp, out, results);
}

void agh_default_cluster_params(agh_cluster_params* p)
{
  if (!p)
    return;
  *p = agh_cluster_params{ { 0.0, 0.0, 1.0, 0.0 }, 0.01, 0.5, 0.01, 50, 16 };
}

int agh_localize_clustered(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  return clustered_call(ctx, xyz, false, stride_bytes, n, nullptr, "agh_localize_clustered", cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_clustered_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  return clustered_call(ctx, d_xyz, true, stride_bytes, n, nullptr, "agh_localize_clustered_device", cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_depth_clustered(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, &n_images, false, "agh_localize_depth_clustered" };
  return clustered_call(ctx, nullptr, false, 12, 0, &depth, depth.who, cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_depth_clustered_device(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_cluster_params* cp,
  const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, &n_images, true, "agh_localize_depth_clustered_device" };
  return clustered_call(ctx, nullptr, true, 12, 0, &depth, depth.who, cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

void agh_default_plane_fit_params(agh_plane_fit_params* p)
{
  if (!p)
    return;
  *p = agh_plane_fit_params{ 128, 1, 3, 0, 0.01, 1 };
}

int agh_localize_clustered_fit(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n, const agh_plane_fit_params* fp,
  const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  return clustered_call(ctx, xyz, false, stride_bytes, n, nullptr, "agh_localize_clustered_fit", cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, fp, true);
}

int agh_localize_clustered_fit_device(agh_ctx* ctx, const float* d_xyz, int64_t stride_bytes, int64_t n,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out,
  int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  return clustered_call(ctx, d_xyz, true, stride_bytes, n, nullptr, "agh_localize_clustered_fit_device", cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, fp, true);
}

int agh_localize_depth_clustered_fit(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, const agh_plane_fit_params* fp,
  const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, &n_images, false, "agh_localize_depth_clustered_fit" };
  return clustered_call(ctx, nullptr, false, 12, 0, &depth, depth.who, cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, fp, true);
}

int agh_localize_depth_clustered_fit_device(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, agh_handle* handles_out,
  int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, &n_images, true, "agh_localize_depth_clustered_fit_device" };
  return clustered_call(ctx, nullptr, true, 12, 0, &depth, depth.who, cp, lp,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, fp, true);
}

// the last chain collected, if it was a fitted one (`fn` refuses otherwise, and mid-chain)
static int plane_fit_getter_check(Ctx* c, const char* fn)
{
  if (refuse_mid_chain(c, fn))
    return AGH_ERR_STATE;
  if (!c->results.is(SourceKind::FittedClusters, false))
  {
    c->err = std::string(fn) + ": the last chain this context collected was not a fitted one (or there was none)";
    return AGH_ERR_STATE;
  }
  return AGH_OK;
}

int agh_get_plane_fit(agh_ctx* ctx, agh_plane_fit_result* out)
{
  if (!ctx || !out)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = plane_fit_getter_check(c, "agh_get_plane_fit"))
    return rc;
  *out = c->results.fit_results[0];
  return AGH_OK;
}

int agh_get_plane_fit_candidates(agh_ctx* ctx, int32_t* idx, double* planes, int64_t* counts, int32_t cap)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = plane_fit_getter_check(c, "agh_get_plane_fit_candidates"))
    return rc;
  const int C = c->results.fit_candidates[0];
  if ((idx || planes || counts) && cap < C)
  {
    c->err = "agh_get_plane_fit_candidates: cap is below the call's n_candidates";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  // (the candidates stay on the device until somebody asks: a blocking copy each, behind whatever the context's stream holds)
  const PlaneFitBuffers* fb = static_cast<const PlaneFitBuffers*>(c->d_fit);
  AGH_HIPCHK(c, hipStreamSynchronize(c->stream));
  if (idx)
    AGH_HIPCHK(c, hipMemcpy(idx, fb->idx, sizeof(int32_t) * 3 * (size_t) C, hipMemcpyDeviceToHost));
  if (planes)
    AGH_HIPCHK(c, hipMemcpy(planes, fb->planes, sizeof(double) * 4 * (size_t) C, hipMemcpyDeviceToHost));
  if (counts)
  {
    unsigned h[kPlaneFitMaxCandidates];
    AGH_HIPCHK(c, hipMemcpy(h, fb->counts, sizeof(unsigned) * (size_t) C, hipMemcpyDeviceToHost));
    for (int k = 0; k < C; k++)
      counts[k] = (int64_t) h[k];
  }
  return C;
}

// the last chain collected, if it was clustered (`fn` refuses otherwise, and mid-chain)
static int cluster_getter_check(Ctx* c, const char* fn)
{
  if (refuse_mid_chain(c, fn))
    return AGH_ERR_STATE;
  if (!c->results.is_clustered(false))
  {
    c->err = std::string(fn) + ": the last chain this context collected was not clustered (or there was none)";
    return AGH_ERR_STATE;
  }
  return AGH_OK;
}

int agh_get_cluster_info(agh_ctx* ctx, agh_cluster_info* info, int64_t* n_voxels, int32_t* ids, int32_t cap_objects)
{
  if (!ctx || !info)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = cluster_getter_check(c, "agh_get_cluster_info"))
    return rc;
  const ChainResults& R = c->results;
  *info = agh_cluster_info{ R.cluster_info[0][0], R.cluster_info[0][1], R.cluster_info[0][2] };
  if ((n_voxels || ids) && cap_objects < R.lists)
  {
    c->err = "agh_get_cluster_info: cap_objects is below the call's max_objects";
    return AGH_ERR_CAPACITY;
  }
  if (n_voxels)
    std::copy(R.counts, R.counts + R.lists, n_voxels);
  if (ids)
    std::copy(R.cluster_ids, R.cluster_ids + R.lists, ids);
  return AGH_OK;
}

int agh_get_cluster_labels(agh_ctx* ctx, uint8_t* labels_out, int64_t cap)
{
  if (!ctx || (cap > 0 && !labels_out) || cap < 0)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = cluster_getter_check(c, "agh_get_cluster_labels"))
    return rc;
  const int64_t nv = c->results.nv;
  if (cap < nv)
  {
    c->err = "agh_get_cluster_labels: cap is below the cloud's voxel count";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  if (nv > 0)
    AGH_HIPCHK(c, hipMemcpy(labels_out, c->d_cluster_label, (size_t) nv, hipMemcpyDeviceToHost));
  return (int) nv;
}

int agh_get_label_counts(agh_ctx* ctx, int64_t* n_eligible, int32_t cap_objects)
{
  if (!ctx || !n_eligible)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_label_counts"))
    return AGH_ERR_STATE;
  if (!c->results.is(SourceKind::Labels, false))
  {
    c->err = "agh_get_label_counts: the last chain this context collected had no label image (or there was none)";
    return AGH_ERR_STATE;
  }
  if (cap_objects < c->results.lists)
  {
    c->err = "agh_get_label_counts: cap_objects is below the call's n_objects";
    return AGH_ERR_CAPACITY;
  }
  std::copy(c->results.counts, c->results.counts + c->results.lists, n_eligible);
  return AGH_OK;
}

int agh_get_sample_mask_count(agh_ctx* ctx, int64_t* n_eligible)
{
  if (!ctx || !n_eligible)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_sample_mask_count"))
    return AGH_ERR_STATE;
  if (!c->results.is(SourceKind::Mask, false))
  {
    c->err = "agh_get_sample_mask_count: the last chain this context collected had no mask (or there was none)";
    return AGH_ERR_STATE;
  }
  *n_eligible = c->results.counts[0];
  return AGH_OK;
}

// The NEXT capture up, beside the chain in flight (stage_captures, for a set of one).
int agh_localize_stage(agh_ctx* ctx, const float* xyz, int64_t stride_bytes, int64_t n)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  if (bad_capture(xyz, stride_bytes, n))
  {
    ctx->c.err = "agh_localize_stage: bad arguments";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  return stage_captures(ctx, "agh_localize_stage", &xyz, &stride_bytes, &n, 1, false);
}

}  // extern "C"
