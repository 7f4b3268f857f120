// localize_batch.hip -- agh_localize over a batch of captures in one call (agh_localize_batch / agh_localize_batch_device of
// include/agh.h).  The captures are voxelised together, one launch per stage with the capture on blockIdx.y (voxelize.hip,
// vox_batch), into one common voxel array (capture k at the device-side offsets d_cloud_off[k], d_cloud_off[k + 1], written by the
// voxeliser itself), bound as a batch of clouds with a grid build
// sized from the raw counts, searched and classified in one launch set, compacted one work-group per capture, and handed to the
// handle search one list per capture side by side (blockIdx.y).  Nothing but the end of the call waits for the device.
#include "agh_internal.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace agh;

namespace agh
{
// (BatchCapture, one capture of the batch as the device sees it: agh_internal.h)
constexpr int kBatchCountsStride = 8;  // ints of host-side counts per capture (as agh_localize's [0..6])

// one batch, from agh_localize_batch_begin to agh_localize_batch_end: the caller's arrays are copied (explicit sample lists into
// the pinned h_samples, where lp[k].sample_idx then points), the captures themselves are read where d_raw says
// C captures and L lists: preprocessing, grid, bound batch and raw offsets run over the captures; sample spans, the kept-hand
// compaction, the handle search, the collection and the outputs over the lists.  Without labels L = C and list k is capture k; a
// labelled batch has a list per (capture, object) in capture order; the labelled single chain (labeled_tail_prepare) is C = 1.
struct BatchCall
{
  int C = 0, L = 0;
  std::vector<int> list_cap, list_obj;  // L: list l's capture and its object there
  std::vector<const float*> d_raw;
  std::vector<int64_t> dev_stride, n, soff, raw_off;  // raw_off: each capture's first point among all the batch's
  std::vector<agh_localize_params> lp;
  int64_t S_tot = 0, n_tot = 0, slot = 0;
  bool classify = false, filters = false;
  double x1 = 0.0, x2 = 0.0;
  // What the samples are drawn under (agh_localize_batch_masked*, _labeled*, _clustered*, _clustered_fit*), as a repeat of the pass
  // reads it: capture k's bytes in the state's d_mask at raw_off[k] or in the caller's device memory, and copies of the records;
  // first_list: the exclusive prefix sum of the captures' objects
  StoredSource source;
  std::vector<int32_t> first_list;
  bool per_object() const { return source.per_object(); }  // (a list per (capture, object))
  const char* who() const { return source.who; }  // the chain's name in the texts of the errors found behind a synchronisation
};

struct LocalizeBatchState
{
  BatchCall call;                 // the batch in flight (loc.active && loc.batch), or the last one
  BatchCapture* d_tab = nullptr;  // kMaxClouds
  BatchCapture* h_tab = nullptr;  // pinned
  int32_t* d_local = nullptr;     // explicit sample lists, capture-local (s_cap entries)
  int32_t* h_samples = nullptr;   // pinned: the lists, capture-local (explicit: copied in; drawn: written by the device)
  int64_t s_cap = 0;
  int* h_counts = nullptr;        // pinned: kMaxClouds x kBatchCountsStride
  int* h_bad = nullptr;           // pinned: kMaxClouds flags, a capture with a sample index outside its cloud
  VoxDesc* h_desc = nullptr;      // pinned: kMaxClouds voxel descriptors
  // the batched preprocessing: capture table, descriptors, raw block counts, and a bitmap slot of slot_words words per capture
  VoxCapture* d_vcap = nullptr;   // kMaxClouds
  VoxCapture* h_vcap = nullptr;   // pinned
  VoxDesc* d_vdesc = nullptr;     // kMaxClouds
  int* d_blk = nullptr;
  int64_t blk_cap = 0;
  unsigned* d_bitmap = nullptr;   // bitmap_slots x slot_words
  unsigned* d_pruned = nullptr;   // agh_set_voxel_filter: k_vox_prune's output, as large; swapped with d_bitmap once queued
  int64_t pruned_words = 0;
  int* d_blk2 = nullptr;          // bitmap_slots x slot_words / 4096
  int64_t slot_words = 0, bitmap_words = 0, last_words = 0;
  // the handle search's lists, slot hands per capture
  HandleBufs d{};
  int* d_count = nullptr;         // kMaxClouds kept-hand counts
  int64_t slot = 0, slots = 0;
  agh_hypothesis* h_hands = nullptr;  // pinned: slots x slot each
  agh_handle* h_handles = nullptr;
  int32_t* h_idx = nullptr;
  int64_t h_slot = 0, h_slots = 0;
  // sample masks (sample_mask.hip, sample_mask_stage_batch), made by the first masked batch
  uint8_t* d_mask = nullptr;          // the chain's copy of host masks and of depth masks, packed: capture k's at raw_off[k]
  int64_t mask_cap = 0;               // bytes
  const uint8_t** d_mptr = nullptr;   // kMaxClouds: where each capture's mask lies
  const uint8_t** h_mptr = nullptr;   // pinned
  unsigned* d_elig = nullptr;         // eligibility slots, the voxel bitmap slots' layout
  int* d_eblk = nullptr;              // their block counts, then capture-local prefixes
  int64_t elig_words = 0;
  long long* d_mtotal = nullptr;      // kMaxClouds: the M_k
  long long* h_mtotal = nullptr;      // pinned, written by the chain
  int32_t* d_elist = nullptr;         // the E_k, capture k's at raw_off[k]
  int64_t elist_cap = 0;
  // label images (sample_labels.hip, sample_label_stage_batch), made by the first labelled batch; the labels travel as masks do
  // (d_mask, d_mptr), the stage's own buffers are the context's
  LabelCapture* d_lcap = nullptr;     // kMaxClouds
  LabelCapture* h_lcap = nullptr;     // pinned
  // clusters (sample_cluster.hip, sample_cluster_stage_batch), made by the first clustered batch: the captures' records as the
  // kernels take them; the lists' table is the labelled batch's (d_lcap), the stage's own buffers are the context's
  ClusterDev* d_ccap = nullptr;       // kMaxClouds
  ClusterDev* h_ccap = nullptr;       // pinned
  // fitted planes (plane_fit.hip, plane_fit_stage_batch), made by the first fitted batch: a block of candidates, counts and sums
  // per capture, the captures' parameters as the kernels take them, and the result records the chain writes
  PlaneFitBuffers* d_fit = nullptr;        // kMaxClouds
  PlaneFitDev* d_fcap = nullptr;           // kMaxClouds
  PlaneFitDev* h_fcap = nullptr;           // pinned
  agh_plane_fit_result* h_fit_result = nullptr;  // pinned: kMaxClouds
};

void localize_batch_release(Ctx* c)
{
  LocalizeBatchState* b = c->lbatch;
  if (!b)
    return;
  void* dev[] = { b->d_tab, b->d_local, b->d.hands, b->d.bits, b->d.rowcnt, b->d.first, b->d.n, b->d.idx, b->d.counts, b->d.tmp,
    b->d.handles, b->d_count, b->d_vcap, b->d_vdesc, b->d_blk, b->d_bitmap, b->d_pruned, b->d_blk2, b->d_mask, b->d_mptr, b->d_elig, b->d_eblk, b->d_mtotal, b->d_elist, b->d_lcap, b->d_ccap, b->d_fit, b->d_fcap };
  for (void* p : dev)
    if (p)
      (void) hipFree(p);
  void* host[] = { b->h_tab, b->h_samples, b->h_counts, b->h_bad, b->h_desc, b->h_hands, b->h_handles, b->h_idx, b->h_vcap, b->h_mptr, b->h_mtotal, b->h_lcap, b->h_ccap, b->h_fcap, b->h_fit_result };
  for (void* p : host)
    if (p)
      (void) hipHostFree(p);
  delete b;
  c->lbatch = nullptr;
}
}  // namespace agh

namespace
{
// The batch's sample list: position j belongs to the capture whose span holds it.  Drawn: agh_localize's strata over that
// capture's voxel count (localize.hip, k_draw_samples) with its seed; explicit: the caller's capture-local index, validated
// against the capture's own voxel count.  Either way the search gets the index into the common voxel array (or kSampleSkip;
// -1 for an index outside the capture: the search flags it), the host the capture-local one.
__global__ void k_batch_samples(const BatchCapture* __restrict__ tab, int C, int64_t S_tot, const int* __restrict__ cloud_off,
  const int32_t* __restrict__ local, int32_t* __restrict__ out, int32_t* __restrict__ host_out, int* __restrict__ bad)
{
  const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= S_tot)
    return;
  int k = 0;
  for (int q = 1; q < C; q++)  // (the last capture whose span starts at or before j and is not empty)
    if (tab[q].soff <= j && tab[q].S > 0)
      k = q;
  const int64_t t = j - tab[k].soff;
  const int S = tab[k].S;
  const long long base = cloud_off[k], N = cloud_off[k + 1] - base;
  int32_t v, g;
  if (tab[k].drawn)
  {
    v = draw_stratum(N, S, (long long) t, tab[k].seed);
    host_out[j] = v;
    g = v == kSampleSkip ? v : (int32_t) (v + base);
  }
  else
  {
    v = local[j];
    if (v == kSampleSkip)
      g = v;
    else if (v >= 0 && v < N)
      g = (int32_t) (v + base);
    else
    {
      g = -1;
      bad[k] = 1;
    }
  }
  out[j] = g;
}

// k_compact_kept (localize.hip) once per capture, one work-group each around the same compact_kept_records (agh_internal.h):
// capture k's hypotheses are the contiguous run of the batch's list whose samples lie in its span (the list is in sample order),
// its kept hands go to its own slot -- on the device and in pinned host memory -- with `sample` made capture-local.  filters: the
// boundary filter against the capture's own workspace (the classifier ran on every hypothesis of the batch).  host_counts:
// kBatchCountsStride ints per capture, [4] hypotheses, [5] kept, [6] the search's error word.
__global__ __launch_bounds__(1024) void k_compact_kept_batch(const agh_hypothesis* __restrict__ in, const int64_t* __restrict__ n_in,
  int64_t cap_in, int use_keep, int filters, const BatchCapture* __restrict__ tab, agh_hypothesis* __restrict__ out, int slot,
  int* __restrict__ n_out, agh_hypothesis* __restrict__ host_out, int host_slot, int* __restrict__ host_counts,
  const int32_t* __restrict__ flags, const uint8_t* __restrict__ drop, const unsigned* __restrict__ hf_counts, int* __restrict__ hf_host,
  MarginOut mg)
{
  __shared__ int src[kCompactList];
  __shared__ int wsum[16];
  __shared__ int carry;
  __shared__ int64_t range[2];
  const int cap = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t n = min(*n_in, cap_in);
  const int64_t s0 = tab[cap].soff, s1 = s0 + tab[cap].S;
  if (tid < 2)
  {
    // first record whose sample is at or beyond the bound
    const int64_t bound = tid == 0 ? s0 : s1;
    int64_t lo = 0, hi = n;
    while (lo < hi)
    {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t) in[mid].sample < bound)
        lo = mid + 1;
      else
        hi = mid;
    }
    range[tid] = lo;
  }
  __syncthreads();
  const int64_t r0 = range[0], r1 = range[1];
  double ws[6];
  for (int q = 0; q < 6; q++)
    ws[q] = tab[cap].ws[q];
  const int room = min(slot, host_slot);
  const int K = compact_kept_records(in, r0, r1, use_keep, filters, ws, src, wsum, &carry, out + (int64_t) cap * slot, room,
    host_out + (int64_t) cap * host_slot, room, (int) s0, drop, mg.sums, mg.out ? mg.out + (int64_t) cap * mg.stride : nullptr,
    mg.host ? mg.host + (int64_t) cap * mg.host_stride : nullptr);
  if (drop && tid < kHandDropCounters)  // (the hand drop stage: the list's counters to pinned memory with its counts)
    hf_host[cap * kHandDropCounters + tid] = (int) hf_counts[cap * kHandDropCounters + tid];
  if (tid == 0)
  {
    n_out[cap] = K;
    int* hc = host_counts + cap * kBatchCountsStride;
    hc[4] = (int) (r1 - r0);
    hc[5] = K;
    hc[6] = flags[0] | (*n_in > cap_in ? 2 : 0);
  }
}

template <typename T>
int pinned_alloc(Ctx* c, T** p, size_t count)
{
  if (*p)
  {
    (void) hipHostFree(*p);
    *p = nullptr;
  }
  void* q = nullptr;
  const hipError_t e = hipHostMalloc(&q, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault);
  if (e != hipSuccess)
  {
    c->err = std::string("hipHostMalloc: ") + hipGetErrorString(e);
    return AGH_ERR_HIP;
  }
  *p = static_cast<T*>(q);
  return AGH_OK;
}

// the context's batch state with its tables of kMaxClouds records, made by the first call that needs it
int ensure_batch_state(Ctx* c)
{
  if (c->lbatch)
    return AGH_OK;
  c->lbatch = new LocalizeBatchState();
  LocalizeBatchState* b = c->lbatch;
  int rc;
  if ((rc = dev_alloc(c, &b->d_tab, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_tab, (size_t) kMaxClouds)) ||
      (rc = pinned_alloc(c, &b->h_counts, (size_t) kMaxClouds * kBatchCountsStride)) ||
      (rc = pinned_alloc(c, &b->h_bad, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_desc, (size_t) kMaxClouds)) ||
      (rc = dev_alloc(c, &b->d_count, (size_t) kMaxClouds)) || (rc = dev_alloc(c, &b->d_vcap, (size_t) kMaxClouds)) ||
      (rc = pinned_alloc(c, &b->h_vcap, (size_t) kMaxClouds)) || (rc = dev_alloc(c, &b->d_vdesc, (size_t) kMaxClouds)))
  {
    localize_batch_release(c);
    return rc;
  }
  return AGH_OK;
}

// the sample lists of the chain: S_tot entries, capture-local, on the device (explicit lists) and pinned
int ensure_batch_samples(Ctx* c, LocalizeBatchState* b, int64_t S_tot)
{
  if (S_tot > b->s_cap || !b->h_samples)
  {
    const int64_t cap = std::max<int64_t>(S_tot, 1024);
    int rc;
    if ((rc = dev_alloc(c, &b->d_local, (size_t) cap)) || (rc = pinned_alloc(c, &b->h_samples, (size_t) cap)))
      return rc;
    b->s_cap = cap;
  }
  return AGH_OK;
}

// the handle search's slots: C lists of `slot` hands (device), and their pinned mirrors
int ensure_batch_slots(Ctx* c, LocalizeBatchState* b, int C, int64_t slot)
{
  slot = std::max<int64_t>(slot, 64);
  if (slot > b->slot || C > b->slots || !b->d.hands)
  {
    const int64_t sl = std::max(slot, b->slot), ns = std::max<int64_t>(C, b->slots);
    const size_t n = (size_t) (sl * ns);
    int rc;
    if ((rc = dev_alloc(c, &b->d.hands, n)) || (rc = dev_alloc(c, &b->d.bits, n * (size_t) ((sl + 63) / 64))) ||
        (rc = dev_alloc(c, &b->d.rowcnt, n)) || (rc = dev_alloc(c, &b->d.first, n)) || (rc = dev_alloc(c, &b->d.n, n)) ||
        (rc = dev_alloc(c, &b->d.idx, n)) || (rc = dev_alloc(c, &b->d.counts, (size_t) ns * 4)) || (rc = dev_alloc(c, &b->d.tmp, n)) ||
        (rc = dev_alloc(c, &b->d.handles, n)))
      return rc;
    b->slot = sl;
    b->slots = ns;
  }
  if (slot > b->h_slot || C > b->h_slots || !b->h_hands)
  {
    const int64_t sl = std::max(slot, b->h_slot), ns = std::max<int64_t>(C, b->h_slots);
    const size_t n = (size_t) (sl * ns);
    int rc;
    if ((rc = pinned_alloc(c, &b->h_hands, n)) || (rc = pinned_alloc(c, &b->h_handles, n)) || (rc = pinned_alloc(c, &b->h_idx, n)))
      return rc;
    b->h_slot = sl;
    b->h_slots = ns;
  }
  return AGH_OK;
}

// C bitmap slots of b->slot_words words (+ one popcount block of slack) and their popcount tables
int ensure_vox_slots(Ctx* c, LocalizeBatchState* b, int C)
{
  const int64_t need = (int64_t) C * b->slot_words;
  if (need > b->bitmap_words || !b->d_bitmap)
  {
    int rc;
    if ((rc = dev_alloc(c, &b->d_bitmap, (size_t) need + 4096)) || (rc = dev_alloc(c, &b->d_blk2, (size_t) (need / 4096) + 1)))
    {
      b->bitmap_words = 0;
      return rc;
    }
    b->bitmap_words = need;
  }
  // (agh_set_voxel_filter: the second set of slots, made by the first filtered batch and regrown with the first set)
  if (c->voxel_filter_set && (b->pruned_words != b->bitmap_words || !b->d_pruned))
  {
    b->pruned_words = 0;
    if (int rc = dev_alloc(c, &b->d_pruned, (size_t) b->bitmap_words + 4096))
      return rc;
    b->pruned_words = b->bitmap_words;
  }
  return AGH_OK;
}

// a masked batch's buffers: the mask table, the M_k, eligibility slots as large as the voxel slots, one list entry per raw point
int ensure_mask_slots(Ctx* c, LocalizeBatchState* b, int64_t n_tot)
{
  int rc;
  // (all four or none: a table that failed half-way is made again by the next masked batch)
  if ((!b->d_mptr || !b->h_mptr || !b->d_mtotal || !b->h_mtotal) &&
      ((rc = dev_alloc(c, &b->d_mptr, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_mptr, (size_t) kMaxClouds)) ||
       (rc = dev_alloc(c, &b->d_mtotal, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_mtotal, (size_t) kMaxClouds))))
    return rc;
  if (b->bitmap_words > b->elig_words || !b->d_elig)
  {
    b->elig_words = 0;
    if ((rc = dev_alloc(c, &b->d_elig, (size_t) b->bitmap_words + 4096)) || (rc = dev_alloc(c, &b->d_eblk, (size_t) (b->bitmap_words / 4096) + 1)))
      return rc;
    b->elig_words = b->bitmap_words;
  }
  if (n_tot > b->elist_cap || !b->d_elist)
  {
    b->elist_cap = 0;
    if ((rc = dev_alloc(c, &b->d_elist, (size_t) std::max<int64_t>(n_tot, 1024))))
      return rc;
    b->elist_cap = std::max<int64_t>(n_tot, 1024);
  }
  return AGH_OK;
}

// a labelled batch's tables: where each capture's labels lie, and its lists
int ensure_label_tables(Ctx* c, LocalizeBatchState* b)
{
  int rc;
  if ((!b->d_mptr || !b->h_mptr) &&
      ((rc = dev_alloc(c, &b->d_mptr, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_mptr, (size_t) kMaxClouds))))
    return rc;
  if ((!b->d_lcap || !b->h_lcap) &&
      ((rc = dev_alloc(c, &b->d_lcap, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_lcap, (size_t) kMaxClouds))))
    return rc;
  return AGH_OK;
}

// a clustered batch's tables: its lists, and the captures' cluster records
int ensure_cluster_tables(Ctx* c, LocalizeBatchState* b)
{
  int rc;
  if ((!b->d_lcap || !b->h_lcap) &&
      ((rc = dev_alloc(c, &b->d_lcap, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_lcap, (size_t) kMaxClouds))))
    return rc;
  if ((!b->d_ccap || !b->h_ccap) &&
      ((rc = dev_alloc(c, &b->d_ccap, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_ccap, (size_t) kMaxClouds))))
    return rc;
  return AGH_OK;
}

// a fitted batch's tables: a block per capture, the captures' parameters, the results
int ensure_fit_tables(Ctx* c, LocalizeBatchState* b)
{
  int rc;
  if ((!b->d_fit || !b->d_fcap || !b->h_fcap || !b->h_fit_result) &&
      ((rc = dev_alloc(c, &b->d_fit, (size_t) kMaxClouds)) || (rc = dev_alloc(c, &b->d_fcap, (size_t) kMaxClouds)) ||
       (rc = pinned_alloc(c, &b->h_fcap, (size_t) kMaxClouds)) || (rc = pinned_alloc(c, &b->h_fit_result, (size_t) kMaxClouds))))
    return rc;
  return AGH_OK;
}

// A per-capture host table (pinned) up to its device twin, queued on st; a failure has drained the stream (chain_fail).
template <typename T>
int table_to_device(Ctx* c, T* d_table, const T* h_table, int count, hipStream_t st)
{
  AGH_HIPCHK_OR(c, hipMemcpyAsync(d_table, h_table, sizeof(T) * (size_t) count, hipMemcpyHostToDevice, st), chain_fail(c, AGH_ERR_HIP));
  return AGH_OK;
}

// The list table of the call, on the host and queued to the device: list l's span of the sample list, its capture's sample
// count, seed and workspace (B.lp[list_cap[l]]), and which object of it the list is.
int fill_list_table(Ctx* c, LocalizeBatchState* b, hipStream_t st)
{
  const BatchCall& B = b->call;
  for (int l = 0; l < B.L; l++)
  {
    const agh_localize_params& p = B.lp[(size_t) B.list_cap[l]];
    BatchCapture& t = b->h_tab[l];
    t.soff = B.soff[l];
    t.S = (int32_t) p.n_samples;
    t.drawn = p.sample_idx ? 0 : 1;  // (a masked or labelled chain has no explicit list)
    t.seed = p.sample_seed;
    for (int q = 0; q < 6; q++)
      t.ws[q] = p.workspace[q];
    t.capture = B.list_cap[l];
    t.object = B.list_obj[l];
    b->h_bad[l] = 0;
  }
  AGH_HIPCHK(c, hipMemcpyAsync(b->d_tab, b->h_tab, sizeof(BatchCapture) * (size_t) B.L, hipMemcpyHostToDevice, st));
  return AGH_OK;
}

}  // namespace

// search -> classification -> per-capture compaction -> handle search, queued (handles_only: the handle search once more); the
// labelled chain of localize.hip queues its tail with this too, one list per object (agh_internal.h)
int batch_queue(agh_ctx* ctx, bool handles_only)
{
  Ctx* c = &ctx->c;
  LocalizeBatchState* b = c->lbatch;
  const BatchCall& B = b->call;
  hipStream_t st = c->stream;
  const int C = B.L;  // (the lists)
  int rc;
  for (int k = 0; k < C; k++)
    for (int q = 0; q < (handles_only ? 4 : kBatchCountsStride); q++)
      b->h_counts[k * kBatchCountsStride + q] = 0;
  c->loc.with_sequential = c->handles_sequential;
  if (!handles_only)
  {
    c->mirror = HostMirror{ nullptr, 0, nullptr };
    if ((rc = agh_find_hands_device(ctx, c->d_idx_own, B.S_tot, 0, c->d_out_own, c->s_cap * 8, c->d_nout, st)) != AGH_OK)
      return rc;
    // (the hand drop stage as in localize_queue, with the list table to find a hand's list, capture and views)
    const int64_t hyp_bound = std::min<int64_t>(c->last_s * 8, c->last_cap);
    const HandDropView hd = hand_drop_stage(c, hyp_bound, b->d_tab, C, st);
    if (hd.rc != AGH_OK)
      return hd.rc;
    if (B.classify && (rc = hog_svm(c, hyp_bound, c->d_keep, st, nullptr, hd.drop)) != AGH_OK)
      return rc;
    // (agh_set_handle_ranking: the kept hands' margins leave with them, list by list; nothing without one)
    MarginOut mg;
    if ((rc = handle_rank_prepare(c, C, b->slot, b->h_slot, B.classify, &mg)) != AGH_OK)
      return rc;
    hipLaunchKernelGGL(k_compact_kept_batch, dim3(C), dim3(1024), 0, st, (const agh_hypothesis*) c->d_out_own,
      (const int64_t*) c->d_nout, c->s_cap * 8, B.classify ? 1 : 0, B.filters ? 1 : 0, (const BatchCapture*) b->d_tab, b->d.hands,
      (int) b->slot, b->d_count, b->h_hands, (int) b->h_slot, b->h_counts, (const int32_t*) c->d_flags, hd.drop,
      hd.d_counts, hd.h_counts, mg);
    if (hipGetLastError() != hipSuccess)
    {
      c->err = "k_compact_kept_batch launch failed";
      return AGH_ERR_HIP;
    }
  }
  const HandleMirror hm{ b->h_handles, (int) b->h_slot, b->h_idx, (int) b->h_slot, b->h_counts };
  timing_begin(c, st);
  rc = handle_search_batch(b->d, C, b->slot, B.slot, B.x1, B.x2, B.lp[0].min_inliers, B.lp[0].min_length, st, hm,
    kBatchCountsStride, c->loc.with_sequential, b->d_count);
  timing_mark(c, "handle_search", st);
  if (rc != AGH_OK)
  {
    c->err = "handle search launch failed";
    return rc;
  }
  return handle_rank_stage(c, b->d, C, b->slot, hm, kBatchCountsStride, st);
}

namespace
{
struct ActiveGuard
{
  Ctx* c;
  explicit ActiveGuard(Ctx* c_) : c(c_) { c->batch_active = true; }
  ~ActiveGuard() { c->batch_active = false; }
};

const char* const kBadArguments = "agh_localize_batch: bad arguments (1 <= n_captures <= 64; see include/agh.h)";

// Steps 2 to 5 of the batch c->lbatch->call, queued on the context's stream: preprocessing, the batch of clouds, the sample list,
// search -> classification -> kept hands per capture -> handle search.  Nothing waits, except the first batch of a context (or one
// after the kept slots were dropped): one synchronisation for the lattice sizes.  An error has drained the stream (chain_fail).
int batch_pass(agh_ctx* ctx)
{
  Ctx* c = &ctx->c;
  LocalizeBatchState* b = c->lbatch;
  BatchCall& B = b->call;
  hipStream_t st = c->stream;
  const int C = B.C;
  const int64_t n_tot = B.n_tot, S_tot = B.S_tot;
  const std::vector<int64_t>& n = B.n;
  std::vector<agh_localize_params>& lp = B.lp;
  const double cell = lp[0].cell_size;
  int rc;
  // ---- 2. preprocessing: one launch per stage for the whole batch, capture = blockIdx.y, each with its own descriptor and
  // bitmap slot; the voxels of all captures go to one array at the device-side cloud offsets ----
  if (n_tot > c->vox_cap || !c->d_vox_code)
  {
    if ((rc = dev_alloc(c, &c->d_vox_code, (size_t) n_tot)) || (rc = dev_alloc(c, &c->d_vox_blk, (size_t) n_tot / 1024 + 2)) ||
        (rc = dev_alloc(c, &c->d_vox_xyz, (size_t) n_tot * 3)) || (rc = dev_alloc(c, &c->d_vox_cam, (size_t) n_tot)))
      return chain_fail(c, rc);
    c->vox_cap = n_tot;
  }
  int64_t nb_max = 0, n_max = 0, blk_tot = 0;
  bool any_scan = false;
  for (int k = 0; k < C; k++)
  {
    VoxCapture& q = b->h_vcap[k];
    q.xyz = B.d_raw[k];
    q.stride = B.dev_stride[k] / 4;
    q.n = n[k];
    q.size_left = lp[k].size_left;
    for (int a = 0; a < 3; a++)
    {
      q.ws.lo[a] = lp[k].workspace[2 * a];
      q.ws.hi[a] = lp[k].workspace[2 * a + 1];
    }
    q.blk_off = blk_tot;
    q.code_off = B.raw_off[k];
    q.dense = lp[k].dense ? 1 : 0;
    q.pad = 0;
    const int64_t nb = (n[k] + 1023) / 1024;
    blk_tot += nb;
    nb_max = std::max(nb_max, nb);
    n_max = std::max(n_max, n[k]);
    any_scan |= n[k] > 0 && !lp[k].dense;
  }
  if (blk_tot + 1 > b->blk_cap || !b->d_blk)
  {
    if ((rc = dev_alloc(c, &b->d_blk, (size_t) blk_tot + 1)))
      return chain_fail(c, rc);
    b->blk_cap = blk_tot + 1;
  }
  AGH_HIPCHK_OR(c, hipMemcpyAsync(b->d_vcap, b->h_vcap, sizeof(VoxCapture) * (size_t) C, hipMemcpyHostToDevice, st), chain_fail(c, AGH_ERR_HIP));
  VoxBatch vb;
  vb.cap = b->d_vcap;
  vb.desc = b->d_vdesc;
  vb.host_desc = b->h_desc;
  // (slots kept from much larger lattices are dropped: every capture would clear and count all of its slot)
  if (b->d_bitmap && b->last_words > 0 && b->slot_words > 8 * b->last_words + (1 << 20))
    b->slot_words = 0;
  if (b->slot_words <= 0)
  {
    // the first batch of a context: the lattices' sizes (one synchronisation) decide the slots
    if ((rc = vox_batch(vb, C, nb_max, n_max, any_scan, cell, true, nullptr, b->d_blk, nullptr, c->d_vox_code, nullptr, nullptr,
           nullptr, st)) != AGH_OK)
    {
      c->err = "preprocessing launch failed";
      return chain_fail(c, rc);
    }
    AGH_HIPCHK_OR(c, hipStreamSynchronize(st), chain_fail(c, AGH_ERR_HIP));
    int64_t words = 0;
    for (int k = 0; k < C; k++)
    {
      if (b->h_desc[k].error)
      {
        c->err = std::string(B.who()) + ": capture " + std::to_string(k) + ": the voxel lattice of the kept points exceeds 2^33 cells "
                 "(1 GiB bitmap): set a workspace that bounds the scene";
        return chain_fail(c, AGH_ERR_CAPACITY);
      }
      words = std::max<int64_t>(words, (int64_t) b->h_desc[k].n_words);
    }
    b->slot_words = std::min<int64_t>(((words + words / 4) / 4096 + 1) * 4096, (int64_t) kVoxMaxWords);
  }
  if ((rc = ensure_vox_slots(c, b, C)) != AGH_OK)
    return chain_fail(c, rc);
  vb.slot_words = b->slot_words;
  timing_begin(c, st);
  if ((rc = vox_batch(vb, C, nb_max, n_max, any_scan, cell, false, b->d_bitmap, b->d_blk, b->d_blk2, c->d_vox_code, c->d_vox_xyz,
         c->d_vox_cam, c->d_cloud_off, st, b->d_pruned, c->voxel_filter_set ? &c->voxel_filter : nullptr)) != AGH_OK)
  {
    c->err = "preprocessing launch failed";
    return chain_fail(c, rc);
  }
  c->vox_filter_captures = 0;
  if (c->voxel_filter_set)
  {
    std::swap(b->d_bitmap, b->d_pruned);  // (queued: "the" bitmap of the batch is the pruned one to every later stage)
    c->vox_filter_captures = C;
    c->vox_filter_mirror = b->h_desc;
  }
  timing_mark(c, "preprocess", st);
  c->cloud_async = false;
  // ---- 3. the batch of clouds: a grid build sized from the raw counts (bounds of the voxel counts, which stay on the device) ----
  {
    std::vector<int64_t> bound(C + 1, 0);
    for (int k = 0; k < C; k++)
      bound[k + 1] = bound[k] + n[k];
    c->defer_cloud_count = true;
    rc = agh_set_cloud_batch_device(ctx, c->d_vox_xyz, 12, c->d_vox_cam, bound.data(), C, nullptr);
    c->defer_cloud_count = false;
    if (rc != AGH_OK)
      return chain_fail(c, rc);
  }
  // ---- 4. buffers for the bounds, the capture table and the sample list ----
  if ((rc = ensure_call_buffers(c, std::max<int64_t>(S_tot, 1))) != AGH_OK)
    return chain_fail(c, rc);
  if (S_tot > c->idx_cap || !c->d_idx_own)
  {
    if ((rc = dev_alloc(c, &c->d_idx_own, (size_t) std::max<int64_t>(S_tot, 1024))))
      return chain_fail(c, rc);
    c->idx_cap = std::max<int64_t>(S_tot, 1024);
  }
  if ((rc = ensure_batch_samples(c, b, S_tot)) != AGH_OK)
    return chain_fail(c, rc);
  if ((rc = ensure_batch_slots(c, b, B.L, B.slot)) != AGH_OK)
    return chain_fail(c, rc);
  if (B.classify)
  {
    AGH_HIPCHK_OR(c, ensure_keep_buffers(c, c->s_cap * 8), chain_fail(c, AGH_ERR_HIP));
  }
  bool any_explicit = false;
  for (int k = 0; k < C; k++)
    if (lp[k].sample_idx && lp[k].n_samples > 0)  // (never with masks or labels: list k is capture k)
    {
      any_explicit = true;
      // (the caller's list is copied once: from here on the record names the pinned copy, which a repeat of the batch reads)
      if (lp[k].sample_idx != b->h_samples + B.soff[k])
        std::memcpy(b->h_samples + B.soff[k], lp[k].sample_idx, sizeof(int32_t) * (size_t) lp[k].n_samples);
      lp[k].sample_idx = b->h_samples + B.soff[k];
    }
  if ((rc = fill_list_table(c, b, st)) != AGH_OK)
    return chain_fail(c, rc);
  if (any_explicit)
  {
    AGH_HIPCHK_OR(c, hipMemcpyAsync(b->d_local, b->h_samples, sizeof(int32_t) * (size_t) S_tot, hipMemcpyHostToDevice, st),
      chain_fail(c, AGH_ERR_HIP));
  }
  const StoredSource& src = B.source;
  BatchStageCommon common;  // (what every sample stage is given: the preprocessing and the grid build are queued)
  common.vb = vb;
  common.C = C;
  common.L = B.L;
  common.n_max = n_max;
  common.n_tot = n_tot;
  common.S_tot = S_tot;
  common.cell = cell;
  common.code = c->d_vox_code;
  common.bitmap = b->d_bitmap;
  common.blk2 = b->d_blk2;
  common.cloud_off = c->d_cloud_off;
  common.tab = b->d_tab;
  common.d_out = c->d_idx_own;
  common.h_out = b->h_samples;
  if (src.kind == SourceKind::Mask)  // (for S_tot = 0 too: the M_k are what a caller sizes the S_k with)
  {
    if ((rc = ensure_mask_slots(c, b, n_tot)) != AGH_OK)
      return chain_fail(c, rc);
    std::copy(src.d_bytes.begin(), src.d_bytes.end(), b->h_mptr);
    if ((rc = table_to_device(c, b->d_mptr, b->h_mptr, C, st)) != AGH_OK)
      return rc;
    BatchMaskStage m{ common, b->d_mptr, b->d_elig, b->d_eblk, b->d_mtotal, b->d_elist, b->h_mtotal };
    if ((rc = sample_mask_stage_batch(c, m, st)) != AGH_OK)
      return chain_fail(c, rc);
  }
  else if (src.clustered())  // (for S_tot = 0 too: the objects found are a result of their own)
  {
    if ((rc = ensure_cluster_tables(c, b)) != AGH_OK)
      return chain_fail(c, rc);
    for (int k = 0; k < C; k++)
    {
      b->h_lcap[k] = LabelCapture{ src.n_objects[k], B.first_list[k] };
      b->h_ccap[k] = cluster_dev(src.cluster[k]);
    }
    if ((rc = table_to_device(c, b->d_lcap, b->h_lcap, C, st)) != AGH_OK || (rc = table_to_device(c, b->d_ccap, b->h_ccap, C, st)) != AGH_OK)
      return rc;
    if (src.fitted())  // (behind the records' upload: k_fit_finish_batch writes capture k's plane into d_ccap[k])
    {
      if ((rc = ensure_fit_tables(c, b)) != AGH_OK)
        return chain_fail(c, rc);
      for (int k = 0; k < C; k++)
      {
        // (camera 0's origin in force for capture k: its row of the table, or the context's own; the setter refuses mid-chain)
        const double* o = c->cam_tab_rows == C ? c->h_cam_tab + 6 * k : c->p.cam_origin[0];
        const agh_plane_fit_params& f = src.fit[k];
        b->h_fcap[k] = PlaneFitDev{ f.n_candidates, f.refine, f.min_inliers, 0, f.distance_threshold, (unsigned long long) f.seed,
          { o[0], o[1], o[2] } };
      }
      if ((rc = table_to_device(c, b->d_fcap, b->h_fcap, C, st)) != AGH_OK)
        return rc;
      BatchFitStage f{ common, b->d_fcap, b->d_fit, b->d_ccap, b->h_fit_result };
      if ((rc = plane_fit_stage_batch(c, f, st)) != AGH_OK)
        return chain_fail(c, rc);
    }
    // (no labels: the object sets come from the clouds, behind the grid build queued above)
    BatchLabelStage m{ common, nullptr, b->d_lcap };
    if ((rc = sample_cluster_stage_batch(c, m, b->d_ccap, st)) != AGH_OK)
      return chain_fail(c, rc);
  }
  else if (src.kind == SourceKind::Labels)  // (for S_tot = 0 too, as the masks')
  {
    if ((rc = ensure_label_tables(c, b)) != AGH_OK)
      return chain_fail(c, rc);
    for (int k = 0; k < C; k++)
    {
      b->h_mptr[k] = src.d_bytes[k];
      b->h_lcap[k] = LabelCapture{ src.n_objects[k], B.first_list[k] };
    }
    if ((rc = table_to_device(c, b->d_mptr, b->h_mptr, C, st)) != AGH_OK || (rc = table_to_device(c, b->d_lcap, b->h_lcap, C, st)) != AGH_OK)
      return rc;
    BatchLabelStage m{ common, b->d_mptr, b->d_lcap };
    if ((rc = sample_label_stage_batch(c, m, st)) != AGH_OK)
      return chain_fail(c, rc);
  }
  else if (S_tot > 0)
  {
    hipLaunchKernelGGL(k_batch_samples, dim3((unsigned) ((S_tot + 255) / 256)), dim3(256), 0, st, (const BatchCapture*) b->d_tab, C,
      S_tot, (const int*) c->d_cloud_off, (const int32_t*) b->d_local, c->d_idx_own, b->h_samples, b->h_bad);
    AGH_HIPCHK_OR(c, hipGetLastError(), chain_fail(c, AGH_ERR_HIP));
  }
  // ---- 5. search -> classification -> kept hands per capture -> handle search ----
  if ((rc = batch_queue(ctx, false)) != AGH_OK)
    return chain_fail(c, rc);
  return AGH_OK;
}

// agh_localize_batch_begin: the arguments checked and copied, the captures up (or adopted from agh_localize_batch_stage, or read in
// place), steps 2 to 5 queued.
int batch_begin_impl(agh_ctx* ctx, const float* const* xyz, bool on_device, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures, const DepthCaptures* depth = nullptr, const SampleSource* src = nullptr)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  const int C = n_captures;
  const std::string who = src ? src->who : (depth ? depth->who : "agh_localize_batch");
  if (L.active)
  {
    c->err = who + ": a localize chain is in flight on this context (agh_localize_end first)";
    return AGH_ERR_STATE;
  }
  std::vector<int64_t> depth_first, depth_left0, depth_n;
  std::vector<agh_localize_params> depth_lp;
  if (depth)
  {
    // (the arguments of the images first: their sizes are the captures'; then size_left and dense as include/agh.h fixes them)
    if (int rc = depth_batch_check(c, depth->who, depth->images, depth->n_images, C, depth->on_device, &depth_first, &depth_left0))
      return rc;
    if (!lp)
    {
      c->err = who + ": lp is NULL";
      return AGH_ERR_INVALID_ARGUMENT;
    }
    depth_lp.assign(lp, lp + C);
    depth_n.resize((size_t) C);
    for (int k = 0; k < C; k++)
    {
      depth_lp[k].size_left = depth_left0[k];
      depth_lp[k].dense = 1;
      depth_n[k] = depth_first[k + 1] - depth_first[k];
    }
    lp = depth_lp.data();
    n = depth_n.data();
    on_device = false;  // (the chain reads the context's raw buffer, whichever memory the images lie in)
  }
  else if (C < 1 || C > kMaxClouds || !xyz || !stride_bytes || !n || !lp)
  {
    c->err = src ? who + ": bad arguments (1 <= n_captures <= 64; see include/agh.h)" : std::string(kBadArguments);
    return AGH_ERR_INVALID_ARGUMENT;
  }
  int64_t n_tot = 0, S_tot = 0;
  for (int k = 0; k < C; k++)
  {
    const agh_localize_params& p = lp[k];
    if ((!depth && bad_capture(xyz[k], stride_bytes[k], n[k])) || !(p.cell_size > 0.0) || p.size_left < 0 || p.n_samples < 0 ||
        p.n_samples > (1 << 24) || p.min_inliers < 1 || (p.filters_boundaries != 0 && p.filters_boundaries != 1))
    {
      c->err = who + ": bad arguments for capture " + std::to_string(k) + " (see include/agh.h)";
      return AGH_ERR_INVALID_ARGUMENT;
    }
    if (p.classify != lp[0].classify || p.cell_size != lp[0].cell_size || p.min_inliers != lp[0].min_inliers ||
        p.min_length != lp[0].min_length || p.filters_boundaries != lp[0].filters_boundaries)
    {
      c->err = who + ": classify, cell_size, min_inliers, min_length and filters_boundaries must be equal across the "
               "batch (capture " + std::to_string(k) + " differs from capture 0)";
      return AGH_ERR_INVALID_ARGUMENT;
    }
    n_tot += n[k];
    S_tot += p.n_samples;
  }
  const bool per_object = src && src->per_object();
  if (per_object)  // (before the sums' limits: such a batch counts its samples per list, and says which capture went too far)
  {
    if (int rc = sample_source_check(c, *src, depth, lp, C, false))
      return rc;
    S_tot = 0;
    for (int k = 0; k < C; k++)
      S_tot += (int64_t) src->objects(k) * lp[k].n_samples;
  }
  if (n_tot >= (1ll << 30) || S_tot > (1 << 24))
  {
    c->err = who + ": need fewer than 2^30 raw points and at most 2^24 samples in all";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (lp[0].classify && !c->has_svm)
  {
    c->err = who + ": classify needs a loaded SVM (agh_load_svm*)";
    return AGH_ERR_NO_SVM;
  }
  // (agh_set_hand_filter's observed-space criterion reads the batch's depth images)
  if (int rc = hand_filter_check(c, who.c_str(), depth ? depth->images : nullptr, depth ? depth->n_images : nullptr, depth ? C : 0,
        depth != nullptr))
    return rc;
  if (int rc = handle_rank_check(c, who.c_str(), lp[0].classify != 0))
    return rc;
  if (cam_table_mismatch(c, who.c_str(), C))  // (capture k = cloud k: row k of agh_set_cloud_cam_origins' table is its rig;
    return AGH_ERR_INVALID_ARGUMENT;                    // the table stays the context's until agh_localize_batch_end: the setter
                                                        // refuses mid-chain, so the repeats search with it too)
  if (src && !per_object)  // (a mask adds nothing to the sums: its rules come behind the limits and the origin table)
    if (int rc = sample_source_check(c, *src, depth, lp, C, false))
      return rc;
  double x1 = 0.0, x2 = 0.0;
  if (!handle_thresholds(&x1, &x2))
  {
    c->err = who + ": this libm's acos is not monotone around the 0.34 rad thresholds";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  int rc;
  if ((rc = ensure_batch_state(c)) != AGH_OK)
    return rc;
  LocalizeBatchState* b = c->lbatch;
  BatchCall& B = b->call;
  B = BatchCall();
  B.C = C;
  B.x1 = x1;
  B.x2 = x2;
  // ---- 1. the raw captures: packed end to end into the context's raw buffer, or read in place ----
  B.d_raw.resize(C);
  B.dev_stride.resize(C);
  B.n.assign(n, n + C);
  B.lp.assign(lp, lp + C);
  B.raw_off.resize(C);
  for (int k = 0, o = 0; k < C; o += (int) n[k], k++)
    B.raw_off[k] = o;
  for (int k = 0; k < C; k++)
  {
    const int K = per_object ? src->objects(k) : 1;
    if (per_object)
      B.first_list.push_back((int32_t) B.list_cap.size());
    for (int j = 0; j < K; j++)
    {
      B.list_cap.push_back(k);
      B.list_obj.push_back(j);
    }
  }
  B.L = (int) B.list_cap.size();
  B.source.keep(src, C, false);
  B.soff.resize((size_t) B.L + 1);
  B.soff[0] = 0;
  for (int l = 0; l < B.L; l++)
    B.soff[l + 1] = B.soff[l] + lp[B.list_cap[l]].n_samples;
  B.S_tot = S_tot;
  B.n_tot = n_tot;
  B.classify = lp[0].classify != 0;
  B.filters = lp[0].filters_boundaries != 0;
  int64_t slot = 0;
  for (int k = 0; k < C; k++)
    slot = std::max<int64_t>(slot, std::min<int64_t>(8 * lp[k].n_samples, 8192));
  B.slot = slot;
  if (depth)
  {
    // one launch back-projects the whole batch into the raw buffer, packed, capture after capture (an error has drained the stream)
    if ((rc = depth_batch_to_raw(ctx, depth->who, depth->images, depth->n_images, C, depth->on_device, true, st)) != AGH_OK)
      return rc;
    for (int k = 0; k < C; k++)
    {
      B.d_raw[k] = c->d_raw_xyz + 3 * B.raw_off[k];
      B.dev_stride[k] = 12;
    }
  }
  else if (on_device)
    for (int k = 0; k < C; k++)
    {
      B.d_raw[k] = xyz[k];
      B.dev_stride[k] = stride_bytes[k];
    }
  else
  {
    int64_t need = 0;
    for (int k = 0; k < C; k++)
    {
      B.dev_stride[k] = device_stride(stride_bytes[k]);
      need += n[k] * (B.dev_stride[k] / 4);
    }
    // (a masked begin of host data never adopts a staged set: it drops a pending one as a begin of another kind does)
    const bool adopt = !src && L.staged_is(xyz, stride_bytes, n, C, true) && c->d_stage_xyz;
    // A staged batch that is this one: it is (or is about to be) in the second raw buffer -- the two buffers change places and the
    // chain waits for the copies.  Anything else that is staged (another batch, a capture of agh_localize_stage) is dropped: its
    // copy may still read the caller's source, so the chain waits for it too and agh_localize_batch_end's synchronisation covers it.
    if (L.staged)
      AGH_HIPCHK(c, hipStreamWaitEvent(st, c->stage_done, 0));
    L.staged = false;
    if (adopt)
      swap_raw_buffers(c);
    else if (need > c->raw_cap || !c->d_raw_xyz)
    {
      if ((rc = dev_alloc(c, &c->d_raw_xyz, (size_t) need)))
        return rc;
      c->raw_cap = need;
    }
    int64_t off = 0;
    for (int k = 0; k < C; k++)
    {
      float* dst = c->d_raw_xyz + off;
      if (!adopt)
        AGH_HIPCHK(c, upload_capture(dst, xyz[k], stride_bytes[k], n[k], st));
      B.d_raw[k] = dst;
      off += n[k] * (B.dev_stride[k] / 4);
    }
  }
  if (src && src->has_bytes() &&
      (rc = sample_source_to_device(c, *src, depth, C, B.n.data(), B.raw_off.data(), n_tot, &b->d_mask, &b->mask_cap, st,
         &B.source.d_bytes)) != AGH_OK)
    return chain_fail(c, rc);  // (the captures' copies may be in flight)
  ActiveGuard guard(c);
  if ((rc = batch_pass(ctx)) != AGH_OK)
    return rc;
  // (the next agh_localize_batch_stage into this raw buffer -- after it has changed places -- waits for this chain's reads)
  if (!on_device && c->raw_read)
  {
    AGH_HIPCHK_OR(c, hipEventRecord(c->raw_read, st), chain_fail(c, AGH_ERR_HIP));
    c->raw_read_set = true;
  }
  L.active = true;
  L.batch = true;
  return AGH_OK;
}

// agh_localize_batch_end: the one synchronisation and everything behind it -- the outgrown-bitmap repeat, the capacity-class
// repeat, the sequential-handle-walk repeat, the copy-out.  The chain is over whatever this returns.
int batch_end_impl(agh_ctx* ctx, const ChainOutputs& out, agh_localize_batch_result* results)
{
  Ctx* c = &ctx->c;
  LocalizeBatchState* b = c->lbatch;
  BatchCall& B = b->call;
  hipStream_t st = c->stream;
  const int C = B.C;
  const int64_t S_tot = B.S_tot;
  c->loc.active = false;
  c->loc.batch = false;
  c->results = ChainResults{};
  hand_drop_collect(c, 0, nullptr);
  handle_rank_collect(c, 0, nullptr);
  ActiveGuard guard(c);
  int rc;
  for (int pass = 0;; pass++)
  {
    if (pass > 0 && (rc = batch_pass(ctx)) != AGH_OK)  // (pass 0 was queued by agh_localize_batch_begin)
      return rc;
    AGH_HIPCHK_OR(c, hipStreamSynchronize(st), chain_fail(c, AGH_ERR_HIP));
    // ---- 6. the voxel descriptors: a lattice that outgrew the kept bitmap -> the batch once more with one sized for all, from
    // the raw buffer (or the caller's device memory) the chain read, which a capture staged meanwhile has not touched ----
    int64_t words = 0;
    bool outgrown = false;
    for (int k = 0; k < C; k++)
    {
      const VoxDesc& h = b->h_desc[k];
      if (h.error == 1)
      {
        drop_bound_cloud(c);
        c->err = std::string(B.who()) + ": capture " + std::to_string(k) + ": the voxel lattice of the kept points exceeds 2^33 cells "
                 "(1 GiB bitmap): set a workspace that bounds the scene";
        return AGH_ERR_CAPACITY;
      }
      outgrown |= h.error == 2;
      words = std::max<int64_t>(words, (int64_t) h.n_words);
    }
    if (outgrown)
    {
      drop_bound_cloud(c);
      if (pass > 0)
      {
        c->err = std::string(B.who()) + ": the voxel bitmap sized from the batch's lattices did not hold them";
        return AGH_ERR_CAPACITY;
      }
      b->slot_words = std::min<int64_t>(((words + words / 4) / 4096 + 1) * 4096, (int64_t) kVoxMaxWords);
      continue;
    }
    b->last_words = words;
    break;
  }
  // the bound batch is now the true one
  std::vector<int64_t> voff(C + 1, 0), nv((size_t) B.L);
  for (int k = 0; k < C; k++)
    voff[k + 1] = voff[k] + (int64_t) (b->h_desc[k].n_vox[0] + b->h_desc[k].n_vox[1]);
  ChainResults& R = c->results;
  R.kind = B.source.kind;
  R.batch = true;
  R.captures = C;
  if (R.kind == SourceKind::Mask)
  {
    R.lists = C;
    for (int k = 0; k < C; k++)
      R.counts[k] = (int64_t) b->h_mtotal[k];
  }
  else if (R.kind == SourceKind::Labels)
  {
    R.lists = B.L;
    for (int l = 0; l < B.L; l++)
      R.counts[l] = (int64_t) c->h_label_counts[l];
  }
  else if (B.source.clustered())
  {
    // (the table of k_cluster_select_batch: four counts per capture, then the M_l and the capture-local ids in list order; the
    // M_l equal the compaction's h_label_counts)
    const long long* t = c->h_cluster_table;
    R.lists = B.L;
    R.nv = voff[C];
    for (int k = 0; k < C; k++)
      std::copy(t + 4 * k, t + 4 * k + 4, R.cluster_info[k]);
    for (int l = 0; l < B.L; l++)
    {
      R.counts[l] = (int64_t) t[4 * kMaxClouds + l];
      R.cluster_ids[l] = (int32_t) t[5 * kMaxClouds + l];
    }
    for (int k = 0; k < C && B.source.fitted(); k++)  // (the records k_fit_finish_batch wrote into pinned memory)
    {
      R.fit_results[k] = b->h_fit_result[k];
      R.fit_candidates[k] = B.source.fit[k].n_candidates;
    }
  }
  for (int l = 0; l < B.L; l++)  // (a list's voxel count is its capture's)
    nv[l] = voff[B.list_cap[l] + 1] - voff[B.list_cap[l]];
  c->n_is_bound = false;
  c->n = voff[C];
  c->cloud_off = voff;
  c->cloud_off_on_device = true;
  c->n_clouds = C;
  return batch_collect(ctx, B.who(), "capture", nv.data(), out, results);
}

void zero_results(agh_localize_batch_result* results, int C)
{
  if (results && C >= 1 && C <= kMaxClouds)
    for (int k = 0; k < C; k++)
      results[k] = agh_localize_batch_result{ { 0, 0, 0, 0, 0 }, 0, 0, 0, 0 };
}

// agh_localize_batch[_device] = begin + end
int batch_call(agh_ctx* ctx, const float* const* xyz, bool on_device, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures, const ChainOutputs& out, agh_localize_batch_result* results,
  const DepthCaptures* depth = nullptr, const SampleSource* src = nullptr)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  {
    // (a labelled batch has a record per list; arguments that do not say how many lists there are get none zeroed)
    int64_t lists = n_captures;
    if (src && src->per_object())
    {
      lists = 0;
      if ((src->clustered() ? src->cluster != nullptr : src->n_objects != nullptr) && n_captures >= 1 && n_captures <= kMaxClouds)
        for (int k = 0; k < n_captures && lists <= kMaxClouds; k++)
          lists = src->objects(k) >= 1 && src->objects(k) <= kMaxClouds ? lists + src->objects(k) : kMaxClouds + 1;
    }
    zero_results(results, lists <= kMaxClouds ? (int) lists : 0);
  }
  if (c->loc.active)
  {
    c->err = std::string(src ? src->who : (depth ? depth->who : "agh_localize_batch")) + ": a localize chain is in flight on this context (agh_localize_end first)";
    return AGH_ERR_STATE;
  }
  if (out.bad())
  {
    c->err = depth || src ? std::string(src ? src->who : depth->who) + ": bad output arguments (see include/agh.h)" : std::string(kBadArguments);
    return AGH_ERR_INVALID_ARGUMENT;
  }
  const int rc = batch_begin_impl(ctx, xyz, on_device, stride_bytes, n, lp, n_captures, depth, src);
  if (rc != AGH_OK)
    return rc;
  return batch_end_impl(ctx, out, results);
}
}  // namespace

// The end of a chain over the batch state's C lists, behind its synchronisation and with its cloud bound: chain_collect's repeats
// and limits, results[k], and the outputs' assembly from the pinned slots, spans in list order (agh_internal.h).
int batch_collect(agh_ctx* ctx, const char* who, const char* unit, const int64_t* nv, const ChainOutputs& out,
  agh_localize_batch_result* results)
{
  Ctx* c = &ctx->c;
  LocalizeBatchState* b = c->lbatch;
  const BatchCall& B = b->call;
  const int C = B.L;  // (the lists)
  const int64_t S_tot = B.S_tot;
  int rc;
  const int* hc = b->h_counts;
  std::vector<std::string> names;
  if (B.per_object())
    for (int l = 0; l < C; l++)
      names.push_back("capture " + std::to_string(B.list_cap[l]) + ", object " + std::to_string(B.list_obj[l]));
  if ((rc = chain_collect(ctx, who, unit, C, hc, kBatchCountsStride, S_tot, b->h_bad, batch_queue, B.per_object() ? &names : nullptr)) != AGH_OK)
    return rc;
  int64_t n_hyp_tot = 0, tot_handles = 0, tot_idx = 0, tot_hands = 0;
  int64_t n_hyp[kMaxClouds];
  for (int k = 0; k < C; k++)
  {
    const int* h = hc + k * kBatchCountsStride;
    n_hyp[k] = h[4];
    if (results)
      results[k] = agh_localize_batch_result{ { nv[k], h[4], h[5], h[0], h[1] }, tot_handles, tot_idx, tot_hands, B.soff[k] };
    n_hyp_tot += h[4];
    tot_handles += h[0];
    tot_idx += h[1];
    tot_hands += h[5];
  }
  hand_drop_collect(c, C, n_hyp);
  {
    int64_t n_kept[kMaxClouds];
    for (int k = 0; k < C; k++)
      n_kept[k] = hc[k * kBatchCountsStride + 5];
    handle_rank_collect(c, C, n_kept);
  }
  c->last_nout = std::min<int64_t>(n_hyp_tot, c->s_cap * 8);
  if (out.samples && S_tot > 0)
    std::memcpy(out.samples, b->h_samples, sizeof(int32_t) * (size_t) S_tot);
  if (tot_handles > out.handle_cap || tot_idx > out.idx_cap || (out.hands && tot_hands > out.hands_cap))
  {
    c->err = std::string(who) + ": output buffers too small (the counts are in results)";
    return AGH_ERR_CAPACITY;
  }
  int64_t oh = 0, oi = 0, ok = 0;
  for (int k = 0; k < C; k++)
  {
    const int* h = hc + k * kBatchCountsStride;
    const size_t base = (size_t) k * (size_t) b->h_slot;
    if (h[0] > 0)
    {
      std::memcpy(out.handles + oh, b->h_handles + base, sizeof(agh_handle) * (size_t) h[0]);
      std::memcpy(out.inlier_idx + oi, b->h_idx + base, sizeof(int32_t) * (size_t) h[1]);
    }
    if (out.hands && h[5] > 0)
      std::memcpy(out.hands + ok, b->h_hands + base, sizeof(agh_hypothesis) * (size_t) h[5]);
    oh += h[0];
    oi += h[1];
    ok += h[5];
  }
  return AGH_OK;
}


// The batch state for the tail of a labelled chain (localize.hip): K lists, list j the samples j * S .. j * S + S - 1 of the one
// capture, every list with the capture's workspace (agh_internal.h).
int labeled_tail_prepare(agh_ctx* ctx, int K, int64_t S, const agh_localize_params* lp, double x1, double x2, int32_t** h_samples)
{
  Ctx* c = &ctx->c;
  int rc;
  if ((rc = ensure_batch_state(c)) != AGH_OK)
    return rc;
  LocalizeBatchState* b = c->lbatch;
  BatchCall& B = b->call;
  B = BatchCall();
  B.C = 1;
  B.L = K;
  B.list_cap.assign((size_t) K, 0);
  for (int j = 0; j < K; j++)
    B.list_obj.push_back(j);
  B.x1 = x1;
  B.x2 = x2;
  B.lp.assign(1, *lp);
  B.lp[0].sample_idx = nullptr;
  B.soff.resize(K + 1);
  for (int j = 0; j <= K; j++)
    B.soff[j] = (int64_t) j * S;
  B.S_tot = (int64_t) K * S;
  B.classify = lp->classify != 0;
  B.filters = lp->filters_boundaries != 0;
  B.slot = std::min<int64_t>(8 * S, 8192);
  if ((rc = ensure_batch_samples(c, b, B.S_tot)) != AGH_OK || (rc = ensure_batch_slots(c, b, K, B.slot)) != AGH_OK)
    return rc;
  if ((rc = fill_list_table(c, b, c->stream)) != AGH_OK)
    return rc;
  *h_samples = b->h_samples;
  return AGH_OK;
}

extern "C" {

int agh_localize_batch(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  return batch_call(ctx, xyz, false, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_batch_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  return batch_call(ctx, xyz, true, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results);
}

int agh_localize_batch_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures)
{
  return batch_begin_impl(ctx, xyz, false, stride_bytes, n, lp, n_captures);
}

int agh_localize_batch_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_localize_params* lp, int32_t n_captures)
{
  return batch_begin_impl(ctx, xyz, true, stride_bytes, n, lp, n_captures);
}

// The batch chain straight from depth images: agh_localize_depth_batch[_device] = begin + agh_localize_batch_end.
int agh_localize_depth_batch(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images, const agh_localize_params* lp,
  int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch" };
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth);
}

int agh_localize_depth_batch_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_device" };
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth);
}

int agh_localize_depth_batch_begin(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_begin" };
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth);
}

int agh_localize_depth_batch_begin_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_begin_device" };
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth);
}

// ---- the masked forms (include/agh.h): the batch chains with every capture's samples drawn under its own mask ----

int agh_localize_batch_masked(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const SampleSource m = mask_source(masks, nullptr, false, "agh_localize_batch_masked");
  return batch_call(ctx, xyz, false, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_masked_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const SampleSource m = mask_source(masks, nullptr, true, "agh_localize_batch_masked_device");
  return batch_call(ctx, xyz, true, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_masked_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = mask_source(masks, nullptr, false, "agh_localize_batch_masked_begin");
  return batch_begin_impl(ctx, xyz, false, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_batch_masked_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* masks, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = mask_source(masks, nullptr, true, "agh_localize_batch_masked_begin_device");
  return batch_begin_impl(ctx, xyz, true, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_depth_batch_masked(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks, const int32_t* n_images,
  const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out,
  int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_masked" };
  const SampleSource m = mask_source(nullptr, masks, false, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_masked_device(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks,
  const int32_t* n_images, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_masked_device" };
  const SampleSource m = mask_source(nullptr, masks, true, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_masked_begin(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks,
  const int32_t* n_images, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_masked_begin" };
  const SampleSource m = mask_source(nullptr, masks, false, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

int agh_localize_depth_batch_masked_begin_device(agh_ctx* ctx, const agh_depth_image* images, const agh_sample_mask* masks,
  const int32_t* n_images, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_masked_begin_device" };
  const SampleSource m = mask_source(nullptr, masks, true, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

int agh_get_batch_mask_counts(agh_ctx* ctx, int64_t* n_eligible, int32_t cap_captures)
{
  if (!ctx || !n_eligible)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_batch_mask_counts"))
    return AGH_ERR_STATE;
  if (!c->results.is(SourceKind::Mask, true))
  {
    c->err = "agh_get_batch_mask_counts: the last chain this context collected was no masked batch (or there was none)";
    return AGH_ERR_STATE;
  }
  if (cap_captures < c->results.captures)
  {
    c->err = "agh_get_batch_mask_counts: cap_captures is below the batch's n_captures";
    return AGH_ERR_CAPACITY;
  }
  std::copy(c->results.counts, c->results.counts + c->results.captures, n_eligible);
  return AGH_OK;
}

// ---- the labelled forms (include/agh.h): the batch chains with one list per object of every capture's label image ----

int agh_localize_batch_labeled(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const SampleSource m = label_source(labels, nullptr, n_objects, false, "agh_localize_batch_labeled");
  return batch_call(ctx, xyz, false, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_labeled_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const SampleSource m = label_source(labels, nullptr, n_objects, true, "agh_localize_batch_labeled_device");
  return batch_call(ctx, xyz, true, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_labeled_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = label_source(labels, nullptr, n_objects, false, "agh_localize_batch_labeled_begin");
  return batch_begin_impl(ctx, xyz, false, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_batch_labeled_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const uint8_t* const* labels, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = label_source(labels, nullptr, n_objects, true, "agh_localize_batch_labeled_begin_device");
  return batch_begin_impl(ctx, xyz, true, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_depth_batch_labeled(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_labeled" };
  const SampleSource m = label_source(nullptr, labels, n_objects, false, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_labeled_device(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_labeled_device" };
  const SampleSource m = label_source(nullptr, labels, n_objects, true, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_labeled_begin(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_labeled_begin" };
  const SampleSource m = label_source(nullptr, labels, n_objects, false, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

int agh_localize_depth_batch_labeled_begin_device(agh_ctx* ctx, const agh_depth_image* images, const agh_label_image* labels,
  const int32_t* n_images, const int32_t* n_objects, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_labeled_begin_device" };
  const SampleSource m = label_source(nullptr, labels, n_objects, true, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

int agh_get_batch_label_counts(agh_ctx* ctx, int64_t* n_eligible, int32_t cap_lists)
{
  if (!ctx || !n_eligible)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_batch_label_counts"))
    return AGH_ERR_STATE;
  if (!c->results.is(SourceKind::Labels, true))
  {
    c->err = "agh_get_batch_label_counts: the last chain this context collected was no labelled batch (or there was none)";
    return AGH_ERR_STATE;
  }
  if (cap_lists < c->results.lists)
  {
    c->err = "agh_get_batch_label_counts: cap_lists is below the call's number of lists";
    return AGH_ERR_CAPACITY;
  }
  std::copy(c->results.counts, c->results.counts + c->results.lists, n_eligible);
  return AGH_OK;
}

// ---- the clustered forms (include/agh.h): the labelled batch chains with every capture's own connected components as its objects ----

int agh_localize_batch_clustered(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const SampleSource m = cluster_source(cp, nullptr, false, "agh_localize_batch_clustered");
  return batch_call(ctx, xyz, false, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_clustered_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const SampleSource m = cluster_source(cp, nullptr, false, "agh_localize_batch_clustered_device");
  return batch_call(ctx, xyz, true, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_clustered_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = cluster_source(cp, nullptr, false, "agh_localize_batch_clustered_begin");
  return batch_begin_impl(ctx, xyz, false, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_batch_clustered_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = cluster_source(cp, nullptr, false, "agh_localize_batch_clustered_begin_device");
  return batch_begin_impl(ctx, xyz, true, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_depth_batch_clustered(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_clustered" };
  const SampleSource m = cluster_source(cp, nullptr, false, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_clustered_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures, agh_handle* handles_out, int64_t handle_cap,
  int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out,
  agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_clustered_device" };
  const SampleSource m = cluster_source(cp, nullptr, false, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_clustered_begin(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_clustered_begin" };
  const SampleSource m = cluster_source(cp, nullptr, false, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

int agh_localize_depth_batch_clustered_begin_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_clustered_begin_device" };
  const SampleSource m = cluster_source(cp, nullptr, false, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

// the last chain collected, if it was a clustered batch (`fn` refuses otherwise, and mid-chain)
static int batch_cluster_getter_check(Ctx* c, const char* fn)
{
  if (refuse_mid_chain(c, fn))
    return AGH_ERR_STATE;
  if (!c->results.is_clustered(true))
  {
    c->err = std::string(fn) + ": the last chain this context collected was no clustered batch (or there was none)";
    return AGH_ERR_STATE;
  }
  return AGH_OK;
}

int agh_get_batch_cluster_info(agh_ctx* ctx, agh_cluster_info* info, int64_t* n_voxels, int32_t* ids, int32_t cap_captures,
  int32_t cap_lists)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = batch_cluster_getter_check(c, "agh_get_batch_cluster_info"))
    return rc;
  const ChainResults& R = c->results;
  if (info && cap_captures < R.captures)
  {
    c->err = "agh_get_batch_cluster_info: cap_captures is below the batch's n_captures";
    return AGH_ERR_CAPACITY;
  }
  if ((n_voxels || ids) && cap_lists < R.lists)
  {
    c->err = "agh_get_batch_cluster_info: cap_lists is below the call's number of lists";
    return AGH_ERR_CAPACITY;
  }
  if (info)
    for (int k = 0; k < R.captures; k++)
      info[k] = agh_cluster_info{ R.cluster_info[k][0], R.cluster_info[k][1], R.cluster_info[k][2] };
  if (n_voxels)
    std::copy(R.counts, R.counts + R.lists, n_voxels);
  if (ids)
    std::copy(R.cluster_ids, R.cluster_ids + R.lists, ids);
  return AGH_OK;
}

int agh_get_batch_cluster_labels(agh_ctx* ctx, uint8_t* labels_out, int64_t cap)
{
  if (!ctx || !labels_out)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = batch_cluster_getter_check(c, "agh_get_batch_cluster_labels"))
    return rc;
  const int64_t nv = c->results.nv;
  if (cap < nv)
  {
    c->err = "agh_get_batch_cluster_labels: cap is below the bound batch's voxel count";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  if (nv > 0)
    AGH_HIPCHK(c, hipMemcpy(labels_out, c->d_cluster_label, (size_t) nv, hipMemcpyDeviceToHost));
  return (int) nv;
}

// ---- the fitted forms (include/agh.h, agh_localize_batch_clustered_fit*): the clustered batch chains with every capture's
// support plane found on its own voxels by plane_fit.hip, in front of the one cluster stage ----

int agh_localize_batch_clustered_fit(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const SampleSource m = cluster_source(cp, fp, true, "agh_localize_batch_clustered_fit");
  return batch_call(ctx, xyz, false, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_clustered_fit_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const SampleSource m = cluster_source(cp, fp, true, "agh_localize_batch_clustered_fit_device");
  return batch_call(ctx, xyz, true, stride_bytes, n, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, nullptr, &m);
}

int agh_localize_batch_clustered_fit_begin(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = cluster_source(cp, fp, true, "agh_localize_batch_clustered_fit_begin");
  return batch_begin_impl(ctx, xyz, false, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_batch_clustered_fit_begin_device(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes,
  const int64_t* n, const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const SampleSource m = cluster_source(cp, fp, true, "agh_localize_batch_clustered_fit_begin_device");
  return batch_begin_impl(ctx, xyz, true, stride_bytes, n, lp, n_captures, nullptr, &m);
}

int agh_localize_depth_batch_clustered_fit(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_clustered_fit" };
  const SampleSource m = cluster_source(cp, fp, true, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_clustered_fit_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures,
  agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap, agh_hypothesis* hands_out,
  int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_clustered_fit_device" };
  const SampleSource m = cluster_source(cp, fp, true, depth.who);
  return batch_call(ctx, nullptr, false, nullptr, nullptr, lp, n_captures,
    { handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out }, results, &depth, &m);
}

int agh_localize_depth_batch_clustered_fit_begin(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, false, "agh_localize_depth_batch_clustered_fit_begin" };
  const SampleSource m = cluster_source(cp, fp, true, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

int agh_localize_depth_batch_clustered_fit_begin_device(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images,
  const agh_plane_fit_params* fp, const agh_cluster_params* cp, const agh_localize_params* lp, int32_t n_captures)
{
  const DepthCaptures depth{ images, n_images, true, "agh_localize_depth_batch_clustered_fit_begin_device" };
  const SampleSource m = cluster_source(cp, fp, true, depth.who);
  return batch_begin_impl(ctx, nullptr, false, nullptr, nullptr, lp, n_captures, &depth, &m);
}

// the last chain collected, if it was a fitted clustered batch (`fn` refuses otherwise, and mid-chain)
static int batch_fit_getter_check(Ctx* c, const char* fn)
{
  if (refuse_mid_chain(c, fn))
    return AGH_ERR_STATE;
  if (!c->results.is(SourceKind::FittedClusters, true))
  {
    c->err = std::string(fn) + ": the last chain this context collected was no fitted clustered batch (or there was none)";
    return AGH_ERR_STATE;
  }
  return AGH_OK;
}

int agh_get_batch_plane_fit(agh_ctx* ctx, agh_plane_fit_result* out, int32_t cap_captures)
{
  if (!ctx || !out)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = batch_fit_getter_check(c, "agh_get_batch_plane_fit"))
    return rc;
  if (cap_captures < c->results.captures)
  {
    c->err = "agh_get_batch_plane_fit: cap_captures is below the batch's n_captures";
    return AGH_ERR_CAPACITY;
  }
  std::copy(c->results.fit_results, c->results.fit_results + c->results.captures, out);
  return c->results.captures;
}

int agh_get_batch_plane_fit_candidates(agh_ctx* ctx, int32_t capture, int32_t* idx, double* planes, int64_t* counts, int32_t cap)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = batch_fit_getter_check(c, "agh_get_batch_plane_fit_candidates"))
    return rc;
  if (capture < 0 || capture >= c->results.captures)
  {
    c->err = "agh_get_batch_plane_fit_candidates: capture must be 0 .. n_captures - 1 of the batch";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  const int C = c->results.fit_candidates[capture];
  if ((idx || planes || counts) && cap < C)
  {
    c->err = "agh_get_batch_plane_fit_candidates: cap is below the capture's n_candidates";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  // (the candidates stay on the device until somebody asks: a blocking copy each, behind whatever the context's stream holds)
  const PlaneFitBuffers* fb = c->lbatch->d_fit + capture;
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

// The NEXT batch's captures up, beside whatever runs on the context's stream (stage_captures, localize.hip).  A pinned source must
// stay valid until the agh_localize_batch_end of the chain that adopts (or drops) the set.
int agh_localize_batch_stage(agh_ctx* ctx, const float* const* xyz, const int64_t* stride_bytes, const int64_t* n, int32_t n_captures)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  const int C = n_captures;
  if (C < 1 || C > kMaxClouds || !xyz || !stride_bytes || !n)
  {
    c->err = "agh_localize_batch_stage: bad arguments (1 <= n_captures <= 64; see include/agh.h)";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  int64_t n_tot = 0;
  for (int k = 0; k < C; k++)
  {
    if (bad_capture(xyz[k], stride_bytes[k], n[k]))
    {
      c->err = "agh_localize_batch_stage: bad arguments for capture " + std::to_string(k) + " (see include/agh.h)";
      return AGH_ERR_INVALID_ARGUMENT;
    }
    n_tot += n[k];
  }
  if (n_tot >= (1ll << 30))
  {
    c->err = "agh_localize_batch_stage: need fewer than 2^30 raw points in all";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  return stage_captures(ctx, "agh_localize_batch_stage", xyz, stride_bytes, n, C, true);
}

int agh_localize_batch_end(agh_ctx* ctx, agh_handle* handles_out, int64_t handle_cap, int32_t* inlier_idx_out, int64_t idx_cap,
  agh_hypothesis* hands_out, int64_t hands_cap, int32_t* samples_out, agh_localize_batch_result* results)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (!c->loc.active || !c->loc.batch)
  {
    c->err = c->loc.active ? "agh_localize_batch_end: the chain in flight is a single capture's (agh_localize_end collects it)"
                           : "agh_localize_batch_end: no agh_localize_batch_begin in flight";
    return AGH_ERR_STATE;
  }
  zero_results(results, c->lbatch->call.L);
  const ChainOutputs out{ handles_out, handle_cap, inlier_idx_out, idx_cap, hands_out, hands_cap, samples_out };
  if (out.bad())
  {
    // (the chain is queued: drain it, leave the context as a failed call does)
    c->loc.active = false;
    c->loc.batch = false;
    c->err = kBadArguments;
    return chain_fail(c, AGH_ERR_INVALID_ARGUMENT);
  }
  return batch_end_impl(ctx, out, results);
}

}  // extern "C"
