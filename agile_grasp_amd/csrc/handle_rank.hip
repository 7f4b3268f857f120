// handle_rank.hip -- agh_set_handle_ranking / agh_rank_handles (include/agh.h; DESIGN.md, "Handle ranking"): the handles of every
// list of a localize chain leave in rank order.  k_handle_rank is queued behind k_handle_build (handles.hip): one work-group per
// list, a wave per handle for the seven terms and the score, then a sort of (key, index) pairs in LDS and the permuted records
// written into the pinned mirror k_handle_build wrote.  The arithmetic is the contract's: float64, left to right, not contracted
// (-ffp-contract=off is the build's); tests/handle_ranking_cases.py is its numpy model.  Included at the end of handles.hip, whose
// translation unit it shares (build.SRC stays as it is; build.needs_build lists this file).
#include "agh_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

using namespace agh;

namespace
{
constexpr int kRankMax = 8192;      // handles of one list (a handle holds at least one of the list's <= 8192 hands)
constexpr int kRankNone = 0x7fffffff;
constexpr int kRankBelow = 1 << 30;  // OR-ed into the index of a handle min_score leaves out: behind every handle that stays
static_assert(sizeof(agh_handle) == 17 * 8 && sizeof(agh_handle_score) == 9 * 8, "the records move as 8-byte words");

__device__ __forceinline__ double rank_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// (key, index) pair a goes in front of pair b: key descending, index ascending -- a total order, the indices are distinct
__device__ __forceinline__ bool rank_before(unsigned long long ka, int ia, unsigned long long kb, int ib)
{
  return ka > kb || (ka == kb && ia < ib);
}

// One work-group of sixteen waves per list (blockIdx.y, the handle kernels' slices).  handles: k_handle_build's device records in
// list order, which stay as they are; margins: the kept hands' (null: 0.0).  tmp: the score records in list order (device).
// host_handles / host_scores / rank_counts / host_counts: pinned memory in the chains (the stage-wise call hands device buffers in).
__global__ __launch_bounds__(1024) void k_handle_rank(const agh_hypothesis* __restrict__ hands, const int* __restrict__ inlier_idx,
  const HandleCounts* __restrict__ counts, const agh_handle* __restrict__ handles, const double* __restrict__ margins,
  agh_handle_ranking_params rp, agh_handle_score* __restrict__ tmp, agh_handle* __restrict__ host_handles, int host_cap,
  agh_handle_score* __restrict__ host_scores, int* __restrict__ rank_counts, int* __restrict__ host_counts, HandleSlots sl)
{
  AGH_HANDLE_SLICE(hands, sl.hands);
  AGH_HANDLE_SLICE(inlier_idx, sl.hands);
  AGH_HANDLE_SLICE(counts, 1);
  AGH_HANDLE_SLICE(handles, sl.hands);
  AGH_HANDLE_SLICE(margins, sl.hands);
  AGH_HANDLE_SLICE(tmp, sl.hands);
  AGH_HANDLE_SLICE(host_handles, sl.host);
  AGH_HANDLE_SLICE(host_scores, sl.host);
  AGH_HANDLE_SLICE(rank_counts, 4);
  AGH_HANDLE_SLICE(host_counts, sl.host_counts);
  __shared__ unsigned long long keys[kRankMax];  // 64 KiB
  __shared__ int idxs[kRankMax];                 // 32 KiB
  __shared__ int s_below;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nh = min(max(counts->n_handles, 0), kRankMax);
  int P = 2;  // the sort's length: a power of two, the tail padded behind everything
  while (P < nh)
    P <<= 1;
  if (tid == 0)
    s_below = 0;
  for (int i = nh + tid; i < P; i += 1024)
  {
    keys[i] = 0ull;
    idxs[i] = kRankNone;
  }
  __syncthreads();
  // ---- a wave per handle: the terms, the score, the sort key ----
  for (int h = wave; h < nh; h += 16)
  {
    const agh_handle& hd = handles[h];
    const int n = hd.n_inliers;
    const int* in = inlier_idx + hd.first_inlier;
    const double ax[3] = { hd.axis[0], hd.axis[1], hd.axis[2] };
    double p = 0.0, xmax = -INFINITY, xmin = INFINITY, best = 0.0;
    int best_k = kRankNone;
    for (int k = lane; k < n; k += 64)  // (n <= 64: one inlier per lane, every load in flight at once)
    {
      const int j = in[k];
      const double g = margins ? margins[j] : 0.0;
      const double x = rank_dot3(ax, hands[j].bottom);
      p = p + g;
      xmax = fmax(xmax, x);
      xmin = fmin(xmin, x);
      if (!(g != g) && (best_k == kRankNone || g > best))  // strict: the first maximum of this lane's (ascending) positions
      {
        best = g;
        best_k = k;
      }
    }
    for (int o = 32; o > 0; o >>= 1)
    {
      p = p + __shfl_xor(p, o);
      xmax = fmax(xmax, __shfl_xor(xmax, o));
      xmin = fmin(xmin, __shfl_xor(xmin, o));
      const double ob = __shfl_xor(best, o);
      const int ok = __shfl_xor(best_k, o);
      if (ok != kRankNone && (best_k == kRankNone || ob > best || (ob == best && ok < best_k)))
      {
        best = ob;
        best_k = ok;
      }
    }
    if (lane == 0)
    {
      agh_handle_score sc;
      const double e[3] = { hd.center[0] - rp.ref_point[0], hd.center[1] - rp.ref_point[1], hd.center[2] - rp.ref_point[2] };
      sc.terms[0] = (double) min(n, rp.support_cap) / (double) rp.support_cap;
      sc.terms[1] = p / (double) n;
      sc.terms[2] = rank_dot3(hd.approach, rp.approach_dir);
      sc.terms[3] = rank_dot3(hd.center, rp.position_dir);
      sc.terms[4] = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
      sc.terms[5] = fabs(hd.width - rp.preferred_width);
      sc.terms[6] = xmax - xmin;
      const double score = (((((rp.w_support * sc.terms[0] + rp.w_margin * sc.terms[1]) + rp.w_approach * sc.terms[2]) +
                               rp.w_position * sc.terms[3]) + rp.w_distance * sc.terms[4]) + rp.w_width * sc.terms[5]) +
                           rp.w_length * sc.terms[6];
      sc.score = score;
      sc.index = h;
      sc.best_inlier = best_k == kRankNone ? 0 : best_k;
      tmp[h] = sc;
      // the key: a monotone 64-bit image of the double (+0 and -0 tie), NaN below every number
      const bool below = rp.min_score != -INFINITY && !(score >= rp.min_score);  // (-inf: no bound, a NaN score stays)
      unsigned long long key = 0ull;
      if (!below && !(score != score))
      {
        const unsigned long long b = (unsigned long long) __double_as_longlong(score == 0.0 ? 0.0 : score);
        key = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
      }
      keys[h] = key;
      idxs[h] = below ? (h | kRankBelow) : h;
      if (below)
        atomicAdd(&s_below, 1);  // (a count: no order in it)
    }
  }
  __syncthreads();
  // ---- bitonic sort of the P pairs by rank_before ----
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1)
    {
      for (int t = tid; t < (P >> 1); t += 1024)
      {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const unsigned long long ka = keys[i], kb = keys[l];
        const int ia = idxs[i], ib = idxs[l];
        const bool up = (i & k) == 0;
        if (up ? rank_before(kb, ib, ka, ia) : rank_before(ka, ia, kb, ib))
        {
          keys[i] = kb;
          keys[l] = ka;
          idxs[i] = ib;
          idxs[l] = ia;
        }
      }
      __syncthreads();
    }
  // ---- the records in rank order ----
  const int n_below = s_below;
  int n_ret = nh - n_below;
  if (rp.max_handles > 0)
    n_ret = min(n_ret, rp.max_handles);
  const int n_out = min(n_ret, host_cap);
  const unsigned long long* hsrc = reinterpret_cast<const unsigned long long*>(handles);
  unsigned long long* hdst = reinterpret_cast<unsigned long long*>(host_handles);
  for (int t = tid; t < n_out * 17; t += 1024)
  {
    const int r = t / 17, part = t - 17 * r;
    hdst[(int64_t) r * 17 + part] = hsrc[(int64_t) idxs[r] * 17 + part];
  }
  const unsigned long long* ssrc = reinterpret_cast<const unsigned long long*>(tmp);
  unsigned long long* sdst = reinterpret_cast<unsigned long long*>(host_scores);
  if (host_scores)
    for (int t = tid; t < n_out * 9; t += 1024)
    {
      const int r = t / 9, part = t - 9 * r;
      sdst[(int64_t) r * 9 + part] = ssrc[(int64_t) idxs[r] * 9 + part];
    }
  if (tid == 0)
  {
    rank_counts[0] = nh;
    rank_counts[1] = n_below;
    rank_counts[2] = n_ret;
    if (host_counts)
      host_counts[0] = n_ret;  // (HandleMirror::counts[0]: the handles the chain returns)
  }
}

std::string ranking_fault(const agh_handle_ranking_params& p)
{
  const char* name[17] = { "w_support", "w_margin", "w_approach", "w_position", "w_distance", "w_width", "w_length", "approach_dir[0]",
    "approach_dir[1]", "approach_dir[2]", "position_dir[0]", "position_dir[1]", "position_dir[2]", "ref_point[0]", "ref_point[1]",
    "ref_point[2]", "preferred_width" };
  const double value[17] = { p.w_support, p.w_margin, p.w_approach, p.w_position, p.w_distance, p.w_width, p.w_length, p.approach_dir[0],
    p.approach_dir[1], p.approach_dir[2], p.position_dir[0], p.position_dir[1], p.position_dir[2], p.ref_point[0], p.ref_point[1],
    p.ref_point[2], p.preferred_width };
  for (int k = 0; k < 17; k++)
    if (!std::isfinite(value[k]))
      return std::string(name[k]) + " is not finite";
  if (!std::isfinite(p.min_score) && !(p.min_score == -std::numeric_limits<double>::infinity()))
    return "min_score must be finite or -inf";
  const double* d = p.approach_dir;
  if (std::fabs(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0) > 1e-6)
    return "approach_dir must be a unit vector (|a^2 + b^2 + c^2 - 1| <= 1e-6)";
  if (p.support_cap < 1)
    return "support_cap must be >= 1";
  if (p.max_handles < 0)
    return "max_handles must be >= 0";
  return std::string();
}

template <typename T>
int rank_pinned(Ctx* c, T** p, size_t count)
{
  if (*p)
  {
    (void) hipHostFree(*p);
    *p = nullptr;
  }
  void* q = nullptr;
  AGH_HIPCHK(c, hipHostMalloc(&q, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault));
  *p = static_cast<T*>(q);
  return AGH_OK;
}

int rank_launch(Ctx* c, const agh_handle_ranking_params& rp, const agh_hypothesis* hands, const int* idx, const int* counts,
  const agh_handle* handles, const double* margins, agh_handle_score* tmp, agh_handle* out_handles, int out_cap,
  agh_handle_score* out_scores, int* rank_counts, int* host_counts, int n_lists, const HandleSlots& sl, hipStream_t st)
{
  hipLaunchKernelGGL(k_handle_rank, dim3(1, (unsigned) n_lists), dim3(1024), 0, st, hands, idx,
    reinterpret_cast<const HandleCounts*>(counts), handles, margins, rp, tmp, out_handles, out_cap, out_scores, rank_counts, host_counts,
    sl);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "k_handle_rank launch failed";
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}
}  // namespace

namespace agh
{
void handle_rank_release(Ctx* c)
{
  HandleRankState& S = c->handle_rank;
  for (void* p : { (void*) S.d_margin, (void*) S.d_scores })
    if (p)
      (void) hipFree(p);
  for (void* p : { (void*) S.h_margin, (void*) S.h_scores, (void*) S.h_counts })
    if (p)
      (void) hipHostFree(p);
  S.d_margin = nullptr;
  S.d_scores = nullptr;
  S.h_margin = nullptr;
  S.h_scores = nullptr;
  S.h_counts = nullptr;
  S.dev_cap = S.host_cap = 0;
}

int handle_rank_check(Ctx* c, const char* who, bool classify)
{
  const HandleRankState& S = c->handle_rank;
  if (S.set && S.p.w_margin != 0.0 && !classify)
  {
    c->err = std::string(who) + ": the handle ranking's w_margin is not 0 and classify is 0 (the margin is the classifier's)";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  return AGH_OK;
}

int handle_rank_prepare(Ctx* c, int n_lists, int64_t slot, int64_t host_slot, bool classify, MarginOut* m)
{
  HandleRankState& S = c->handle_rank;
  *m = MarginOut{ nullptr, nullptr, nullptr, 0, 0 };
  S.queued = false;
  if (!S.set)
    return AGH_OK;
  int rc;
  slot = std::max<int64_t>(slot, 1);
  host_slot = std::max<int64_t>(host_slot, 1);
  const int64_t dev = slot * n_lists, host = host_slot * n_lists;
  if (dev > S.dev_cap || !S.d_margin)
  {
    S.dev_cap = 0;
    if ((rc = dev_alloc(c, &S.d_margin, (size_t) dev)) || (rc = dev_alloc(c, &S.d_scores, (size_t) dev)))
      return rc;
    S.dev_cap = dev;
  }
  if (host > S.host_cap || !S.h_margin)
  {
    S.host_cap = 0;
    if ((rc = rank_pinned(c, &S.h_margin, (size_t) host)) || (rc = rank_pinned(c, &S.h_scores, (size_t) host)))
      return rc;
    S.host_cap = host;
  }
  if (!S.h_counts && (rc = rank_pinned(c, &S.h_counts, (size_t) kMaxClouds * 4)))
    return rc;
  for (int k = 0; k < n_lists * 4; k++)
    S.h_counts[k] = 0;
  S.queued = true;
  S.with_margins = classify;
  S.slot = slot;
  S.host_slot = host_slot;
  // (without a classifier the margins are 0.0 by contract: the kernel is told so by a null pointer, the compaction writes nothing)
  if (classify)
    *m = MarginOut{ c->d_svm_sums, S.d_margin, S.h_margin, slot, host_slot };
  return AGH_OK;
}

int handle_rank_stage(Ctx* c, const HandleBufs& b, int n_lists, int64_t slot, const HandleMirror& hm, int host_counts_stride,
  hipStream_t st)
{
  HandleRankState& S = c->handle_rank;
  if (!S.queued)
    return AGH_OK;
  // (the lists' strides: the handle search's on the device; the pinned scores follow the pinned handles' when there are several)
  const bool many = n_lists > 1 || slot > 0;
  const HandleSlots sl{ many ? slot : 0, 0, many ? (int64_t) hm.handle_cap : 0, host_counts_stride };
  if (many && (slot != S.slot || (int64_t) hm.handle_cap != S.host_slot))
  {
    c->err = "k_handle_rank: the lists' slots changed behind the compaction";
    return AGH_ERR_HIP;
  }
  return rank_launch(c, S.p, b.hands, b.idx, b.counts, b.handles, S.with_margins ? S.d_margin : nullptr, S.d_scores, hm.handles,
    (int) std::min<int64_t>(hm.handle_cap, S.host_slot), S.h_scores, S.h_counts, hm.counts, n_lists, sl, st);
}

void handle_rank_collect(Ctx* c, int lists, const int64_t* n_kept)
{
  HandleRankState& S = c->handle_rank;
  S.ran = false;
  S.lists = 0;
  S.scores.clear();
  S.margins.clear();
  if (lists <= 0 || !S.queued)
    return;
  for (int l = 0; l < lists; l++)
  {
    const int* h = S.h_counts + l * 4;
    S.counts[l] = agh_handle_ranking_counts{ h[0], h[1], h[2] };
    const int64_t n_ret = std::min<int64_t>(h[2], S.host_slot), n_h = std::min<int64_t>(n_kept[l], S.host_slot);
    const agh_handle_score* sc = S.h_scores + (int64_t) l * S.host_slot;
    S.scores.insert(S.scores.end(), sc, sc + n_ret);
    if (S.with_margins)
      S.margins.insert(S.margins.end(), S.h_margin + (int64_t) l * S.host_slot, S.h_margin + (int64_t) l * S.host_slot + n_h);
    else
      S.margins.insert(S.margins.end(), (size_t) n_h, 0.0);
  }
  S.ran = true;
  S.lists = lists;
  S.queued = false;
}
}  // namespace agh

namespace
{
// the three result getters' common refusals
int rank_results_refused(Ctx* c, const char* fn)
{
  if (refuse_mid_chain(c, fn))
    return AGH_ERR_STATE;
  if (c->batch_active)
  {
    c->err = std::string(fn) + ": an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  if (!c->handle_rank.ran)
  {
    c->err = std::string(fn) + ": the last chain collected ran without a handle ranking (agh_set_handle_ranking)";
    return AGH_ERR_STATE;
  }
  return AGH_OK;
}
}  // namespace

extern "C" {

void agh_default_handle_ranking_params(agh_handle_ranking_params* p)
{
  if (!p)
    return;
  std::memset(p, 0, sizeof(*p));
  p->w_support = 1.0;
  p->w_margin = 1.0;
  p->approach_dir[2] = -1.0;
  p->position_dir[2] = 1.0;
  p->min_score = -std::numeric_limits<double>::infinity();
  p->support_cap = 10;
  p->max_handles = 0;
}

int agh_set_handle_ranking(agh_ctx* ctx, const agh_handle_ranking_params* rp)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_set_handle_ranking"))
    return AGH_ERR_STATE;
  if (c->batch_active)
  {
    c->err = "agh_set_handle_ranking: an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  if (!rp)
  {
    c->handle_rank.set = false;
    return AGH_OK;
  }
  const std::string fault = ranking_fault(*rp);
  if (!fault.empty())
  {
    c->err = "agh_set_handle_ranking: " + fault;
    return AGH_ERR_INVALID_ARGUMENT;
  }
  c->handle_rank.p = *rp;
  c->handle_rank.set = true;
  return AGH_OK;
}

int agh_get_handle_ranking(agh_ctx* ctx, agh_handle_ranking_params* out)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (!c->handle_rank.set)
    return 0;
  if (!out)
  {
    c->err = "agh_get_handle_ranking: out is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  *out = c->handle_rank.p;
  return 1;
}

int agh_get_handle_scores(agh_ctx* ctx, agh_handle_score* out, int64_t cap)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = rank_results_refused(c, "agh_get_handle_scores"))
    return rc;
  const int64_t n = (int64_t) c->handle_rank.scores.size();
  if (cap < n || (n > 0 && !out))
  {
    c->err = "agh_get_handle_scores: room for " + std::to_string(n) + " records is needed";
    return AGH_ERR_CAPACITY;
  }
  if (n > 0)
    std::memcpy(out, c->handle_rank.scores.data(), sizeof(agh_handle_score) * (size_t) n);
  return (int) n;
}

int agh_get_handle_ranking_counts(agh_ctx* ctx, agh_handle_ranking_counts* out, int32_t cap_lists)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = rank_results_refused(c, "agh_get_handle_ranking_counts"))
    return rc;
  const int lists = c->handle_rank.lists;
  if (cap_lists < lists || !out)
  {
    c->err = "agh_get_handle_ranking_counts: room for " + std::to_string(lists) + " lists is needed";
    return AGH_ERR_CAPACITY;
  }
  std::copy(c->handle_rank.counts, c->handle_rank.counts + lists, out);
  return lists;
}

int agh_get_hand_margins(agh_ctx* ctx, double* out, int64_t cap)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (int rc = rank_results_refused(c, "agh_get_hand_margins"))
    return rc;
  const int64_t n = (int64_t) c->handle_rank.margins.size();
  if (cap < n || (n > 0 && !out))
  {
    c->err = "agh_get_hand_margins: room for " + std::to_string(n) + " values is needed";
    return AGH_ERR_CAPACITY;
  }
  if (n > 0)
    std::memcpy(out, c->handle_rank.margins.data(), sizeof(double) * (size_t) n);
  return (int) n;
}

int agh_rank_handles(agh_ctx* ctx, const agh_handle_ranking_params* rp, const agh_hypothesis* hands, int64_t n_hands,
  const double* margins, const agh_handle* handles, int64_t n_handles, const int32_t* inlier_idx, int64_t n_idx,
  agh_handle* handles_out, agh_handle_score* scores_out, int64_t cap, agh_handle_ranking_counts* counts)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (counts)
    *counts = agh_handle_ranking_counts{ 0, 0, 0 };
  if (refuse_mid_chain(c, "agh_rank_handles"))
    return AGH_ERR_STATE;
  if (c->batch_active)
  {
    c->err = "agh_rank_handles: an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  auto bad = [c](const std::string& what) {
    c->err = "agh_rank_handles: " + what;
    return AGH_ERR_INVALID_ARGUMENT;
  };
  if (!rp)
    return bad("rp is NULL");
  const std::string fault = ranking_fault(*rp);
  if (!fault.empty())
    return bad(fault);
  if (n_hands < 0 || n_handles < 0 || n_idx < 0 || cap < 0 || (n_hands > 0 && !hands) || (n_handles > 0 && !handles) ||
      (n_idx > 0 && !inlier_idx) || (cap > 0 && !handles_out && !scores_out))
    return bad("bad arguments (see include/agh.h)");
  if (n_hands > kRankMax || n_handles > kRankMax)
  {
    c->err = "agh_rank_handles: more than 8192 hands or handles";
    return AGH_ERR_CAPACITY;
  }
  // every inlier span inside n_idx, every index a span covers inside n_hands
  std::vector<int32_t> cover((size_t) n_idx + 1, 0);
  for (int64_t h = 0; h < n_handles; h++)
  {
    const int64_t n = handles[h].n_inliers, f = handles[h].first_inlier;
    if (n < 1)
      return bad("handle " + std::to_string(h) + ": n_inliers is below 1");
    if (f < 0 || f + n > n_idx)
      return bad("handle " + std::to_string(h) + ": its inliers lie outside n_idx");
    cover[(size_t) f]++;
    cover[(size_t) (f + n)]--;
  }
  for (int64_t k = 0, open = 0; k < n_idx; k++)
  {
    open += cover[(size_t) k];
    if (open > 0 && (inlier_idx[k] < 0 || inlier_idx[k] >= n_hands))
      return bad("inlier_idx[" + std::to_string(k) + "] is outside n_hands");
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  // the call's own device buffers (a stage-wise call: made and dropped here)
  struct Bufs
  {
    agh_hypothesis* hands = nullptr;
    double* marg = nullptr;
    agh_handle *handles = nullptr, *out = nullptr;
    int32_t* idx = nullptr;
    agh_handle_score *tmp = nullptr, *scores = nullptr;
    int* counts = nullptr;  // HandleCounts, then the three rank counts
    ~Bufs()
    {
      for (void* p : { (void*) hands, (void*) marg, (void*) handles, (void*) out, (void*) idx, (void*) tmp, (void*) scores, (void*) counts })
        if (p)
          (void) hipFree(p);
    }
  } B;
  int rc;
  const size_t nh = (size_t) n_handles;
  if ((rc = dev_alloc(c, &B.hands, (size_t) n_hands)) || (margins && (rc = dev_alloc(c, &B.marg, (size_t) n_hands))) ||
      (rc = dev_alloc(c, &B.handles, nh)) || (rc = dev_alloc(c, &B.out, nh)) || (rc = dev_alloc(c, &B.idx, (size_t) n_idx)) ||
      (rc = dev_alloc(c, &B.tmp, nh)) || (rc = dev_alloc(c, &B.scores, nh)) || (rc = dev_alloc(c, &B.counts, 8)))
    return rc;
  hipStream_t st = c->stream;
  const int h_counts[8] = { (int) n_handles, (int) n_idx, 0, 0, 0, 0, 0, 0 };
  if (n_hands > 0)
    AGH_HIPCHK(c, hipMemcpyAsync(B.hands, hands, sizeof(agh_hypothesis) * (size_t) n_hands, hipMemcpyHostToDevice, st));
  if (margins && n_hands > 0)
    AGH_HIPCHK(c, hipMemcpyAsync(B.marg, margins, sizeof(double) * (size_t) n_hands, hipMemcpyHostToDevice, st));
  if (n_handles > 0)
    AGH_HIPCHK(c, hipMemcpyAsync(B.handles, handles, sizeof(agh_handle) * nh, hipMemcpyHostToDevice, st));
  if (n_idx > 0)
    AGH_HIPCHK(c, hipMemcpyAsync(B.idx, inlier_idx, sizeof(int32_t) * (size_t) n_idx, hipMemcpyHostToDevice, st));
  AGH_HIPCHK(c, hipMemcpyAsync(B.counts, h_counts, sizeof(h_counts), hipMemcpyHostToDevice, st));
  AGH_HIPCHK(c, hipStreamSynchronize(st));  // (h_counts and the caller's buffers are pageable: read before this returns)
  if ((rc = rank_launch(c, *rp, B.hands, B.idx, B.counts, B.handles, margins ? B.marg : nullptr, B.tmp, B.out, (int) n_handles, B.scores,
         B.counts + 4, nullptr, 1, HandleSlots{ 0, 0, 0, 0 }, st)) != AGH_OK)
    return rc;
  int got[3] = { 0, 0, 0 };
  AGH_HIPCHK(c, hipMemcpyAsync(got, B.counts + 4, sizeof(got), hipMemcpyDeviceToHost, st));
  AGH_HIPCHK(c, hipStreamSynchronize(st));
  if (counts)
    *counts = agh_handle_ranking_counts{ got[0], got[1], got[2] };
  if (got[2] > cap)
  {
    c->err = "agh_rank_handles: room for " + std::to_string(got[2]) + " records is needed";
    return AGH_ERR_CAPACITY;
  }
  if (got[2] > 0 && handles_out)
    AGH_HIPCHK(c, hipMemcpy(handles_out, B.out, sizeof(agh_handle) * (size_t) got[2], hipMemcpyDeviceToHost));
  if (got[2] > 0 && scores_out)
    AGH_HIPCHK(c, hipMemcpy(scores_out, B.scores, sizeof(agh_handle_score) * (size_t) got[2], hipMemcpyDeviceToHost));
  return AGH_OK;
}

}  // extern "C"
