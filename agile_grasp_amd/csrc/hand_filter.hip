// hand_filter.hip -- agh_set_hand_filter (include/agh.h; DESIGN.md, "Hand filter"): the hands a cell cannot execute are dropped
// inside the localize chains, between the search and the classifier.  k_hand_filter writes one drop byte per hypothesis of the
// search's list and counts, per list of the chain, the hands each criterion dropped; k_hog_svm / k_svm_decide label a dropped
// hand 0 without classifying it and compact_kept_records leaves it out, so the handle search (and its 8192-hand limit) sees the
// survivors only.  The arithmetic is the contract's, float64, left to right, not contracted (-ffp-contract=off is the build's);
// tests/hand_filter_cases.py is its numpy model.  The bytes, the counters and what a chain leaves are hand_drop.hip's, whose stage
// calls hand_filter_launch.
#include "agh_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace agh;

namespace
{
constexpr int kHfBlock = 256;  // four waves

// criteria 1 and 2 on a record's own doubles: 0 kept, else 1 + the counter of the criterion the hand fails (the approach cone,
// then the aperture)
__device__ __forceinline__ int cone_and_aperture(const agh_hypothesis& H, const agh_hand_filter_params& p)
{
  if (p.approach_on)
  {
    const double dot = (H.approach[0] * p.approach_dir[0] + H.approach[1] * p.approach_dir[1]) + H.approach[2] * p.approach_dir[2];
    if (dot < p.min_approach_cos)
      return 1 + kDropApproach;
  }
  if (p.width_on && (H.width < p.min_width || H.width > p.max_width))
    return 1 + kDropWidth;
  return 0;
}

// is the probe w seen in view V: in front of the camera, on a valid pixel of the image, and not behind that pixel's surface
// (beyond depth_margin)?  The pixel's depth is k_deproject's float32 z.  The row and the column are tested as doubles, so the
// conversions below see values in [0, h) and [0, w) only and the load stays inside the image.
__device__ __forceinline__ bool probe_seen(const HandView& V, double w0, double w1, double w2, double margin)
{
  const double e0 = w0 - V.t[0], e1 = w1 - V.t[1], e2 = w2 - V.t[2];
  const double qx = (V.R[0] * e0 + V.R[3] * e1) + V.R[6] * e2;
  const double qy = (V.R[1] * e0 + V.R[4] * e1) + V.R[7] * e2;
  const double qz = (V.R[2] * e0 + V.R[5] * e1) + V.R[8] * e2;
  if (!(qz > 0.0))
    return false;
  const double u = floor(((V.fx * qx) / qz + V.cx) + 0.5);
  const double v = floor(((V.fy * qy) / qz + V.cy) + 0.5);
  if (!(u >= 0.0 && u < (double) V.w && v >= 0.0 && v < (double) V.h))
    return false;
  const uint8_t* row = V.data + (int64_t) v * V.stride;
  float z;
  bool ok;
  if (V.fmt == AGH_DEPTH_U16)
  {
    const uint32_t raw = reinterpret_cast<const uint16_t*>(row)[(int) u];
    z = (float) raw * V.scale;
    ok = raw != 0;
  }
  else
  {
    z = reinterpret_cast<const float*>(row)[(int) u];
    ok = z > 0.0f && z < __builtin_huge_valf();
  }
  return ok && qz <= (double) z + margin;
}

// One drop byte per hypothesis in[0, min(*n_in, cap_in)) and the lists' counters (kHandDropCounters per list; this kernel's
// are approach, width and unobserved).  The launch is sized for the bound of the list and exits on the count.
// VIEW = false: a lane per hypothesis.  VIEW = true: a wave per hypothesis, so that the list, the capture and its views are
// wave-uniform and the view records are read with scalar loads; the lanes take the hand's 2 x n x 3 <= 96 probes, two rounds
// with a ballot each, every lane testing its probe against the capture's one or two views in turn; lane 0 writes the byte and
// bumps the counter.
// tab == null: the single chain's one list, its views in `pair`; else list l = list_of_sample, capture tab[l].capture, whose views
// are table[vfirst[capture]] .. table[vfirst[capture + 1] - 1].
template <bool VIEW>
__global__ __launch_bounds__(kHfBlock) void k_hand_filter(const agh_hypothesis* __restrict__ in, const int64_t* __restrict__ n_in,
  int64_t cap_in, HandFilterArgs a, const BatchCapture* __restrict__ tab, int n_lists, HandViewPair pair,
  const HandView* __restrict__ table, const int32_t* __restrict__ vfirst, const int32_t* __restrict__ samples, int64_t n_samples,
  const float* __restrict__ xyz, int64_t stride, const int* __restrict__ cloud_off, int n_clouds, uint8_t* __restrict__ drop,
  unsigned* __restrict__ counts)
{
  const int64_t n = min(*n_in, cap_in);
  if (!VIEW)
  {
    const int64_t i = (int64_t) blockIdx.x * kHfBlock + threadIdx.x;
    if (i >= n)
      return;
    const int reason = cone_and_aperture(in[i], a.p);
    drop[i] = reason ? 1 : 0;
    if (reason)
      atomicAdd(&counts[(tab ? list_of_sample(tab, n_lists, in[i].sample) : 0) * kHandDropCounters + reason - 1], 1u);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t) blockIdx.x * (kHfBlock / 64) + (threadIdx.x >> 6);
  if (i >= n)  // (wave-uniform)
    return;
  const agh_hypothesis& H = in[i];
  const int64_t sample = H.sample;
  const int l = tab ? list_of_sample(tab, n_lists, sample) : 0;
  int reason = cone_and_aperture(H, a.p);
  const int64_t n_points = cloud_off[n_clouds];
  // (the search made the record from this position of the list, whose entry is a point of the cloud: the tests keep a record
  // that says otherwise from steering a load)
  const int32_t idx = sample >= 0 && sample < n_samples ? samples[sample] : -1;
  if (reason == 0 && idx >= 0 && idx < n_points)
  {
    const int capture = tab ? tab[l].capture : 0;
    const int first = tab ? vfirst[capture] : 0;
    const int nv = tab ? vfirst[capture + 1] - first : pair.n;
    const double s0 = (double) xyz[(int64_t) idx * stride + 0], s1 = (double) xyz[(int64_t) idx * stride + 1],
                 s2 = (double) xyz[(int64_t) idx * stride + 2];
    const double g0 = H.bottom[0] - s0, g1 = H.bottom[1] - s1, g2 = H.bottom[2] - s2;
    const double h = (g0 * H.binormal[0] + g1 * H.binormal[1]) + g2 * H.binormal[2];
    const int di = min(max(H.depth_index, 0), a.n_depths - 1);
    const double y0 = a.depths[di] - a.hand_depth;
    const int np = a.p.probes_per_finger, per_finger = 3 * np, P = 2 * per_finger;
    int unobserved = 0;
    for (int p0 = 0; p0 < P; p0 += 64)
    {
      const int p = p0 + lane;
      bool unobs = false;
      if (p < P)
      {
        const int f = p / per_finger, r = p - f * per_finger, j = r / 3, m = r - 3 * j;
        const double cb = f == 0 ? h - a.finger_off : h + a.finger_off;
        const double y = y0 + ((double) j + 0.5) * a.step;
        const double z = m == 0 ? -a.hand_height : (m == 1 ? 0.0 : a.hand_height);
        const double w0 = ((s0 + cb * H.binormal[0]) + y * H.approach[0]) + z * H.axis[0];
        const double w1 = ((s1 + cb * H.binormal[1]) + y * H.approach[1]) + z * H.axis[1];
        const double w2 = ((s2 + cb * H.binormal[2]) + y * H.approach[2]) + z * H.axis[2];
        bool seen = false;
        for (int k = 0; k < nv; k++)  // (uniform: the record comes by scalar loads)
          seen |= probe_seen(tab ? table[first + k] : pair.v[k], w0, w1, w2, a.p.depth_margin);
        unobs = !seen && w0 == w0 && w1 == w1 && w2 == w2;  // (a NaN probe is not counted: the hand is kept, as include/agh.h says)
      }
      unobserved += __popcll(__ballot(unobs));
    }
    if (unobserved > a.p.max_unobserved)
      reason = 1 + kDropUnobserved;
  }
  if (lane == 0)
  {
    drop[i] = reason ? 1 : 0;
    if (reason)
      atomicAdd(&counts[l * kHandDropCounters + reason - 1], 1u);
  }
}

std::string params_fault(const agh_hand_filter_params& p)
{
  const int32_t flags[3] = { p.approach_on, p.width_on, p.view_on };
  const char* flag_name[3] = { "approach_on", "width_on", "view_on" };
  for (int k = 0; k < 3; k++)
    if (flags[k] != 0 && flags[k] != 1)
      return std::string(flag_name[k]) + " must be 0 or 1";
  const double* d = p.approach_dir;
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(d[k]))
      return "approach_dir[" + std::to_string(k) + "] is not finite";
  if (std::fabs(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0) > 1e-6)
    return "approach_dir must be a unit vector (|a^2 + b^2 + c^2 - 1| <= 1e-6)";
  if (!(p.min_approach_cos >= -1.0 && p.min_approach_cos <= 1.0))
    return "min_approach_cos must be in [-1, 1]";
  if (!std::isfinite(p.min_width) || !std::isfinite(p.max_width) || p.min_width < 0.0 || p.min_width > p.max_width)
    return "min_width and max_width must be finite with 0 <= min_width <= max_width";
  if (p.probes_per_finger < 1 || p.probes_per_finger > 16)
    return "probes_per_finger must be 1 .. 16";
  if (!std::isfinite(p.depth_margin) || p.depth_margin < 0.0)
    return "depth_margin must be finite and >= 0";
  if (p.max_unobserved < 0)
    return "max_unobserved must be >= 0";
  return std::string();
}
}  // namespace

namespace agh
{
int hand_filter_check(Ctx* c, const char* who, const agh_depth_image* images, const int32_t* n_images, int C, bool has_depth)
{
  if (!c->hand_drop.filter_set || !c->hand_drop.filter.view_on)
    return AGH_OK;
  if (!has_depth)
  {
    c->err = std::string(who) + ": the hand filter's observed-space criterion (view_on) needs depth images: call an "
             "agh_localize_depth* form, or set a filter without view_on";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  for (int cap = 0, k = 0; cap < C; cap++)
   for (int j = 0; j < n_images[cap]; j++, k++)
   {
    const double* P = images[k].pose;
    double worst = 0.0;  // the largest entry of |R^T R - I|
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
      {
        const double g = (P[0 + i] * P[0 + j] + P[4 + i] * P[4 + j]) + P[8 + i] * P[8 + j];  // (R^T R)_ij
        worst = std::max(worst, std::fabs(g - (i == j ? 1.0 : 0.0)));
      }
    if (!(worst <= 1e-4))
    {
      // (a batch's text names the capture too, as depth_check's)
      c->err = std::string(who) + ": " + (C > 1 ? "capture " + std::to_string(cap) + ", " : std::string()) + "image " +
               std::to_string(j) + ": the hand filter's observed-space criterion needs an "
               "orthonormal rotation in pose (every entry of |R^T R - I| <= 1e-4)";
      return AGH_ERR_INVALID_ARGUMENT;
    }
   }
  return AGH_OK;
}

void hand_filter_keep_views(Ctx* c, const agh_depth_image* images, const int32_t* n_images, int C, const uint8_t* const* data,
  const int64_t* stride)
{
  HandDropState& S = c->hand_drop;
  S.views.clear();
  S.view_first.assign(1, 0);
  if (!S.filter_set || !S.filter.view_on)
    return;
  int j = 0;
  for (int k = 0; k < C; k++)
  {
    for (int q = 0; q < n_images[k]; q++, j++)
    {
      const agh_depth_image& im = images[j];
      HandView v;
      std::memset(&v, 0, sizeof(v));
      v.data = data[j];
      v.stride = stride[j];
      v.w = im.width;
      v.h = im.height;
      v.fmt = im.format;
      v.scale = im.depth_scale;
      v.fx = im.fx;
      v.fy = im.fy;
      v.cx = im.cx;
      v.cy = im.cy;
      for (int r = 0; r < 3; r++)
      {
        for (int s = 0; s < 3; s++)
          v.R[3 * r + s] = im.pose[4 * r + s];
        v.t[r] = im.pose[4 * r + 3];
      }
      S.views.push_back(v);
    }
    S.view_first.push_back(j);
  }
}

// k_hand_filter queued on st, a batch's view table uploaded in front of it: every drop byte and the filter's counters
int hand_filter_launch(Ctx* c, int64_t bound, const BatchCapture* tab, int n_lists, hipStream_t st)
{
  HandDropState& S = c->hand_drop;
  if (!S.filter_set)
    return AGH_OK;
  static_assert(sizeof(HandView) % 8 == 0, "the table's records are read with scalar loads");
  const agh_hand_filter_params& p = S.filter;
  const int64_t cap = c->s_cap * 8;
  HandFilterArgs a;
  std::memset(&a, 0, sizeof(a));
  a.p = p;
  a.finger_off = c->geom.hand_outer_diameter / 2.0 - c->geom.finger_width / 2.0;
  a.hand_depth = c->geom.hand_depth;
  a.hand_height = c->geom.hand_height;
  a.step = c->geom.hand_depth / (double) p.probes_per_finger;
  a.n_depths = c->geom.n_depths;
  for (int k = 0; k < 16; k++)
    a.depths[k] = c->geom.depths[k];
  HandViewPair pair;
  std::memset(&pair, 0, sizeof(pair));
  const HandView* d_table = nullptr;
  const int32_t* d_vfirst = nullptr;
  if (p.view_on)
  {
    const int views = (int) S.views.size();
    const int captures = (int) S.view_first.size() - 1;
    if (views < 1 || views > kMaxHandViews || captures < 1 || captures > kMaxClouds)
    {
      c->err = "the hand filter's observed-space criterion has no views for this chain";
      return AGH_ERR_INVALID_ARGUMENT;
    }
    if (tab)
    {
      std::memcpy(S.h_views, S.views.data(), sizeof(HandView) * (size_t) views);
      std::memcpy(S.h_views + sizeof(HandView) * (size_t) kMaxHandViews, S.view_first.data(),
        sizeof(int32_t) * (size_t) (captures + 1));
      AGH_HIPCHK(c, hipMemcpyAsync(S.d_views, S.h_views, kHandViewTableBytes, hipMemcpyHostToDevice, st));
      d_table = reinterpret_cast<const HandView*>(S.d_views);
      d_vfirst = reinterpret_cast<const int32_t*>(S.d_views + sizeof(HandView) * (size_t) kMaxHandViews);
    }
    else
    {
      pair.n = std::min(views, 2);
      for (int k = 0; k < pair.n; k++)
        pair.v[k] = S.views[(size_t) k];
    }
    hipLaunchKernelGGL(k_hand_filter<true>, dim3((unsigned) ((bound + kHfBlock / 64 - 1) / (kHfBlock / 64))), dim3(kHfBlock), 0, st,
      (const agh_hypothesis*) c->d_out_own, (const int64_t*) c->d_nout, cap, a, tab, n_lists, pair, d_table, d_vfirst,
      (const int32_t*) c->d_idx_own, c->last_s, c->d_xyz, c->stride_floats, (const int*) c->d_cloud_off, c->n_clouds, S.d_drop,
      S.d_counts);
  }
  else
    hipLaunchKernelGGL(k_hand_filter<false>, dim3((unsigned) ((bound + kHfBlock - 1) / kHfBlock)), dim3(kHfBlock), 0, st,
      (const agh_hypothesis*) c->d_out_own, (const int64_t*) c->d_nout, cap, a, tab, n_lists, pair, d_table, d_vfirst,
      (const int32_t*) c->d_idx_own, c->last_s, c->d_xyz, c->stride_floats, (const int*) c->d_cloud_off, c->n_clouds, S.d_drop,
      S.d_counts);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "k_hand_filter launch failed";
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}
}  // namespace agh

extern "C" {

void agh_default_hand_filter_params(agh_hand_filter_params* p)
{
  if (!p)
    return;
  std::memset(p, 0, sizeof(*p));
  p->probes_per_finger = 4;
  p->approach_dir[2] = 1.0;
  p->min_approach_cos = -1.0;
  p->min_width = 0.0;
  p->max_width = 0.1;
  p->depth_margin = 0.01;
  p->max_unobserved = 0;
}

int agh_set_hand_filter(agh_ctx* ctx, const agh_hand_filter_params* fp)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_set_hand_filter"))
    return AGH_ERR_STATE;
  if (c->batch_active)
  {
    c->err = "agh_set_hand_filter: an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  if (!fp)
  {
    c->hand_drop.filter_set = false;
    return AGH_OK;
  }
  const std::string fault = params_fault(*fp);
  if (!fault.empty())
  {
    c->err = "agh_set_hand_filter: " + fault;
    return AGH_ERR_INVALID_ARGUMENT;
  }
  c->hand_drop.filter = *fp;
  c->hand_drop.filter.reserved = 0;
  c->hand_drop.filter_set = true;
  return AGH_OK;
}

int agh_get_hand_filter(agh_ctx* ctx, agh_hand_filter_params* out)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (!c->hand_drop.filter_set)
    return 0;
  if (!out)
  {
    c->err = "agh_get_hand_filter: out is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  *out = c->hand_drop.filter;
  return 1;
}

int agh_get_hand_filter_counts(agh_ctx* ctx, agh_hand_filter_counts* out, int32_t cap_lists)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_hand_filter_counts"))
    return AGH_ERR_STATE;
  const int lists = c->hand_drop.lists;
  if (!c->hand_drop.filter_ran || lists == 0)
    return 0;
  if (cap_lists < lists || !out)
  {
    c->err = "agh_get_hand_filter_counts: room for " + std::to_string(lists) + " lists is needed";
    return AGH_ERR_CAPACITY;
  }
  for (int k = 0; k < lists; k++)
  {
    const HandDropCounts n = hand_drop_counts(c, k);
    out[k].n_hypotheses = n.hypotheses;
    out[k].n_dropped_approach = n.approach;
    out[k].n_dropped_width = n.width;
    out[k].n_dropped_unobserved = n.unobserved;
    out[k].n_kept = n.past_filter();
  }
  return lists;
}

}  // extern "C"
