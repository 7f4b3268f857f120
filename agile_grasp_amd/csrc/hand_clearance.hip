// hand_clearance.hip -- agh_set_hand_clearance (include/agh.h; DESIGN.md, "Hand clearance"): the hands whose approach corridor -- an
// oriented box behind the palm, swept backwards along the approach -- holds more than max_points points of the capture's own
// voxelised cloud are dropped inside the localize chains, behind the hand filter and ahead of the classifier.  k_hand_clearance
// writes the hand drop stage's bytes and its own counter of a list (hand_drop.hip, whose stage calls hand_clearance_launch behind
// hand_filter_launch), so the classifier kernels and the compactions need nothing of its own.  The arithmetic is the contract's,
// float64, left to right, not contracted (-ffp-contract=off is the build's); tests/hand_clearance_cases.py is its numpy model.
#include "agh_internal.h"

#include <cmath>
#include <cstring>

using namespace agh;

namespace
{
constexpr int kHcBlock = 256;  // four waves, a hypothesis each
// The candidates come from the corridor's axis-aligned bounding box, which is exact for an orthonormal frame; the search's frames
// are orthonormal to rounding, and the box is widened by this factor and kHcPad metres so that rounding never costs a candidate.
constexpr double kHcWiden = 1.0001, kHcPad = 1e-6;

// the smallest and the largest value of v . (p - o) over the box lo <= p <= hi (interval arithmetic, per coordinate)
__device__ __forceinline__ void span_along(const double* v, const double* o, const double* lo, const double* hi, double* mn, double* mx)
{
  double a = 0.0, b = 0.0;
  for (int k = 0; k < 3; k++)
  {
    const double p = v[k] * (lo[k] - o[k]), q = v[k] * (hi[k] - o[k]);
    a += fmin(p, q);
    b += fmax(p, q);
  }
  *mn = a;
  *mx = b;
}

// One drop byte per hypothesis in[0, min(*n_in, cap_in)) and the lists' kDropClearance counter.  The launch is sized for the bound of the
// list and exits on the count.  A wave per hypothesis: the record, its list, its capture and the capture's grid descriptor are
// wave-uniform.  The corridor's bounding box becomes cell ranges (cell_coord clamps them as the build clamped the points, so the
// border cells of a kept descriptor, which hold the points outside its box, are always inside the range); every (y, z) row of the
// range is ONE run of the cell-sorted array.  64 rows at a time, a lane each, fetch their run from the cell table -- a row whose
// cell cannot meet the corridor is left out by interval arithmetic, border rows never -- then the wave walks the runs that hold
// points, a lane per point, the contract's test, a ballot and a popcount into a wave-uniform count.  The wave leaves once the
// count exceeds max_points: the decision is fixed then.  No LDS, no atomics on the count.
// has_drop: the bytes are written already (a dropped hand is skipped and stays dropped); else this kernel writes every byte.
// tab == null: the single chain's one list, capture 0; else list l = list_of_sample, capture tab[l].capture.
__global__ __launch_bounds__(kHcBlock) void k_hand_clearance(const agh_hypothesis* __restrict__ in, const int64_t* __restrict__ n_in,
  int64_t cap_in, HandClearanceArgs a, const BatchCapture* __restrict__ tab, int n_lists, GridView gv,
  const int32_t* __restrict__ samples, int64_t n_samples, const float* __restrict__ xyz, int64_t stride, int has_drop,
  uint8_t* __restrict__ drop, unsigned* __restrict__ counts)
{
  const int64_t n = min(*n_in, cap_in);
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t) blockIdx.x * (kHcBlock / 64) + (threadIdx.x >> 6);
  if (i >= n)  // (wave-uniform, as every branch below but the lanes' own tests)
    return;
  if (has_drop && drop[i])
    return;
  const agh_hypothesis& H = in[i];
  const int64_t sample = H.sample;
  const int l = tab ? list_of_sample(tab, n_lists, sample) : 0;
  const int capture = tab ? tab[l].capture : 0;
  const int64_t n_points = gv.cloud_off[gv.n_clouds];
  // (the guards of k_hand_filter: a record that names no position of the list, or an entry that is no point, steers no load)
  const int32_t idx = sample >= 0 && sample < n_samples ? samples[sample] : -1;
  int count = 0;
  if (idx >= 0 && idx < n_points && capture >= 0 && capture < gv.n_clouds)
  {
    const double s[3] = { (double) xyz[(int64_t) idx * stride + 0], (double) xyz[(int64_t) idx * stride + 1],
      (double) xyz[(int64_t) idx * stride + 2] };
    const double g0 = H.bottom[0] - s[0], g1 = H.bottom[1] - s[1], g2 = H.bottom[2] - s[2];
    const double h = (g0 * H.binormal[0] + g1 * H.binormal[1]) + g2 * H.binormal[2];
    const int di = min(max(H.depth_index, 0), a.n_depths - 1);
    const double y0 = a.depths[di] - a.hand_depth;
    double o[3], lo[3], hi[3];
    const double mid = -0.5 * (a.p.near_offset + a.p.far_offset), half_len = 0.5 * (a.p.far_offset - a.p.near_offset);
    for (int k = 0; k < 3; k++)
    {
      o[k] = (s[k] + h * H.binormal[k]) + y0 * H.approach[k];
      const double centre = o[k] + mid * H.approach[k];
      const double ext = ((half_len * fabs(H.approach[k]) + a.p.half_width * fabs(H.binormal[k])) + a.p.half_height * fabs(H.axis[k])) *
                           kHcWiden + kHcPad;
      lo[k] = centre - ext;
      hi[k] = centre + ext;
    }
    const GridView gc = grid_of_cloud(gv, capture);
    const GridDesc g = *gc.desc;
    const int p0 = gv.cloud_off[capture], p1 = gv.cloud_off[capture + 1];  // the capture's part of the cell-sorted array
    if (g.dim[0] >= 1 && g.dim[1] >= 1 && g.dim[2] >= 1)  // (a cloud without a grid has no hypotheses; nothing is indexed then)
    {
      // (a NaN bound ends in cell 0: cell_coord; the exact test then counts nothing)
      const int lx = cell_coord(g, lo[0], 0), hx = max(cell_coord(g, hi[0], 0), lx);
      const int ly = cell_coord(g, lo[1], 1), hy = max(cell_coord(g, hi[1], 1), ly);
      const int lz = cell_coord(g, lo[2], 2), hz = max(cell_coord(g, hi[2], 2), lz);
      const int ny = hy - ly + 1, nrows = ny * (hz - lz + 1);  // (at most dim[1] x dim[2] <= the cell table's size)
      for (int r0 = 0; r0 < nrows && count <= a.p.max_points; r0 += 64)
      {
        const int r = r0 + lane;
        int b = 0, len = 0;
        if (r < nrows)
        {
          const int q = r / ny, cy = ly + (r - q * ny), cz = lz + q;
          bool keep = true;
          // a row inside the grid holds points of its own (y, z) cell only: if no point of that cell, x anywhere in the corridor's
          // box, can satisfy the three closed tests (kHcPad to spare against their rounding), the row is left out.  A border row
          // may hold points from beyond the descriptor's box (GridDesc::open) and is never left out.
          if (cy > 0 && cy < g.dim[1] - 1 && cz > 0 && cz < g.dim[2] - 1)
          {
            const double blo[3] = { lo[0], g.mn[1] + cy * g.cell - kHcPad, g.mn[2] + cz * g.cell - kHcPad };
            const double bhi[3] = { hi[0], g.mn[1] + (cy + 1) * g.cell + kHcPad, g.mn[2] + (cz + 1) * g.cell + kHcPad };
            double mn, mx;
            span_along(H.approach, o, blo, bhi, &mn, &mx);
            const bool miss_y = mx < -a.p.far_offset - kHcPad || mn > -a.p.near_offset + kHcPad;
            span_along(H.binormal, o, blo, bhi, &mn, &mx);
            const bool miss_x = mx < -a.p.half_width - kHcPad || mn > a.p.half_width + kHcPad;
            span_along(H.axis, o, blo, bhi, &mn, &mx);
            const bool miss_z = mx < -a.p.half_height - kHcPad || mn > a.p.half_height + kHcPad;
            keep = !(miss_y || miss_x || miss_z);  // (a NaN compares false: nothing is left out)
          }
          if (keep)
          {
            const int base = (cz * g.dim[1] + cy) * g.dim[0];
            // (clamped to the capture's own part of the array: a run is never read outside it)
            b = max(gc.cell_start[base + lx], p0);
            len = min(gc.cell_start[base + hx + 1], p1) - b;
          }
        }
        unsigned long long rows = __ballot(len > 0);
        while (rows && count <= a.p.max_points)
        {
          const int k = __ffsll((long long) rows) - 1;
          rows &= rows - 1ull;
          const int rb = __shfl(b, k), rlen = __shfl(len, k);
          for (int j0 = 0; j0 < rlen && count <= a.p.max_points; j0 += 64)
          {
            bool inside = false;
            if (j0 + lane < rlen)
            {
              const float4 p = gc.sorted[rb + j0 + lane];
              const double e0 = (double) p.x - o[0], e1 = (double) p.y - o[1], e2 = (double) p.z - o[2];
              const double yb = (e0 * H.approach[0] + e1 * H.approach[1]) + e2 * H.approach[2];
              const double xb = (e0 * H.binormal[0] + e1 * H.binormal[1]) + e2 * H.binormal[2];
              const double zb = (e0 * H.axis[0] + e1 * H.axis[1]) + e2 * H.axis[2];
              inside = -a.p.far_offset <= yb && yb <= -a.p.near_offset && fabs(xb) <= a.p.half_width && fabs(zb) <= a.p.half_height;
            }
            count += __popcll(__ballot(inside));
          }
        }
      }
    }
  }
  if (lane == 0)
  {
    const bool dropped = count > a.p.max_points;
    drop[i] = dropped ? 1 : 0;
    if (dropped)
      atomicAdd(&counts[l * kHandDropCounters + kDropClearance], 1u);
  }
}

std::string clearance_fault(const agh_hand_clearance_params& p)
{
  const char* name[4] = { "near_offset", "far_offset", "half_width", "half_height" };
  const double value[4] = { p.near_offset, p.far_offset, p.half_width, p.half_height };
  for (int k = 0; k < 4; k++)
    if (!std::isfinite(value[k]))
      return std::string(name[k]) + " is not finite";
  if (p.near_offset < 0.0)
    return "near_offset must be >= 0";
  if (!(p.near_offset < p.far_offset) || p.far_offset > 0.5)
    return "far_offset must satisfy near_offset < far_offset <= 0.5";
  if (!(p.half_width > 0.0 && p.half_width <= 0.25))
    return "half_width must satisfy 0 < half_width <= 0.25";
  if (!(p.half_height > 0.0 && p.half_height <= 0.25))
    return "half_height must satisfy 0 < half_height <= 0.25";
  if (p.max_points < 0)
    return "max_points must be >= 0";
  return std::string();
}
}  // namespace

namespace agh
{
int hand_clearance_launch(Ctx* c, int64_t bound, const BatchCapture* tab, int n_lists, hipStream_t st, bool has_drop)
{
  const HandDropState& S = c->hand_drop;
  if (!S.clearance_set)
    return AGH_OK;
  HandClearanceArgs a;
  std::memset(&a, 0, sizeof(a));
  a.p = S.clearance;
  a.hand_depth = c->geom.hand_depth;
  a.n_depths = c->geom.n_depths;
  for (int k = 0; k < 16; k++)
    a.depths[k] = c->geom.depths[k];
  const GridView gv{ c->d_desc, c->d_cell_start, c->d_sorted, c->d_cloud_off, c->n_clouds };
  hipLaunchKernelGGL(k_hand_clearance, dim3((unsigned) ((bound + kHcBlock / 64 - 1) / (kHcBlock / 64))), dim3(kHcBlock), 0, st,
    (const agh_hypothesis*) c->d_out_own, (const int64_t*) c->d_nout, c->s_cap * 8, a, tab, n_lists, gv, (const int32_t*) c->d_idx_own,
    c->last_s, (const float*) c->d_xyz, c->stride_floats, has_drop ? 1 : 0, S.d_drop, S.d_counts);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "k_hand_clearance launch failed";
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}
}  // namespace agh

extern "C" {

void agh_default_hand_clearance_params(agh_hand_clearance_params* p)
{
  if (!p)
    return;
  std::memset(p, 0, sizeof(*p));
  p->near_offset = 0.0;
  p->far_offset = 0.12;
  p->half_width = 0.05;
  p->half_height = 0.04;
  p->max_points = 0;
}

int agh_set_hand_clearance(agh_ctx* ctx, const agh_hand_clearance_params* cp)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_set_hand_clearance"))
    return AGH_ERR_STATE;
  if (c->batch_active)
  {
    c->err = "agh_set_hand_clearance: an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  if (!cp)
  {
    c->hand_drop.clearance_set = false;
    return AGH_OK;
  }
  const std::string fault = clearance_fault(*cp);
  if (!fault.empty())
  {
    c->err = "agh_set_hand_clearance: " + fault;
    return AGH_ERR_INVALID_ARGUMENT;
  }
  c->hand_drop.clearance = *cp;
  c->hand_drop.clearance.reserved = 0;
  c->hand_drop.clearance_set = true;
  return AGH_OK;
}

int agh_get_hand_clearance(agh_ctx* ctx, agh_hand_clearance_params* out)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (!c->hand_drop.clearance_set)
    return 0;
  if (!out)
  {
    c->err = "agh_get_hand_clearance: out is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  *out = c->hand_drop.clearance;
  return 1;
}

int agh_get_hand_clearance_counts(agh_ctx* ctx, agh_hand_clearance_counts* out, int32_t cap_lists)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_hand_clearance_counts"))
    return AGH_ERR_STATE;
  const int lists = c->hand_drop.lists;
  if (!c->hand_drop.clearance_ran || lists == 0)
    return 0;
  if (cap_lists < lists || !out)
  {
    c->err = "agh_get_hand_clearance_counts: room for " + std::to_string(lists) + " lists is needed";
    return AGH_ERR_CAPACITY;
  }
  for (int k = 0; k < lists; k++)
  {
    const HandDropCounts n = hand_drop_counts(c, k);
    out[k].n_tested = n.past_filter();
    out[k].n_dropped = n.clearance;
    out[k].n_kept = out[k].n_tested - out[k].n_dropped;
  }
  return lists;
}

}  // extern "C"
