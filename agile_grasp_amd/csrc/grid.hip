// grid.hip -- K0: uniform-grid build (cell histogram, scan, cell-major scatter; a bounding box on cold builds).
//
// Stands in for pcl::KdTreeFLANN::setInputCloud (reference src/agile_grasp/hand_search.cpp:10-11): the search
// structure behind the three radius searches of the hot path.  The cloud is re-laid out cell-major as
// float4 {x, y, z, bits((index << 1) | cam)} so that a ball query is a handful of contiguous runs read with
// coalesced 16-byte loads.  Everything runs on the device without a host round trip: the grid descriptor
// (origin, cell size, dimensions) lives in device memory and later kernels read it from there.
//
// Which descriptor a build uses does not change a single result: the searches only see neighbour SETS, and a point outside
// the descriptor's box is clamped into a border cell whose face is then marked open (GridDesc::open, build_rows), so every ball
// that reaches the point still reaches its cell.  Only the cell size matters (it bounds the rows of a ball query), and it
// follows the rule of desc_finish.  So a build does not wait for its own cloud's bounding box: it bins the points into the
// descriptor the previous build decided (Ctx::d_desc_next), and k_cell_scan decides the next one from the extrema that
// k_cell_count leaves behind -- the same one again while it covers the cloud and is not much larger than needed.  A cold
// build (a context's first, one after a failed build, a batch of another size) takes the bounding box first (k_bbox), as before.
#include "agh_internal.h"

#include <algorithm>
#include <cstdlib>

namespace agh
{

// Reset state of the self-cleaning fields (also written once by agh_create / after a failed build).
__global__ void k_desc_reset(GridDesc* d)
{
  d += blockIdx.x;
  d->open = 0u;
  d->ticket = 0u;
}

__device__ void desc_finish(GridDesc* d, double base_cell, int64_t n, const float lo[3], const float hi[3])
{
  double mn[3], mx[3];
  for (int a = 0; a < 3; a++)
  {
    // (an empty cloud, or one without a single finite point, leaves the sentinels: a one-cell grid at the origin)
    const bool any = n > 0 && lo[a] <= hi[a];
    mn[a] = any ? (double) lo[a] : 0.0;
    mx[a] = any ? (double) hi[a] : 0.0;
  }
  // The cell doubles until the grid fits kCellCap cells.  The counts stay in double until they do: an extent of 1e9 cells and
  // more (two finite points 2e30 m apart are a valid float32 cloud) does not fit an int, and a converted count that wrapped
  // would end the loop with a negative product.  Every count is >= 1, so a product <= kCellCap bounds each of them by kCellCap
  // and the conversion below is exact.  The loop ends: a doubling halves every quotient, the largest one (float32 extents:
  // below 2^129 / 0.02 < 2^135) drops below 1 after at most 135 of them, and 0.02 x 2^135 is far from overflowing a double.
  double cell = base_cell;
  double cnt[3];
  for (;;)
  {
    double prod = 1.0;
    for (int a = 0; a < 3; a++)
    {
      cnt[a] = floor((mx[a] - mn[a]) / cell) + 1.0;
      prod *= cnt[a];
    }
    if (prod <= (double) kCellCap)
      break;
    cell *= 2.0;
  }
  int dim[3];
  for (int a = 0; a < 3; a++)
  {
    dim[a] = (int) cnt[a];
    d->mn[a] = mn[a];
    d->dim[a] = dim[a];
  }
  d->cell = cell;
  d->inv_cell = 1.0 / cell;
  d->ncell = dim[0] * dim[1] * dim[2];
}

// Bounding box of the cloud, first half: every work-group leaves its six extrema in its own slot of `part` (plain stores).
// The second half -- the reduction of the (<= 128) slots and the grid descriptor -- is done by EVERY work-group of
// k_cell_count for itself, behind its own point load: the "last work-group finishes" form of this kernel (slot stores, fence,
// arrival counter, fence, agent-scope reads of the slots, descriptor) was a chain of four memory round trips inside one
// launch, 8.2 us for a 300k-point cloud of which the point loop is two.  (Six atomicMin/Max per work-group on one cache
// line, the form before that: 9.8 us.)
constexpr int kBboxThreads = 1024;
__global__ __launch_bounds__(kBboxThreads) void k_bbox(const float* __restrict__ xyz, int64_t stride, const int* __restrict__ cloud_off,
  float* __restrict__ part)
{
  // blockIdx.y = cloud of the batch
  const int64_t p0 = cloud_off[blockIdx.y], n = cloud_off[blockIdx.y + 1] - p0;
  xyz += p0 * stride;
  part += (int64_t) blockIdx.y * kBboxBlocks * 6;
  float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
  // (the loop is latency bound: 131072 threads, two points in flight per thread, so a 300k-point cloud takes two rounds)
  const int64_t step = (int64_t) gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x; i < n; i += 2 * step)
  {
    const float* p = xyz + i * stride;
    const float* q = xyz + (i + step < n ? i + step : i) * stride;
    const float pv[3] = { p[0], p[1], p[2] }, qv[3] = { q[0], q[1], q[2] };
    // a point with a non-finite coordinate is no point of the search structure (pcl::KdTreeFLANN::setInputCloud drops it:
    // it can be nobody's neighbour) and does not stretch the box
    const bool pf = isfinite(pv[0]) && isfinite(pv[1]) && isfinite(pv[2]), qf = isfinite(qv[0]) && isfinite(qv[1]) && isfinite(qv[2]);
    for (int a = 0; a < 3; a++)
    {
      mn[a] = fminf(mn[a], fminf(pf ? pv[a] : INFINITY, qf ? qv[a] : INFINITY));
      mx[a] = fmaxf(mx[a], fmaxf(pf ? pv[a] : -INFINITY, qf ? qv[a] : -INFINITY));
    }
  }
  constexpr int kW = kBboxThreads / 64;
  __shared__ float smn[kW][3], smx[kW][3];
  for (int a = 0; a < 3; a++)
    for (int o = 32; o > 0; o >>= 1)
    {
      mn[a] = fminf(mn[a], __shfl_down(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_down(mx[a], o));
    }
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; a++)
    {
      smn[threadIdx.x >> 6][a] = mn[a];
      smx[threadIdx.x >> 6][a] = mx[a];
    }
  __syncthreads();
  if (threadIdx.x < 3)
  {
    const int a = threadIdx.x;
    float lo = smn[0][a], hi = smx[0][a];
    for (int w = 1; w < kW; w++)
    {
      lo = fminf(lo, smn[w][a]);
      hi = fmaxf(hi, smx[w][a]);
    }
    part[blockIdx.x * 6 + a] = lo;
    part[blockIdx.x * 6 + 3 + a] = hi;
  }
}

static_assert(kCountBlocks % 256 == 0, "reduce_parts: whole rounds of 256 slots");

// Minima and maxima of three coordinates over the wave, on every lane (DPP / permlane moves: no LDS round trips).
__device__ __forceinline__ void wave_minmax3(float lo[3], float hi[3])
{
  for (int a = 0; a < 3; a++)
  {
    lo[a] = fminf(lo[a], __int_as_float(xor_partner_i32<32>(__float_as_int(lo[a]))));
    hi[a] = fmaxf(hi[a], __int_as_float(xor_partner_i32<32>(__float_as_int(hi[a]))));
    lo[a] = fminf(lo[a], __int_as_float(xor_partner_i32<16>(__float_as_int(lo[a]))));
    hi[a] = fmaxf(hi[a], __int_as_float(xor_partner_i32<16>(__float_as_int(hi[a]))));
    lo[a] = fminf(lo[a], __int_as_float(xor_partner_i32<8>(__float_as_int(lo[a]))));
    hi[a] = fmaxf(hi[a], __int_as_float(xor_partner_i32<8>(__float_as_int(hi[a]))));
    lo[a] = fminf(lo[a], __int_as_float(xor_partner_i32<4>(__float_as_int(lo[a]))));
    hi[a] = fmaxf(hi[a], __int_as_float(xor_partner_i32<4>(__float_as_int(hi[a]))));
    lo[a] = fminf(lo[a], __int_as_float(xor_partner_i32<2>(__float_as_int(lo[a]))));
    hi[a] = fmaxf(hi[a], __int_as_float(xor_partner_i32<2>(__float_as_int(hi[a]))));
    lo[a] = fminf(lo[a], __int_as_float(xor_partner_i32<1>(__float_as_int(lo[a]))));
    hi[a] = fmaxf(hi[a], __int_as_float(xor_partner_i32<1>(__float_as_int(hi[a]))));
  }
}

// The reduction of `nparts` slots of six extrema by one work-group (256 threads): thread 0 ends with the cloud's box.
__device__ __forceinline__ void reduce_parts(const float* __restrict__ part, int nparts, float lo[3], float hi[3])
{
  __shared__ float red[4][6];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int a = 0; a < 3; a++)
  {
    lo[a] = INFINITY;
    hi[a] = -INFINITY;
  }
  // (nparts <= kCountBlocks = 8 x 256: unrolled, so that all of a thread's slot loads are in flight at once -- the slots were
  // written by other XCDs, one round trip each)
#pragma unroll
  for (int k = 0; k < kCountBlocks / 256; k++)
  {
    const int b = tid + 256 * k;
    if (b < nparts)
      for (int a = 0; a < 3; a++)
      {
        lo[a] = fminf(lo[a], part[b * 6 + a]);
        hi[a] = fmaxf(hi[a], part[b * 6 + 3 + a]);
      }
  }
  wave_minmax3(lo, hi);
  if (lane == 0 && tid < 256)
    for (int a = 0; a < 3; a++)
    {
      red[tid >> 6][a] = lo[a];
      red[tid >> 6][3 + a] = hi[a];
    }
  __syncthreads();
  if (tid == 0)
    for (int a = 0; a < 3; a++)
      for (int w = 1; w < 4; w++)
      {
        lo[a] = fminf(lo[a], red[w][a]);
        hi[a] = fmaxf(hi[a], red[w][3 + a]);
      }
}

// The reduction of k_bbox's slots and the grid descriptor, by one work-group for itself (256 threads; `g` in LDS).
__device__ __forceinline__ void desc_from_parts(const float* __restrict__ part, int nparts, double base_cell, int64_t n, GridDesc* g)
{
  float lo[3], hi[3];
  reduce_parts(part, nparts, lo, hi);
  if (threadIdx.x == 0)
    desc_finish(g, base_cell, n, lo, hi);
  __syncthreads();
}

// Cell histogram.  Clouds arrive in voxel order (localization.cpp:282-351), so consecutive points mostly share a cell:
// each run of equal cells inside a wave issues ONE atomic (with return), and every point remembers its rank inside its
// cell, which makes the scatter below atomic-free.
// COLD: the descriptor from k_bbox's slots, every work-group for itself (a cold build).  Otherwise the kept descriptor of the
// cloud, one scalar load.  Either way the first work-group of a cloud publishes the descriptor it bins into for the kernels
// after this one, and every work-group leaves the extrema of its finite points in its slot of `part_out` for k_cell_scan.
template <bool COLD>
__global__ __launch_bounds__(256) void k_cell_count(const float* __restrict__ xyz, int64_t stride,
  const int* __restrict__ cloud_off, GridDesc* __restrict__ d, const GridDesc* __restrict__ kept, int* __restrict__ cell_of,
  int* __restrict__ rank_of, int* __restrict__ count, const float* __restrict__ part, int nparts, double base_cell,
  float* __restrict__ part_out)
{
  const int64_t p0 = cloud_off[blockIdx.y], n = cloud_off[blockIdx.y + 1] - p0;
  xyz += p0 * stride;
  cell_of += p0;
  rank_of += p0;
  count += (int64_t) blockIdx.y * kCellCap;
  GridDesc g;
  if (COLD)
  {
    __shared__ GridDesc gs;
    desc_from_parts(part + (int64_t) blockIdx.y * kBboxBlocks * 6, nparts, base_cell, n, &gs);
    g = gs;
  }
  else
    g = kept[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    GridDesc* o = d + blockIdx.y;  // (field by field: `ticket` belongs to k_cell_scan)
    for (int a = 0; a < 3; a++)
    {
      o->mn[a] = g.mn[a];
      o->dim[a] = g.dim[a];
    }
    o->cell = g.cell;
    o->inv_cell = g.inv_cell;
    o->ncell = g.ncell;
    o->open = 0u;  // (k_cell_scan opens the faces the cloud crosses)
  }
  float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t) gridDim.x * blockDim.x;
  const int64_t n_up = (n + 63) & ~(int64_t) 63;  // whole waves iterate together (the shuffles below need all lanes)
  for (int64_t i = blockIdx.x * (int64_t) blockDim.x + threadIdx.x; i < n_up; i += step)
  {
    int c = -1;
    if (i < n)
    {
      const float* p = xyz + i * stride;
      const float px = p[0], py = p[1], pz = p[2];
      const int cx = cell_coord(g, (double) px, 0), cy = cell_coord(g, (double) py, 1), cz = cell_coord(g, (double) pz, 2);
      c = (cz * g.dim[1] + cy) * g.dim[0] + cx;
      // A non-finite point keeps its place in the index space (the callers' indices do not move) and its own coordinates in the
      // sorted array, where every query's float32 distance test rejects it (NaN and Inf compare false with `< r^2`); which cell
      // it lies in is therefore free -- spread over the cells by index, so that no cell collects a sensor's drop-outs.  It does
      // not stretch the box either (pcl::KdTreeFLANN::setInputCloud drops it: it can be nobody's neighbour).
      if (!(isfinite(px) && isfinite(py) && isfinite(pz)))
        c = (int) (i % (int64_t) g.ncell);
      else
      {
        mn[0] = fminf(mn[0], px);
        mn[1] = fminf(mn[1], py);
        mn[2] = fminf(mn[2], pz);
        mx[0] = fmaxf(mx[0], px);
        mx[1] = fmaxf(mx[1], py);
        mx[2] = fmaxf(mx[2], pz);
      }
    }
    const int prev = __shfl_up(c, 1);
    const bool head = (lane == 0) || (c != prev);
    const unsigned long long hm = __ballot(head);
    const int hl = 63 - __clzll((long long) (hm & ((2ull << lane) - 1ull)));  // head lane of this lane's run
    const unsigned long long after = (hl == 63) ? 0ull : (hm >> (hl + 1));
    const int runlen = after ? (__ffsll((long long) after)) : (64 - hl);
    int base = 0;
    if (head && c >= 0)
      base = atomicAdd(&count[c], runlen);
    base = __shfl(base, hl);
    if (i < n)
    {
      cell_of[i] = c;
      rank_of[i] = base + (lane - hl);
    }
  }
  // the work-group's extrema into its slot (after the point loop: its atomics are in flight meanwhile)
  __shared__ float smn[4][3], smx[4][3];
  wave_minmax3(mn, mx);
  if (lane == 0)
    for (int a = 0; a < 3; a++)
    {
      smn[threadIdx.x >> 6][a] = mn[a];
      smx[threadIdx.x >> 6][a] = mx[a];
    }
  __syncthreads();
  if (threadIdx.x < 3)
  {
    const int a = threadIdx.x;
    const float lo = fminf(fminf(smn[0][a], smn[1][a]), fminf(smn[2][a], smn[3][a]));
    const float hi = fmaxf(fmaxf(smx[0][a], smx[1][a]), fmaxf(smx[2][a], smx[3][a]));
    float* slot = part_out + ((int64_t) blockIdx.y * kCountBlocks + blockIdx.x) * 6;
    slot[a] = lo;
    slot[3 + a] = hi;
  }
}

// The descriptor the next build of a cloud keeps, from the descriptor `u` this build used and the cloud's true box (thread 0 of
// one work-group of k_cell_scan).  Faces of `u` the cloud crosses are opened in the used descriptor (the searches then treat
// their border layers as unbounded) and the build counts as a miss.  `u` is kept while it covers the cloud, has the cell size
// the cloud's own box would give, and exceeds that box by at most 4 kGridMargin cells along every axis; otherwise the next
// build takes the cloud's box padded by kGridMargin cells on every face (none if the padded grid would pass kCellCap).  The
// descriptor of a cold build is the unpadded box: never kept.
__device__ void desc_next(const GridDesc u, GridDesc* used, GridDesc* next, unsigned* miss, double base_cell, int64_t n,
  const float lo[3], const float hi[3], bool cold)
{
  GridDesc t;
  desc_finish(&t, base_cell, n, lo, hi);
  const bool any = n > 0 && lo[0] <= hi[0];  // (a finite point sets all six extrema)
  unsigned open = 0u;
  bool fits = !cold && any && u.cell == t.cell;
  if (any)
    for (int a = 0; a < 3; a++)
    {
      // exactly the arithmetic of cell_coord, before its clamp
      if (floor(((double) lo[a] - u.mn[a]) * u.inv_cell) < 0.0)
        open |= 1u << (2 * a);
      if (floor(((double) hi[a] - u.mn[a]) * u.inv_cell) > (double) (u.dim[a] - 1))
        open |= 2u << (2 * a);
      fits = fits && u.dim[a] - t.dim[a] <= 4 * kGridMargin;
    }
  if (open)
  {
    used->open = open;
    atomicAdd(miss, 1u);
  }
  GridDesc o = u;
  if (!fits || open)
  {
    int m = kGridMargin;
    if ((double) (t.dim[0] + 2 * m) * (double) (t.dim[1] + 2 * m) * (double) (t.dim[2] + 2 * m) > (double) kCellCap)
      m = 0;
    o = t;
    for (int a = 0; a < 3; a++)
    {
      o.mn[a] = t.mn[a] - m * t.cell;
      o.dim[a] = t.dim[a] + 2 * m;
    }
    o.ncell = o.dim[0] * o.dim[1] * o.dim[2];
  }
  o.open = 0u;
  o.ticket = 0u;
  *next = o;
}

// Exclusive scan of the cell histogram in ONE launch (decoupled look-back): tiles of kScanBlock cells are walked round-robin
// by the G = gridDim.x work-groups of a cloud (256 for one cloud, 64 per cloud of a batch), so a tile's predecessors are always
// running or done and the look-back cannot deadlock.
// Forward progress, also for the tiles of a second and later pass (more than G tiles: above 8.4 m^3 of box at the base cell
// for one cloud, above 2.1 m^3 per cloud of a batch).  A look-back only reads tiles of its OWN cloud, and tile t only waits
// for tiles < t.  (i) While all G groups of a cloud are dispatched, every tile of that cloud completes, by induction over
// t: tile 0 waits for nothing; the owner of tile t (group t mod G) reaches it after its earlier tiles t - G, t - 2G, ..., all
// < t and complete by induction, and then waits only for tiles < t.  A group of a second pass may wait for the FIRST tile of a
// higher-numbered group, which is why (i) asks for all G groups and not only the lower-numbered ones.  (ii) Groups are
// dispatched in order, x fastest, then y: when a group of cloud k is dispatched, every group of the clouds < k has been.  Take
// the lowest cloud that is not complete.  Either all its groups are dispatched, and it completes by (i), or the dispatcher
// stands inside it; then no group of a later cloud holds a slot, the earlier clouds are complete and their groups have
// left, so its remaining groups are dispatched as soon as the device has room for them.  What this needs from the device is
// room for G groups of 256 threads at once (256 groups: one per CU of an MI355X; the batch's 64 x 64 = 4096 groups are more
// than are resident at once, and need not be) and that nothing else on the device holds its slots for ever.  A tile
// publishes (build number, flag, value) in one 64-bit word: flag 1 = the tile's own total, 2 = its inclusive prefix;
// the build number makes stale words from earlier builds invisible, so the descriptors never need clearing.  The kernel
// also zeroes the histogram it has read: the next build starts from a clean one without a memset.  And its last work-group, which
// has no tile unless the grid is huge, reduces k_cell_count's extrema slots and decides the next build's descriptor (desc_next).
constexpr int kScanBlock = 4096;  // cells per tile: 16 per thread, four 16-byte accesses each way

__device__ __forceinline__ int block_scan_excl(int v, int* total)
{
  // 256 threads: wave scan + cross-wave
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan_i32(v);
  if (lane == 63)
    wsum[w] = inc;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; k++)
    base += wsum[k];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return base + inc - v;
}

__global__ __launch_bounds__(256) void k_cell_scan(int* __restrict__ count, GridDesc* __restrict__ d,
  unsigned long long* __restrict__ tile_state, unsigned gen, int* __restrict__ cell_start, const int* __restrict__ cloud_off,
  const float* __restrict__ part, int nparts, GridDesc* __restrict__ next, unsigned* __restrict__ miss, double base_cell, int cold)
{
  __shared__ int s_prefix;
  // blockIdx.y = cloud: its own histogram, tile descriptors and cell table; the table holds positions in the common
  // sorted array, i.e. it starts at the cloud's first point.  (Work-groups are dispatched x-fastest, so the predecessors a
  // tile waits for were dispatched before it, for every cloud.)
  const int p0 = cloud_off[blockIdx.y], n = cloud_off[blockIdx.y + 1] - p0;
  count += (int64_t) blockIdx.y * kCellCap;
  tile_state += (int64_t) blockIdx.y * (kCellCap / kScanBlock);
  cell_start += (int64_t) blockIdx.y * kCellStride;
  d += blockIdx.y;
  const int ncell = d->ncell;
  // 256 resident work-groups walk the tiles round-robin: tile t only ever waits for tiles < t, which belong to the
  // first pass of lower-numbered groups or to an earlier pass, so the look-back cannot deadlock (and no same-address
  // ticket atomics, ~12 ns each, are needed to order the tiles)
  for (int tile = blockIdx.x; tile * kScanBlock < ncell; tile += gridDim.x)
  {
  const int b0 = tile * kScanBlock;
  // thread t owns the cells b0 + 16 t .. + 15 (the table is padded to whole tiles, and cells past ncell hold zero counts)
  int4 v[4];
  int sum = 0;
  for (int k = 0; k < 4; k++)
  {
    v[k] = reinterpret_cast<const int4*>(count + b0)[threadIdx.x * 4 + k];
    sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  int total;
  int ex = block_scan_excl(sum, &total);
  const unsigned long long tag = (unsigned long long) gen << 34;
  if (threadIdx.x < 64)  // wave 0 publishes and looks back, 64 predecessors per round (one serial load per
  {                      // predecessor would make the last tile wait ~0.6 us x its index)
    const int lane = threadIdx.x;
    int prefix = 0;
    if (lane == 0)
      __hip_atomic_store(&tile_state[tile], tag | ((tile == 0 ? 2ull : 1ull) << 32) | (unsigned) total, __ATOMIC_RELEASE,
        __HIP_MEMORY_SCOPE_AGENT);
    for (int j0 = tile - 1; j0 >= 0; j0 -= 64)
    {
      const int j = j0 - lane;
      unsigned long long w = 0;
      for (;;)
      {
        bool ready = true;
        if (j >= 0)
        {
          w = __hip_atomic_load(&tile_state[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          ready = (w >> 34) == gen && ((w >> 32) & 3ull) != 0ull;
        }
        if (__ballot(!ready) == 0ull)
          break;
        __builtin_amdgcn_s_sleep(1);  // a predecessor has not published yet
      }
      const unsigned long long incl = __ballot(j >= 0 && ((w >> 32) & 3ull) == 2ull);
      const int stop = incl ? __ffsll((long long) incl) - 1 : 63;  // nearest predecessor with an inclusive prefix
      int val = (j >= 0 && lane <= stop) ? (int) (unsigned) w : 0;
      for (int o = 32; o > 0; o >>= 1)
        val += __shfl_xor(val, o);
      prefix += val;
      if (incl)
        break;
    }
    if (lane == 0)
    {
      if (tile != 0)
        __hip_atomic_store(&tile_state[tile], tag | (2ull << 32) | (unsigned) (prefix + total), __ATOMIC_RELEASE,
          __HIP_MEMORY_SCOPE_AGENT);
      s_prefix = prefix;
    }
  }
  __syncthreads();
  ex += s_prefix + p0;
  for (int k = 0; k < 4; k++)
  {
    int4 o;
    o.x = ex;
    o.y = o.x + v[k].x;
    o.z = o.y + v[k].y;
    o.w = o.z + v[k].z;
    ex = o.w + v[k].w;
    // (entries past ncell are scratch of the padded table; the one AT ncell is written below, after everybody's stores)
    reinterpret_cast<int4*>(cell_start + b0)[threadIdx.x * 4 + k] = o;
    reinterpret_cast<int4*>(count + b0)[threadIdx.x * 4 + k] = make_int4(0, 0, 0, 0);
  }
  if (tile == 0 && threadIdx.x == 0)
    cell_start[ncell] = p0 + n;
  __syncthreads();  // s_prefix is reused by the next tile of this group
  }
  if (blockIdx.x == gridDim.x - 1)
  {
    float lo[3], hi[3];
    reduce_parts(part + (int64_t) blockIdx.y * kCountBlocks * 6, nparts, lo, hi);
    if (threadIdx.x == 0)
      desc_next(*d, d, next + blockIdx.y, miss, base_cell, n, lo, hi, cold != 0);
  }
}

__global__ __launch_bounds__(256) void k_scatter(const float* __restrict__ xyz, int64_t stride,
  const int32_t* __restrict__ cam, const int* __restrict__ cloud_off, const int* __restrict__ cell_of,
  const int* __restrict__ rank_of, const int* __restrict__ cell_start, float4* __restrict__ sorted)
{
  const int64_t p0 = cloud_off[blockIdx.y], p1 = cloud_off[blockIdx.y + 1];
  cell_start += (int64_t) blockIdx.y * kCellStride;
  for (int64_t i = p0 + blockIdx.x * (int64_t) blockDim.x + threadIdx.x; i < p1; i += (int64_t) gridDim.x * blockDim.x)
  {
    const int pos = cell_start[cell_of[i]] + rank_of[i];
    const float* p = xyz + i * stride;
    const unsigned w = ((unsigned) i << 1) | (cam ? (unsigned) (cam[i] & 1) : 0u);
    sorted[pos] = make_float4(p[0], p[1], p[2], __uint_as_float(w));
  }
}

int grid_build(Ctx* c, hipStream_t st)
{
  // one launch per stage for the whole batch: blockIdx.y = cloud
  const int C = c->n_clouds;
  int64_t nmax = 0;
  for (int k = 0; k < C; k++)
    nmax = std::max<int64_t>(nmax, c->cloud_off[(size_t) k + 1] - c->cloud_off[(size_t) k]);
  const int nblk = (int) std::max<int64_t>(1, std::min<int64_t>((nmax + 255) / 256, kCountBlocks));
  // the kept descriptors belong to the cloud slots of the last build: a batch of another size (or a failed build) starts cold.
  // A cloud of another point count in the same slot does not: the descriptor is only geometry, and a cloud it does not fit
  // is a miss or a shrink (desc_next).
  const bool cold = !c->grid_clean || c->grid_force_cold || c->grid_key_clouds != C;
  if (!c->grid_miss_zeroed)
  {
    hipMemsetAsync(c->d_grid_miss, 0, sizeof(unsigned), st);
    c->grid_miss_zeroed = true;
  }
  if (!c->grid_clean)  // first build of the context, or the previous one failed half-way
  {
    hipMemsetAsync(c->d_cell_count, 0, sizeof(int) * (size_t) kCellCap * c->clouds_cap, st);
    hipMemsetAsync(c->d_tile_state, 0, sizeof(unsigned long long) * (size_t) (kCellCap / kScanBlock) * c->clouds_cap, st);
    hipLaunchKernelGGL(k_desc_reset, dim3(c->clouds_cap), dim3(1), 0, st, c->d_desc);
    c->build_gen = 0;
  }
  c->grid_clean = false;
  if (++c->build_gen >= (1u << 30))  // the tag has 30 bits: start over long before it wraps
  {
    hipMemsetAsync(c->d_tile_state, 0, sizeof(unsigned long long) * (size_t) (kCellCap / kScanBlock) * c->clouds_cap, st);
    c->build_gen = 1;
  }
  // host-buffer agh_set_cloud: the camera ids go up on a stream of their own beside the coordinate-only kernels below.  That
  // stream must not write own_cam while work queued EARLIER on `st` (the previous build's k_scatter, a search) still reads it:
  // with a pinned source nothing else orders the two (a pageable copy happened to, by blocking).  The gate is recorded here,
  // before this build's kernels, so the copy waits for the earlier work only.
  bool cam_gate = false;
  if (c->pending_cam_host)
  {
    if (!c->copy_stream && !c->copy_stream_failed &&
        (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
         hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming) != hipSuccess ||
         hipEventCreateWithFlags(&c->copy_gate, hipEventDisableTiming) != hipSuccess))
    {
      // whatever was created goes again, and the failure is remembered: the camera ids then go up on the build's own stream
      // for the rest of the context's life instead of retrying (and leaking) on every build
      if (c->copy_gate)
        (void) hipEventDestroy(c->copy_gate);
      if (c->copy_done)
        (void) hipEventDestroy(c->copy_done);
      if (c->copy_stream)
        (void) hipStreamDestroy(c->copy_stream);
      c->copy_gate = nullptr;
      c->copy_done = nullptr;
      c->copy_stream = nullptr;
      c->copy_stream_failed = true;
    }
    if (c->copy_stream)
      cam_gate = hipEventRecord(c->copy_gate, st) == hipSuccess && hipStreamWaitEvent(c->copy_stream, c->copy_gate, 0) == hipSuccess;
  }
  // cell >= r_hands/4 keeps a ball query within 9 x 9 rows
  const double base_cell = std::max(0.02, c->p.nn_radius_hands / 4.0);
  // (also for an empty cloud: one work-group writes the descriptor of an empty grid)
  if (cold)
  {
    const int nparts = std::max(1, std::min(nblk, kBboxBlocks));
    hipLaunchKernelGGL(k_bbox, dim3(nparts, C), dim3(kBboxThreads), 0, st, c->d_xyz, c->stride_floats,
      (const int*) c->d_cloud_off, c->d_bbox_part);
    hipLaunchKernelGGL(k_cell_count<true>, dim3(nblk, C), dim3(256), 0, st, c->d_xyz, c->stride_floats, (const int*) c->d_cloud_off,
      c->d_desc, (const GridDesc*) c->d_desc_next, c->d_cell_of, c->d_rank_of, c->d_cell_count, (const float*) c->d_bbox_part,
      nparts, base_cell, c->d_count_part);
  }
  else
    hipLaunchKernelGGL(k_cell_count<false>, dim3(nblk, C), dim3(256), 0, st, c->d_xyz, c->stride_floats, (const int*) c->d_cloud_off,
      c->d_desc, (const GridDesc*) c->d_desc_next, c->d_cell_of, c->d_rank_of, c->d_cell_count, (const float*) nullptr, 0,
      base_cell, c->d_count_part);
  hipLaunchKernelGGL(k_cell_scan, dim3(C == 1 ? 256 : 64, C), dim3(256), 0, st, c->d_cell_count, c->d_desc, c->d_tile_state,
    c->build_gen, c->d_cell_start, (const int*) c->d_cloud_off, (const float*) c->d_count_part, nblk, c->d_desc_next,
    c->d_grid_miss, base_cell, cold ? 1 : 0);
  c->grid_builds++;
  c->grid_cold_builds += cold ? 1 : 0;
  if (c->pending_cam_host)
  {
    // host-buffer agh_set_cloud: the camera ids (a blocking pageable copy, ~1.2 MB for 300k points) go up while the three
    // kernels above run -- they read coordinates only.  On a stream of its own: on `st` the transfer would queue behind those
    // kernels.  A pageable copy returns when the SOURCE has been read (into the runtime's staging buffers), not necessarily
    // when the data is on the device, so k_scatter waits for an event behind the copy; the coordinates' copy, which was
    // ordered behind everything earlier on the context's stream, has already returned when this one is issued.
    hipStream_t cs = (c->copy_stream && cam_gate) ? c->copy_stream : st;  // (no gate: in order on `st`, behind the kernels above)
    hipError_t e = hipMemcpyAsync(c->own_cam, c->pending_cam_host, sizeof(int32_t) * (size_t) c->pending_cam_n,
      hipMemcpyHostToDevice, cs);
    c->pending_cam_host = nullptr;
    c->cam_copy_on_copy_stream = cs != st;
    if (e == hipSuccess && cs != st)
    {
      e = hipEventRecord(c->copy_done, cs);
      if (e == hipSuccess)
        e = hipStreamWaitEvent(st, c->copy_done, 0);
    }
    if (e != hipSuccess)
      return AGH_ERR_HIP;
  }
  if (nmax > 0)
    hipLaunchKernelGGL(k_scatter, dim3(nblk, C), dim3(256), 0, st, c->d_xyz, c->stride_floats, c->d_cam,
      (const int*) c->d_cloud_off, c->d_cell_of, c->d_rank_of, c->d_cell_start, c->d_sorted);
  if (hipGetLastError() != hipSuccess)
    return AGH_ERR_HIP;
  c->grid_clean = true;
  c->grid_key_clouds = C;
  return AGH_OK;
}

}  // namespace agh
