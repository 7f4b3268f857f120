// sample_cluster.hip -- the object sets of a clustered chain (include/agh.h, agh_localize_clustered*; DESIGN.md, "Clusters as the
// label source").
//
// A labelled chain gets objset[voxel], one bit per object, from a label image (sample_labels.hip, k_label_mark).  Here the same
// array comes from the cloud itself: the caller names the support plane, the voxels that stand above it are FOREGROUND, two
// foreground voxels within `tolerance` of each other are adjacent, and the objects are the largest connected components.
//   k_cluster_init      height per voxel; parent[v] = v (foreground) or -1 (background); size[v] = 0; the foreground count
//   k_cluster_link      the hot kernel: by group of grid cells, the candidates of the cells around it staged through LDS, every
//                       adjacent pair united in a lock-free union-find whose parents are voxel indices
//   k_cluster_flatten   parent[v] = its root; the roots' sizes and their number by integer atomics
//   k_cluster_select    one work-group: the roots of size >= min_voxels, the K largest of them by (size, smaller id), their rank
//                       into size[root] (as -1 - rank), ids, sizes and counts into the pinned table
//   k_cluster_mark      objset[v] = 1 << rank of v's root (or 0), and the label byte of agh_get_cluster_labels
// A fitted chain (agh_localize_clustered_fit*, plane_fit.hip) finds the plane on the device: k_cluster_init_dev and
// k_cluster_link_dev read the ClusterDev record from device memory, where k_fit_finish left it, around the same bodies.
// From there the label stage's compaction runs unchanged (label_compact_stage).  Everything is queued on the chain's stream behind
// the grid build; launches are sized from the raw point count, the voxel count and the grid's descriptor are read on the device.
//
// The batch forms (include/agh.h, agh_localize_batch_clustered*; DESIGN.md, "Clusters in the batch chains") run the same five steps
// once for all captures, capture = blockIdx.y (blockIdx.x for the selection): k_cluster_init_batch, k_cluster_link_batch,
// k_cluster_flatten_batch, k_cluster_select_batch, k_cluster_mark_batch around the SAME bodies (cluster_init_voxel ...
// cluster_mark_voxel below).  parent / size / label lie over the COMMON voxel array, capture k's voxels at cloud_off[k]; the
// union-find's indices are the ones the cell-sorted array carries, positions in that common array, so capture k's roots are its
// smallest COMMON indices, which are its smallest capture-local ones too (ids are reported less cloud_off[k]).  Capture k walks
// its own grid descriptor and cell table and unites only what ITS cells hold: no pair is formed across captures.  From there the
// labelled batch's compaction runs unchanged (label_compact_stage_batch).
//
// Nothing depends on the order of an atomic operation: the union-find hooks the LARGER root under the smaller one, so a finished
// component's root is its smallest voxel index whatever the order; sizes and counts are integer sums; the selection's keys are
// distinct.
#include "agh_internal.h"

#include <algorithm>

namespace agh
{

constexpr int kClusterGroupX = 2;   // grid cells, along x, whose voxels one work-group pass owns
constexpr int kClusterTile = 256;   // candidates staged per pass = threads of k_cluster_link
constexpr int kClusterReach = 3;    // most cells a ball of `tolerance` reaches: tolerance <= 0.05 (refused beyond), cell >= 0.02
constexpr int kClusterRows = (2 * kClusterReach + 1) * (2 * kClusterReach + 1);

// min_height < h < max_height, h = ((a x + b y) + c z) + d in double on the float coordinates, left to right (the build does
// not contract); a non-finite h compares false
__device__ __forceinline__ bool cluster_foreground(const ClusterDev& cp, float x, float y, float z)
{
  const double h = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(cp.plane[0], (double) x), __dmul_rn(cp.plane[1], (double) y)),
                               __dmul_rn(cp.plane[2], (double) z)), cp.plane[3]);
  return h > cp.min_height && h < cp.max_height;
}

// ---- the union-find.  Invariant: parent[x] <= x for every foreground voxel, with equality exactly at a root; a word only ever
// decreases (atomicMin, or a compare-and-swap that replaces a root's own index by a smaller one).  Every access inside
// k_cluster_link is an agent-scope atomic: a value read late is an older one, and whatever parent[x] ever held stays an ancestor
// of x (a hook gives a ROOT a parent, halving replaces a parent by a grandparent), so a stale read costs steps, never a result. ----
__device__ __forceinline__ int cluster_load(int* p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x, halving the path on the way.  The loop ends: x is replaced by its grandparent gp <= p < x while x is no
// root, so x strictly decreases and is bounded by 0.
__device__ __forceinline__ int cluster_find(int* parent, int x)
{
  for (;;)
  {
    const int p = cluster_load(parent + x);
    if (p == x || p < 0)  // (p < 0: a background voxel, which no caller passes)
      return x;
    const int gp = cluster_load(parent + p);
    if (gp != p)
      atomicMin(parent + x, gp);
    x = gp;
  }
}

// a and b into one component: the larger of their roots is hooked under the smaller, by a compare-and-swap on the larger root's
// own word.  The loop ends: a failed swap means another thread hooked that root meanwhile, so the next find from it returns a
// strictly smaller root, and the other side's root never grows -- the larger of the two roots strictly decreases with every
// repeat, at most `a` times.
__device__ __forceinline__ void cluster_unite(int* parent, int a, int b)
{
  for (;;)
  {
    a = cluster_find(parent, a);
    b = cluster_find(parent, b);
    if (a == b)
      return;
    if (a < b)
    {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(parent + a, a, b) == a)
      return;
  }
}

// counts: [0] foreground voxels, [1] components (zeroed in front of the launch).  The cloud's nv voxels start at `base` of the
// voxel array (0 for a single cloud, cloud_off[k] in a batch): the index a voxel is known by is base + its local one.
__device__ __forceinline__ void cluster_init_voxel(const float* __restrict__ xyz, int64_t stride, int64_t base, int64_t nv,
  const ClusterDev& cp, int* __restrict__ parent, int* __restrict__ size, unsigned long long* __restrict__ counts)
{
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  bool fg = false;
  if (v < nv)
  {
    const float* p = xyz + (base + v) * stride;
    fg = cluster_foreground(cp, p[0], p[1], p[2]);
    parent[base + v] = fg ? (int) (base + v) : -1;
    size[base + v] = 0;
  }
  const unsigned long long m = __ballot(fg);
  if ((threadIdx.x & 63) == 0 && m)
    atomicAdd(counts, (unsigned long long) __popcll(m));
}

// (the single cloud's form, wherever its record lies)
__device__ __forceinline__ void cluster_init_single(const float* __restrict__ xyz, int64_t stride, const VoxDesc* __restrict__ d,
  int64_t n, const ClusterDev& cp, int* __restrict__ parent, int* __restrict__ size, unsigned long long* __restrict__ counts)
{
  cluster_init_voxel(xyz, stride, 0, label_voxels(d, n), cp, parent, size, counts);
}

__global__ __launch_bounds__(256) void k_cluster_init(const float* __restrict__ xyz, int64_t stride, const VoxDesc* __restrict__ d,
  int64_t n, ClusterDev cp, int* __restrict__ parent, int* __restrict__ size, unsigned long long* __restrict__ counts)
{
  cluster_init_single(xyz, stride, d, n, cp, parent, size, counts);
}

// ... with the record read from device memory: a fitted chain's, which k_fit_finish (plane_fit.hip) wrote in front of this launch
__global__ __launch_bounds__(256) void k_cluster_init_dev(const float* __restrict__ xyz, int64_t stride, const VoxDesc* __restrict__ d,
  int64_t n, const ClusterDev* __restrict__ cpd, int* __restrict__ parent, int* __restrict__ size, unsigned long long* __restrict__ counts)
{
  const ClusterDev cp = *cpd;
  cluster_init_single(xyz, stride, d, n, cp, parent, size, counts);
}

// ... for capture blockIdx.y of a batch, with ITS record of the device table and its four counters (no voxel for a capture whose
// descriptor carries an error: label_voxels)
__global__ __launch_bounds__(256) void k_cluster_init_batch(VoxBatch vb, const float* __restrict__ xyz, int64_t stride,
  const int* __restrict__ cloud_off, const ClusterDev* __restrict__ cps, int* __restrict__ parent, int* __restrict__ size,
  unsigned long long* __restrict__ counts)
{
  const int k = blockIdx.y;
  const ClusterDev cp = cps[k];
  cluster_init_voxel(xyz, stride, cloud_off[k], label_voxels(vb.desc + k, vb.cap[k].n), cp, parent, size, counts + 4 * k);
}

// Work goes out by GROUP of kClusterGroupX cells along x of one (y, z) row of the search grid: the group's voxels are one run
// of the cell-sorted array (the owners, a thread each), and they share their candidates -- the cells within `reach` cells of the
// group in every direction, one run of the sorted array per (y, z) row around it.  reach comes from the descriptor's OWN cell size
// (it may have doubled): two voxels within `tolerance` lie at most reach cells apart along every axis.  A voxel outside the
// descriptor's box sits clamped in a border cell (GridDesc::open); clamping moves cell coordinates no further apart, so cell
// offsets -- where a geometric ball would have to reach outwards through an open face -- find such pairs too.
// The candidates pass through LDS a tile at a time, background ones already marked, and every owner tests the whole tile with the
// float32 rule; a pair is united once, from the side with the larger voxel index.
// (gv: the view of ONE cloud's grid -- its descriptor, its cell table; the whole work-group comes here, and the work-groups
// along x share the cloud's cell groups)
__device__ __forceinline__ void cluster_link_groups(const GridView& gv, const ClusterDev& cp, int* parent)
{
  __shared__ float4 cand[kClusterTile];
  __shared__ int row_begin[kClusterRows];
  __shared__ int row_prefix[64 + 1];
  const GridDesc g = *gv.desc;
  const int tid = threadIdx.x;
  // (the margin covers the rounding of the float32 rule: a pair may pass it a few ulp beyond `tolerance`)
  const int reach = min((int) floor(cp.tolerance * g.inv_cell * 1.0001) + 1, kClusterReach);
  const int side = 2 * reach + 1, nrows = side * side;
  const int gx = (g.dim[0] + kClusterGroupX - 1) / kClusterGroupX;
  const long long n_groups = (long long) gx * g.dim[1] * g.dim[2];
  for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x)  // (uniform over the work-group, as every branch around a barrier below)
  {
    const int row = (int) (grp / gx), x0 = (int) (grp - (long long) row * gx) * kClusterGroupX;
    const int x1 = min(x0 + kClusterGroupX, g.dim[0]);
    const int cz = row / g.dim[1], cy = row - cz * g.dim[1];
    const int o0 = gv.cell_start[row * g.dim[0] + x0], o1 = gv.cell_start[row * g.dim[0] + x1];
    if (o1 <= o0)
      continue;
    // the candidate runs, one per (y, z) row around the group, and their exclusive scan (wave 0)
    __syncthreads();  // (the previous group's table and tile are done with)
    if (tid < 64)
    {
      int len = 0;
      if (tid < nrows)
      {
        const int qz = tid / side, yy = cy + (tid - qz * side) - reach, zz = cz + qz - reach;
        int b = 0;
        if (yy >= 0 && yy < g.dim[1] && zz >= 0 && zz < g.dim[2])
        {
          const int base = (zz * g.dim[1] + yy) * g.dim[0];
          b = gv.cell_start[base + max(x0 - reach, 0)];
          len = gv.cell_start[base + min(x1 + reach, g.dim[0])] - b;
        }
        row_begin[tid] = b;
      }
      const int incl = wave_incl_scan_i32(len);
      row_prefix[tid + 1] = incl;
      if (tid == 0)
        row_prefix[0] = 0;
    }
    __syncthreads();
    const int total = row_prefix[nrows];
    for (int ot = o0; ot < o1; ot += kClusterTile)
    {
      int v = -1;
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ot + tid < o1)
      {
        p = gv.sorted[ot + tid];
        if (cluster_foreground(cp, p.x, p.y, p.z))
          v = (int) (__float_as_uint(p.w) >> 1);
      }
      int root = v;  // an ancestor of v (v itself to begin with), kept as close to its root as this thread knows
      if (!__syncthreads_or(v >= 0))  // (no foreground owner: nothing to link)
        continue;
      for (int ct = 0; ct < total; ct += kClusterTile)
      {
        const int q = ct + tid;
        float4 c4 = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        if (q < total)
        {
          int r = 0;
          while (row_prefix[r + 1] <= q)  // (q < total = row_prefix[nrows]: r stops below nrows)
            r++;
          c4 = gv.sorted[row_begin[r] + (q - row_prefix[r])];
          const int u = (int) (__float_as_uint(c4.w) >> 1);
          c4.w = __int_as_float(cluster_foreground(cp, c4.x, c4.y, c4.z) ? u : -1);
        }
        cand[tid] = c4;
        __syncthreads();
        // Two passes per 64 candidates.  First the float32 rule alone, the hits as bits: no memory operation, every lane reads
        // the same LDS word.  Then every lane walks ITS hits -- the lanes of a wave issue their parent loads together, so a wave
        // waits once per hit of its busiest lane, not once per candidate that any lane hits.  Most hits join what is joined
        // already: one load, parent[u] == root, tells (root: an ancestor of v, as u's parent then is of u); the rest go
        // through the union-find.  (A lane without a foreground owner, v = -1, has no hit: u < v fails.)
        const int cnt = min(kClusterTile, total - ct);
        for (int s0 = 0; s0 < cnt; s0 += 64)
        {
          const int c64 = min(64, cnt - s0);
          unsigned long long hit = 0ull;
          for (int k = 0; k < c64; k++)
          {
            const float4 c = cand[s0 + k];
            const int u = __float_as_int(c.w);
            const float dx = c.x - p.x, dy = c.y - p.y, dz = c.z - p.z;
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            if (u >= 0 && u < v && d2 <= cp.tol2)
              hit |= 1ull << k;
          }
          while (hit)  // (ends: a bit less with every pass)
          {
            const int k = __ffsll((long long) hit) - 1;
            hit &= hit - 1ull;
            const int u = __float_as_int(cand[s0 + k].w);
            if (cluster_load(parent + u) != root)
            {
              cluster_unite(parent, v, u);
              root = cluster_find(parent, v);
            }
          }
        }
        __syncthreads();
      }
    }
  }
}

// (the single cloud's form, wherever its record lies)
__device__ __forceinline__ void cluster_link_single(const GridView& gv, const VoxDesc* __restrict__ d, const ClusterDev& cp, int* parent)
{
  if (d->error)
    return;
  cluster_link_groups(gv, cp, parent);
}

__global__ __launch_bounds__(kClusterTile) void k_cluster_link(GridView gv, const VoxDesc* __restrict__ d, ClusterDev cp, int* parent)
{
  cluster_link_single(gv, d, cp, parent);
}

// ... with the record read from device memory (a fitted chain's, as k_cluster_init_dev)
__global__ __launch_bounds__(kClusterTile) void k_cluster_link_dev(GridView gv, const VoxDesc* __restrict__ d,
  const ClusterDev* __restrict__ cpd, int* parent)
{
  const ClusterDev cp = *cpd;
  cluster_link_single(gv, d, cp, parent);
}

// ... for capture blockIdx.y of a batch: the cell groups of ITS descriptor and cell table, shared among the gridDim.x work-groups
// of its row of the launch.  The voxel indices in the cell-sorted array are positions in the common voxel array, and so are the
// parents: the invariant parent[x] <= x, a word only ever decreases, the larger root under the smaller, reads the same, and a
// finished component's root is its smallest common index.  Its candidates come from its own cell table, whose runs lie inside the
// capture's span of the sorted array: no pair reaches into another capture, whatever the coordinates.
__global__ __launch_bounds__(kClusterTile) void k_cluster_link_batch(GridView gv, VoxBatch vb, const ClusterDev* __restrict__ cps,
  int* parent)
{
  const int k = blockIdx.y;
  if (vb.desc[k].error)
    return;
  const ClusterDev cp = cps[k];
  cluster_link_groups(grid_of_cloud(gv, k), cp, parent);
}

// parent[v] = the root of v (the links are all made: the kernel before this one has ended), the roots' sizes and their number.
// The lanes of a wave that share a root -- most of them do -- add to its counter once.
// (the cloud's nv voxels at `base` of the voxel array, as cluster_init_voxel)
__device__ __forceinline__ void cluster_flatten_voxel(int64_t base, int64_t nv, int* parent, int* size,
  unsigned long long* __restrict__ counts)
{
  const int64_t v = base + (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  int r = -1;
  if (v < base + nv && cluster_load(parent + v) >= 0)
  {
    r = cluster_find(parent, (int) v);
    atomicMin(parent + v, r);
  }
  const unsigned long long roots = __ballot(r >= 0 && r == (int) v);
  if ((threadIdx.x & 63) == 0 && roots)
    atomicAdd(counts + 1, (unsigned long long) __popcll(roots));
  // (the loop ends: every pass retires the lanes of one root, the first pending lane's among them)
  unsigned long long pending = __ballot(r >= 0);
  while (pending)
  {
    const int lead = __ffsll((long long) pending) - 1;
    const int r0 = __shfl(r, lead);
    const unsigned long long same = __ballot(r == r0) & pending;
    if ((int) (threadIdx.x & 63) == lead)
      atomicAdd(size + r0, __popcll(same));
    pending &= ~same;
  }
}

__global__ __launch_bounds__(256) void k_cluster_flatten(const VoxDesc* __restrict__ d, int64_t n, int* parent, int* size,
  unsigned long long* __restrict__ counts)
{
  cluster_flatten_voxel(0, label_voxels(d, n), parent, size, counts);
}

__global__ __launch_bounds__(256) void k_cluster_flatten_batch(VoxBatch vb, const int* __restrict__ cloud_off, int* parent, int* size,
  unsigned long long* __restrict__ counts)
{
  const int k = blockIdx.y;
  cluster_flatten_voxel(cloud_off[k], label_voxels(vb.desc + k, vb.cap[k].n), parent, size, counts + 4 * k);
}

// One work-group.  list (n entries of scratch): the roots of size >= min_voxels, in any order; then at most K passes, pass j
// taking the largest key (size << 32) | (0xFFFFFFFF - id) below pass j - 1's -- the keys are distinct, so nothing is marked and
// the outcome does not depend on the list's order.  table (pinned): [0] foreground, [1] components, [2] objects = min(qualifying,
// K), [3] qualifying; [8 + j] M_j; [8 + 64 + j] id_j (-1: none).
constexpr int kClusterTableSizes = 8, kClusterTableIds = 8 + kMaxClouds, kClusterTableWords = 8 + 2 * kMaxClouds;
// (the body: one cloud's nv voxels at `base`; list holds LOCAL indices, at most nv of them; info: 4 words; sizes, ids: n_out
// entries each, the ids local)
__device__ __forceinline__ void cluster_select_roots(int64_t base, int64_t nv, int min_voxels, int K, const int* __restrict__ parent,
  int* size, int32_t* __restrict__ list, const unsigned long long* __restrict__ counts, long long* __restrict__ info,
  long long* __restrict__ sizes, long long* __restrict__ ids, int n_out)
{
  __shared__ int n_list;
  __shared__ unsigned long long best;
  __shared__ unsigned long long picked[kMaxClouds];
  const int tid = threadIdx.x;
  if (tid == 0)
    n_list = 0;
  __syncthreads();
  for (int64_t v = tid; v < nv; v += 1024)
    if (parent[base + v] == (int) (base + v) && size[base + v] >= min_voxels)
      list[atomicAdd(&n_list, 1)] = (int32_t) v;  // (at most nv <= n entries)
  __syncthreads();
  const int L = n_list;
  unsigned long long prev = ~0ull;
  int n_obj = 0;
  for (int j = 0; j < K && j < L; j++)  // (uniform)
  {
    if (tid == 0)
      best = 0ull;
    __syncthreads();
    unsigned long long mine = 0ull;
    for (int i = tid; i < L; i += 1024)
    {
      const int r = list[i];
      const unsigned long long key =
        ((unsigned long long) (unsigned) size[base + r] << 32) | (unsigned long long) (0xFFFFFFFFu - (unsigned) r);
      if (key < prev && key > mine)
        mine = key;
    }
    if (mine)
      atomicMax(&best, mine);
    __syncthreads();
    prev = best;  // (j < L: a key below prev is left, sizes being >= 1)
    if (tid == 0)
      picked[j] = prev;
    n_obj = j + 1;
    __syncthreads();
  }
  // (the passes have read the sizes: now the picked roots' words become their ranks)
  if (tid < n_out)
  {
    long long m = 0, id = -1;
    if (tid < n_obj)
    {
      m = (long long) (picked[tid] >> 32);
      id = (long long) (0xFFFFFFFFu - (unsigned) (picked[tid] & 0xFFFFFFFFull));
      size[base + id] = -1 - tid;
    }
    sizes[tid] = m;
    ids[tid] = id;
  }
  if (tid == 0)
  {
    info[0] = (long long) counts[0];
    info[1] = (long long) counts[1];
    info[2] = n_obj;
    info[3] = L;
  }
}

__global__ __launch_bounds__(1024) void k_cluster_select(const VoxDesc* __restrict__ d, int64_t n, int min_voxels, int K,
  const int* __restrict__ parent, int* size, int32_t* __restrict__ list, const unsigned long long* __restrict__ counts,
  long long* __restrict__ table)
{
  cluster_select_roots(0, label_voxels(d, n), min_voxels, K, parent, size, list, counts, table, table + kClusterTableSizes,
    table + kClusterTableIds, kMaxClouds);
}

// One work-group PER CAPTURE, capture blockIdx.x.  Its scratch list is its own region [code_off, code_off + n) of the list buffer
// (code_off = raw_off[k]: the capture's first raw point; free until the compaction's emit), at most K_k picks, and the batch's
// pinned table: [4 k .. 4 k + 3] capture k's counts as the single table's [0 .. 3]; [4 x 64 + l] M_l and [5 x 64 + l] id_l, the
// capture-local smallest voxel index, for its lists l = first_list[k] + j, j < K_k.
constexpr int kClusterBatchSizes = 4 * kMaxClouds, kClusterBatchIds = 5 * kMaxClouds, kClusterBatchWords = 6 * kMaxClouds;
__global__ __launch_bounds__(1024) void k_cluster_select_batch(VoxBatch vb, const int* __restrict__ cloud_off,
  const ClusterDev* __restrict__ cps, const LabelCapture* __restrict__ lc, const int* __restrict__ parent, int* size,
  int32_t* __restrict__ list, const unsigned long long* __restrict__ counts, long long* __restrict__ table)
{
  const int k = blockIdx.x;
  const VoxCapture* q = vb.cap + k;
  const int first = lc[k].first_list;
  cluster_select_roots(cloud_off[k], label_voxels(vb.desc + k, q->n), cps[k].min_voxels, lc[k].K, parent, size, list + q->code_off,
    counts + 4 * k, table + 4 * k, table + kClusterBatchSizes + first, table + kClusterBatchIds + first, lc[k].K);
}

// (the cloud's nv voxels at `base` of the voxel array: objset and label are indexed as parent is)
__device__ __forceinline__ void cluster_mark_voxel(int64_t base, int64_t nv, const int* __restrict__ parent,
  const int* __restrict__ size, unsigned long long* __restrict__ objset, uint8_t* __restrict__ label)
{
  const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv)
    return;
  const int r = parent[base + v];
  const int s = r >= 0 ? size[r] : 0;
  const int j = s < 0 ? -1 - s : -1;
  objset[base + v] = j >= 0 ? 1ull << j : 0ull;
  label[base + v] = (uint8_t) (j + 1);
}

__global__ __launch_bounds__(256) void k_cluster_mark(const VoxDesc* __restrict__ d, int64_t n, const int* __restrict__ parent,
  const int* __restrict__ size, unsigned long long* __restrict__ objset, uint8_t* __restrict__ label)
{
  cluster_mark_voxel(0, label_voxels(d, n), parent, size, objset, label);
}

// ... for capture blockIdx.y of a batch: objset[cloud_off[k] + v] = 1 << rank, bit j the capture-local object, where the labelled
// batch's compaction reads it
__global__ __launch_bounds__(256) void k_cluster_mark_batch(VoxBatch vb, const int* __restrict__ cloud_off,
  const int* __restrict__ parent, const int* __restrict__ size, unsigned long long* __restrict__ objset, uint8_t* __restrict__ label)
{
  const int k = blockIdx.y;
  cluster_mark_voxel(cloud_off[k], label_voxels(vb.desc + k, vb.cap[k].n), parent, size, objset, label);
}

// two ints and a byte per raw point, the counters and the pinned table: made by the first clustered call, grown with n.  The
// counters (four per capture) and the table (4 words per capture, 2 per list) are sized for a batch of kMaxClouds captures and
// lists at once: 2 KiB and 3 KiB, which the single chain shares.
static_assert(kClusterBatchWords >= kClusterTableWords, "one pinned table serves the single chain and the batch");
static int ensure_cluster_buffers(Ctx* c, int64_t n)
{
  int rc;
  if (!c->d_cluster_counts)
  {
    if ((rc = dev_alloc(c, &c->d_cluster_counts, (size_t) 4 * kMaxClouds)))
      return rc;
    if (hipHostMalloc((void**) &c->h_cluster_table, sizeof(long long) * kClusterBatchWords, hipHostMallocDefault) != hipSuccess)
    {
      c->h_cluster_table = nullptr;
      c->err = "hipHostMalloc failed (cluster table)";
      return AGH_ERR_HIP;
    }
  }
  if (n > c->cluster_cap || !c->d_cluster_parent)
  {
    c->cluster_cap = 0;
    const size_t room = (size_t) std::max<int64_t>(n, 1024);
    if ((rc = dev_alloc(c, &c->d_cluster_parent, room)) || (rc = dev_alloc(c, &c->d_cluster_size, room)) ||
        (rc = dev_alloc(c, &c->d_cluster_label, room)))
      return rc;
    c->cluster_cap = (int64_t) room;
  }
  return AGH_OK;
}

// (d_cp: a fitted chain's record in device memory -- k_cluster_init_dev and k_cluster_link_dev read it in place of cp, same
// shapes; the selection takes min_voxels from the host's cp either way)
int sample_cluster_stage(Ctx* c, int64_t n, const ClusterDev& cp, int K, int64_t S, unsigned long long seed, int32_t* d_out,
  int32_t* h_out, hipStream_t st, const ClusterDev* d_cp)
{
  int rc;
  const int64_t n_groups = (n + kLabelGroup - 1) / kLabelGroup;
  if ((rc = ensure_label_buffers(c, c->vox_bitmap_cap, n, (int64_t) K * n_groups)) != AGH_OK ||
      (rc = ensure_cluster_buffers(c, n)) != AGH_OK)
    return rc;
  const VoxDesc* desc = (const VoxDesc*) c->d_vox_desc;
  AGH_HIPCHK(c, hipMemsetAsync(c->d_cluster_counts, 0, sizeof(unsigned long long) * 4, st));
  if (n > 0)
  {
    const unsigned blocks = (unsigned) ((n + 255) / 256);
    // (the voxelised cloud is the context's bound cloud: the preprocessing queued in front of this stage bound it)
    if (d_cp)
      hipLaunchKernelGGL(k_cluster_init_dev, dim3(blocks), dim3(256), 0, st, c->d_xyz, c->stride_floats, desc, n, d_cp,
        c->d_cluster_parent, c->d_cluster_size, c->d_cluster_counts);
    else
      hipLaunchKernelGGL(k_cluster_init, dim3(blocks), dim3(256), 0, st, c->d_xyz, c->stride_floats, desc, n, cp, c->d_cluster_parent,
        c->d_cluster_size, c->d_cluster_counts);
    const GridView gv{ c->d_desc, c->d_cell_start, c->d_sorted, c->d_cloud_off, 1 };
    // (a work-group per 64 raw points, at most 4096: each walks its share of the grid's cell groups)
    if (d_cp)
      hipLaunchKernelGGL(k_cluster_link_dev, dim3((unsigned) std::min<int64_t>((n + 63) / 64, 4096)), dim3(kClusterTile), 0, st, gv,
        desc, d_cp, c->d_cluster_parent);
    else
      hipLaunchKernelGGL(k_cluster_link, dim3((unsigned) std::min<int64_t>((n + 63) / 64, 4096)), dim3(kClusterTile), 0, st, gv, desc,
        cp, c->d_cluster_parent);
    hipLaunchKernelGGL(k_cluster_flatten, dim3(blocks), dim3(256), 0, st, desc, n, c->d_cluster_parent, c->d_cluster_size,
      c->d_cluster_counts);
  }
  // (the lists' buffer is free until the compaction's emit: the selection borrows it)
  hipLaunchKernelGGL(k_cluster_select, dim3(1), dim3(1024), 0, st, desc, n, (int) cp.min_voxels, K, (const int*) c->d_cluster_parent,
    c->d_cluster_size, c->d_mask_list, (const unsigned long long*) c->d_cluster_counts, c->h_cluster_table);
  if (n > 0)
    hipLaunchKernelGGL(k_cluster_mark, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, desc, n, (const int*) c->d_cluster_parent,
      (const int*) c->d_cluster_size, c->d_label_set, c->d_cluster_label);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "sample cluster launch failed";
    return AGH_ERR_HIP;
  }
  return label_compact_stage(c, n, K, n > 0, S, seed, d_out, h_out, st);
}

// The stage over a batch (BatchLabelStage, agh_internal.h; its labels, codes and bitmaps are not read): one launch per step, the
// capture on blockIdx.y (blockIdx.x for the selection), none that depends on n_captures or L.  cps: the device table of the
// captures' records.  The launches are sized from n_max; k_cluster_link_batch takes min(ceil(n_max / 64), max(256, 32768 / C))
// work-groups per capture, at most 32 768 in all (C <= 64): the single form gives one capture up to 4096, and a capture's busy
// cell groups should not queue behind one another in a batch either -- with 4096 in all, eight captures of the bench scene
// took 1676 us in this kernel, with 4096 each 1305 us (profiles/NOTES.md).  Work-groups beyond a capture's groups leave at once.
int sample_cluster_stage_batch(Ctx* c, const BatchLabelStage& m, const ClusterDev* cps, hipStream_t st)
{
  int rc;
  const int64_t n_groups = (m.n_max + kLabelGroup - 1) / kLabelGroup;
  // (no label bytes, so no word ranks: the rank buffer keeps whatever size it has)
  if ((rc = ensure_label_buffers(c, 0, m.n_tot, (int64_t) m.L * n_groups)) != AGH_OK ||
      (rc = ensure_cluster_buffers(c, m.n_tot)) != AGH_OK)
    return rc;
  const unsigned Cy = (unsigned) m.C;
  AGH_HIPCHK(c, hipMemsetAsync(c->d_cluster_counts, 0, sizeof(unsigned long long) * 4 * (size_t) m.C, st));
  const unsigned blocks = (unsigned) ((m.n_max + 255) / 256);
  if (m.n_max > 0)
  {
    // (the voxelised batch is the context's bound batch: the preprocessing queued in front of this stage bound it)
    hipLaunchKernelGGL(k_cluster_init_batch, dim3(blocks, Cy), dim3(256), 0, st, m.vb, (const float*) c->d_xyz, c->stride_floats,
      m.cloud_off, cps, c->d_cluster_parent, c->d_cluster_size, c->d_cluster_counts);
    const GridView gv{ c->d_desc, c->d_cell_start, c->d_sorted, c->d_cloud_off, m.C };
    const int64_t per_capture = std::min<int64_t>((m.n_max + 63) / 64, std::max(256, 32768 / m.C));
    hipLaunchKernelGGL(k_cluster_link_batch, dim3((unsigned) per_capture, Cy), dim3(kClusterTile), 0, st, gv, m.vb, cps,
      c->d_cluster_parent);
    hipLaunchKernelGGL(k_cluster_flatten_batch, dim3(blocks, Cy), dim3(256), 0, st, m.vb, m.cloud_off, c->d_cluster_parent,
      c->d_cluster_size, c->d_cluster_counts);
  }
  // (the lists' buffer is free until the compaction's emit: every capture's selection borrows its own region of it)
  hipLaunchKernelGGL(k_cluster_select_batch, dim3(Cy), dim3(1024), 0, st, m.vb, m.cloud_off, cps, m.lists,
    (const int*) c->d_cluster_parent, c->d_cluster_size, c->d_mask_list, (const unsigned long long*) c->d_cluster_counts,
    c->h_cluster_table);
  if (m.n_max > 0)
    hipLaunchKernelGGL(k_cluster_mark_batch, dim3(blocks, Cy), dim3(256), 0, st, m.vb, m.cloud_off, (const int*) c->d_cluster_parent,
      (const int*) c->d_cluster_size, c->d_label_set, c->d_cluster_label);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "sample cluster launch failed";
    return AGH_ERR_HIP;
  }
  return label_compact_stage_batch(c, m, m.n_max > 0, st);
}

}  // namespace agh
