// voxelize.hip -- K-1: the preprocessing in front of the search.
//
// Stands in for the head of Localization::localizeHands (reference src/agile_grasp/localization.cpp):
//   17-24    camera id of raw point i = (i >= size_left), assigned before the NaN removal and never re-indexed
//   25-27    pcl::removeNaNFromPointCloud (order preserving; a cloud flagged is_dense is passed through)
//   216-245  filterWorkspace: min <= p <= max per axis
//   247-355  voxelizeCloud: per-camera minimum, floor((p - min) / cell), std::set in lexicographic (x, y, z) order,
//            coordinates back as v * cell + min, camera 0 block then camera 1 block.
//
// The std::set is replaced by a bitmap over each camera's voxel lattice laid out x-major, z-fastest: a set bit's
// position IS its lexicographic rank order, so "insert" is an atomicOr and "iterate in order" is a popcount scan --
// no sort.  A 1.3 m x 1.0 m x 0.5 m scene at 3 mm is 24 Mbit = 3 MB per camera (L2 / Infinity-Cache resident).
// The arithmetic that defines the voxel of a point and the coordinates of a voxel is the reference's, in double,
// without contraction.
#include "agh_internal.h"

#include <utility>

namespace agh
{

constexpr int kPreBlock = 256;
constexpr int kPrePerBlock = 1024;   // points per block (4 rounds of 256)
constexpr int kWordsPerBlock = 4096; // bitmap words per block in the popcount passes (16 per thread)
constexpr int kPruneWords = 1024;    // bitmap words per work-group of k_vox_prune (4 per thread): a quarter block

// agh_localize_batch: the kernels below with a VoxBatch whose `cap` is set run one capture per blockIdx.y -- its points, its
// descriptor, its slice of the block tables and its slot of the bitmap (vb.slot_words words each); without it (cap == nullptr,
// a grid of one row) they run the single cloud of their other arguments.
__device__ __forceinline__ const VoxCapture* vox_capture(const VoxBatch& vb)
{
  return vb.cap ? vb.cap + blockIdx.y : nullptr;
}

__device__ __forceinline__ void vox_desc_init(VoxDesc* d)
{
  for (int c = 0; c < 2; c++)
    for (int a = 0; a < 3; a++)
    {
      d->mn_enc[c][a] = enc_float(10000.0f);  // the reference's initial minimum (localization.cpp:250-252)
      d->mx_enc[c][a] = 0u;
    }
  d->n_kept[0] = d->n_kept[1] = 0;
  d->n_vox[0] = d->n_vox[1] = 0;
  d->n_occupied[0] = d->n_occupied[1] = 0;
  d->n_pruned[0] = d->n_pruned[1] = 0;
  d->error = 0;
}
__global__ void k_vox_init(VoxDesc* d)
{
  vox_desc_init(d);
}

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
  return isfinite(x) && isfinite(y) && isfinite(z);
}

// Finite points per block of 1024 raw points (rank base of the NaN-free cloud).
__global__ __launch_bounds__(kPreBlock) void k_vox_count(const float* __restrict__ xyz, int64_t stride, int64_t n,
  int* __restrict__ blk_cnt, VoxBatch vb)
{
  if (const VoxCapture* q = vox_capture(vb))
  {
    if (q->dense)
      return;
    xyz = q->xyz;
    stride = q->stride;
    n = q->n;
    blk_cnt += q->blk_off;
  }
  const int64_t base = (int64_t) blockIdx.x * kPrePerBlock;
  if (base >= n)  // (a batch's launch is sized for its largest capture)
    return;
  int cnt = 0;
  for (int r = 0; r < 4; r++)
  {
    const int64_t i = base + r * kPreBlock + threadIdx.x;
    if (i < n)
    {
      const float* p = xyz + i * stride;
      cnt += finite3(p[0], p[1], p[2]) ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1)
    cnt += __shfl_down(cnt, o);
  __shared__ int s[4];
  if ((threadIdx.x & 63) == 0)
    s[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0)
    blk_cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__device__ void vox_totals(VoxDesc* d, const int* __restrict__ blk_prefix, long long total, VoxDesc* host_desc, int* cloud_off_out);

// Exclusive scan of an int array with one block (in place); total to *total if given.  Two one-thread kernels ride along
// (each was a ~5 us launch of its own: a few dependent global accesses by one thread): init_desc -- the descriptor's
// reset in front of k_vox_classify --, and totals_desc -- the voxel counts per camera and the host mirror behind the second scan.
// cloud_off_out: the context's device-side cloud offsets {0, voxel count} -- so that a grid build queued behind this kernel
// finds the count on the device, without the host having to wait for it (agh_localize).
// vb (a batch): the first scan (init_desc set) runs over the capture's raw block counts, the second (totals_desc set) over its
// bitmap slot's popcounts; descriptors and mirrors are the capture's, cloud_off_out and total are not written (k_vox_chain).
__global__ __launch_bounds__(1024) void k_vox_scan(int* __restrict__ v, int64_t nb, long long* total, VoxDesc* init_desc,
  VoxDesc* totals_desc, VoxDesc* host_desc, int* cloud_off_out, VoxBatch vb)
{
  if (const VoxCapture* q = vox_capture(vb))
  {
    const int y = blockIdx.y;
    total = nullptr;
    cloud_off_out = nullptr;
    if (init_desc)
    {
      v += q->blk_off;
      nb = q->dense ? 0 : (q->n + kPrePerBlock - 1) / kPrePerBlock;
      init_desc = vb.desc + y;
    }
    if (totals_desc)
    {
      v += (int64_t) y * (vb.slot_words / kWordsPerBlock);
      nb = q->n > 0 ? vb.slot_words / kWordsPerBlock : 0;
      totals_desc = vb.desc + y;
      host_desc = vb.host_desc ? vb.host_desc + y : nullptr;
    }
  }
  __shared__ long long carry;
  __shared__ int wsum[16];
  if (threadIdx.x == 0)
  {
    carry = 0;
    if (init_desc)
      vox_desc_init(init_desc);
  }
  __syncthreads();
  for (int64_t b0 = 0; b0 < nb; b0 += 1024)
  {
    const int64_t i = b0 + threadIdx.x;
    const int x = i < nb ? v[i] : 0;
    int incl = x;
    for (int o = 1; o < 64; o <<= 1)
    {
      const int y = __shfl_up(incl, o);
      if ((int) (threadIdx.x & 63) >= o)
        incl += y;
    }
    if ((threadIdx.x & 63) == 63)
      wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < (int) (threadIdx.x >> 6); w++)
      wbase += wsum[w];
    if (i < nb)
      v[i] = (int) (carry + wbase + incl - x);  // (ranks < 2^30 by the API's bound on n)
    __syncthreads();
    if (threadIdx.x == 1023)
      carry += wbase + incl;
    __syncthreads();
  }
  if (total && threadIdx.x == 0)
    *total = carry;
  if (totals_desc && threadIdx.x == 0)  // (v was written by this work-group: the barriers above order it)
    vox_totals(totals_desc, v, carry, host_desc, cloud_off_out);
}

// Camera id (rank in the NaN-free cloud >= size_left), workspace test, per-camera minimum and maximum.
__global__ __launch_bounds__(kPreBlock) void k_vox_classify(const float* __restrict__ xyz, int64_t stride, int64_t n,
  const int* __restrict__ blk_prefix, int64_t size_left, VoxWorkspace ws, uint8_t* __restrict__ code, VoxDesc* d, VoxBatch vb)
{
  if (const VoxCapture* q = vox_capture(vb))
  {
    xyz = q->xyz;
    stride = q->stride;
    n = q->n;
    blk_prefix = q->dense ? nullptr : blk_prefix + q->blk_off;
    size_left = q->size_left;
    ws = q->ws;
    code += q->code_off;
    d = vb.desc + blockIdx.y;
    if ((int64_t) blockIdx.x * kPrePerBlock >= n)
      return;
  }
  __shared__ int wcnt[4];
  __shared__ unsigned smn[2][3], smx[2][3];
  __shared__ int skept[2];
  if (threadIdx.x < 6)
  {
    smn[threadIdx.x / 3][threadIdx.x % 3] = 0xffffffffu;
    smx[threadIdx.x / 3][threadIdx.x % 3] = 0u;
  }
  if (threadIdx.x < 2)
    skept[threadIdx.x] = 0;
  const int64_t base = (int64_t) blockIdx.x * kPrePerBlock;
  int64_t running = blk_prefix ? (int64_t) blk_prefix[blockIdx.x] : base;  // finite points before this round
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned mn[2][3], mx[2][3];
  for (int c = 0; c < 2; c++)
    for (int a = 0; a < 3; a++)
    {
      mn[c][a] = 0xffffffffu;
      mx[c][a] = 0u;
    }
  int kept[2] = { 0, 0 };
  for (int r = 0; r < 4; r++)
  {
    const int64_t i = base + r * kPreBlock + threadIdx.x;
    float p[3] = { 0.f, 0.f, 0.f };
    bool fin = false;
    if (i < n)
    {
      const float* q = xyz + i * stride;
      p[0] = q[0];
      p[1] = q[1];
      p[2] = q[2];
      fin = blk_prefix ? finite3(p[0], p[1], p[2]) : true;
    }
    const unsigned long long m = __ballot(fin);
    __syncthreads();  // (also orders the LDS initialisation above before its first use)
    if (lane == 0)
      wcnt[wave] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++)
      before += wcnt[w];
    const int64_t rank = running + before;
    running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (i < n)
    {
      const int cam = rank >= size_left ? 1 : 0;
      const bool in = fin && (double) p[0] >= ws.lo[0] && (double) p[0] <= ws.hi[0] && (double) p[1] >= ws.lo[1] &&
                      (double) p[1] <= ws.hi[1] && (double) p[2] >= ws.lo[2] && (double) p[2] <= ws.hi[2];
      code[i] = in ? (uint8_t) (1 | (cam << 1)) : (uint8_t) 0;
      if (in)
      {
        kept[cam]++;
        for (int a = 0; a < 3; a++)
        {
          const unsigned e = enc_float(p[a]);
          mn[cam][a] = min(mn[cam][a], e);
          mx[cam][a] = max(mx[cam][a], e);
        }
      }
    }
  }
  for (int c = 0; c < 2; c++)
  {
    for (int a = 0; a < 3; a++)
    {
      unsigned lo = mn[c][a], hi = mx[c][a];
      for (int o = 32; o > 0; o >>= 1)
      {
        lo = min(lo, (unsigned) __shfl_down(lo, o));
        hi = max(hi, (unsigned) __shfl_down(hi, o));
      }
      if (lane == 0)
      {
        atomicMin(&smn[c][a], lo);
        atomicMax(&smx[c][a], hi);
      }
    }
    int k = kept[c];
    for (int o = 32; o > 0; o >>= 1)
      k += __shfl_down(k, o);
    if (lane == 0 && k)
      atomicAdd(&skept[c], k);
  }
  __syncthreads();
  if (threadIdx.x < 6)  // one global atomic pair per block, camera and axis
  {
    const int c = threadIdx.x / 3, a = threadIdx.x % 3;
    if (skept[c] > 0)
    {
      atomicMin(&d->mn_enc[c][a], smn[c][a]);
      atomicMax(&d->mx_enc[c][a], smx[c][a]);
    }
  }
  if (threadIdx.x < 2 && skept[threadIdx.x] > 0)
    atomicAdd((unsigned long long*) &d->n_kept[threadIdx.x], (unsigned long long) skept[threadIdx.x]);
}

// (vox_index, the voxel index along one axis, exactly as localization.cpp:288: agh_internal.h)

// error: 1 = the lattice exceeds max_words (the hard limit), 2 = it exceeds cap_words, the bitmap the host has allocated from an
// earlier cloud (stage 2 was launched speculatively for that size and does nothing; the host enlarges and repeats).
__device__ void vox_lattice(VoxDesc* d, double cell, unsigned long long max_words, unsigned long long cap_words, VoxDesc* host_desc)
{
  unsigned long long ofs = 0;
  for (int c = 0; c < 2; c++)
  {
    unsigned long long bits = 0;
    for (int a = 0; a < 3; a++)
    {
      d->mn[c][a] = (double) dec_float(d->mn_enc[c][a]);
      d->dim[c][a] = 0;
    }
    if (d->n_kept[c] > 0)
    {
      bits = 1;
      for (int a = 0; a < 3; a++)
      {
        const long long top = vox_index(dec_float(d->mx_enc[c][a]), d->mn[c][a], cell);
        if (top < 0 || top >= (1ll << 31) - 1)
        {
          d->error = 1;
          bits = 0;
          break;
        }
        d->dim[c][a] = (int) top + 1;
        // (the product is checked against max_words step by step so that it cannot wrap)
        if (bits > (max_words * 32ull) / (unsigned long long) d->dim[c][a])
        {
          d->error = 1;
          bits = 0;
          break;
        }
        bits *= (unsigned long long) d->dim[c][a];
      }
    }
    d->bits[c] = bits;
    d->word_ofs[c] = ofs;
    unsigned long long words = (bits + 31ull) / 32ull;
    words = (words + kWordsPerBlock - 1ull) / kWordsPerBlock * kWordsPerBlock;  // camera 1 starts on a block boundary
    ofs += words;
  }
  d->n_words = ofs;
  if (ofs > max_words)
    d->error = 1;
  else if (!d->error && ofs > cap_words)
    d->error = 2;
  if (host_desc)
    *host_desc = *d;
}
__global__ void k_vox_lattice(VoxDesc* d, double cell, unsigned long long max_words, unsigned long long cap_words, VoxDesc* host_desc,
  VoxBatch vb)
{
  if (vb.cap)
  {
    d = vb.desc + blockIdx.y;
    host_desc = vb.host_desc ? vb.host_desc + blockIdx.y : nullptr;
  }
  vox_lattice(d, cell, max_words, cap_words, host_desc);
}
// The speculative pass (agh_preprocess_device from the second cloud on): the bitmap of the size the context already has is
// cleared by all work-groups while one thread computes the lattice -- one launch for what were a runtime fill kernel and a
// one-thread kernel, ~5 us each.  (k_vox_mark, the next kernel, is the first reader of both.)
__global__ __launch_bounds__(256) void k_vox_clear_lattice(uint4* __restrict__ bitmap16, int64_t n16, VoxDesc* d, double cell,
  unsigned long long max_words, unsigned long long cap_words, VoxDesc* host_desc, VoxBatch vb)
{
  if (vb.cap)
  {
    bitmap16 += (int64_t) blockIdx.y * (vb.slot_words / 4);
    d = vb.desc + blockIdx.y;
    host_desc = vb.host_desc ? vb.host_desc + blockIdx.y : nullptr;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    vox_lattice(d, cell, max_words, cap_words, host_desc);
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t) gridDim.x * 256)
    bitmap16[i] = z;
}

__global__ __launch_bounds__(256) void k_vox_mark(const float* __restrict__ xyz, int64_t stride, int64_t n,
  const uint8_t* __restrict__ code, const VoxDesc* __restrict__ d, double cell, unsigned* __restrict__ bitmap, VoxBatch vb)
{
  if (const VoxCapture* q = vox_capture(vb))
  {
    xyz = q->xyz;
    stride = q->stride;
    n = q->n;
    code += q->code_off;
    d = vb.desc + blockIdx.y;
    bitmap += (int64_t) blockIdx.y * vb.slot_words;
  }
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const unsigned cd = code[i];
  if (!cd || d->error)
    return;
  const int c = (int) (cd >> 1);
  const unsigned long long pos = vox_bit(d, c, xyz + i * stride, cell);  // (agh_internal.h: k_mask_mark sets the same bit)
  atomicOr(&bitmap[d->word_ofs[c] + (pos >> 5)], 1u << (unsigned) (pos & 31ull));
}

__global__ __launch_bounds__(256) void k_vox_popcount(const unsigned* __restrict__ bitmap, int* __restrict__ blk_cnt, VoxBatch vb)
{
  if (vb.cap)
  {
    bitmap += (int64_t) blockIdx.y * vb.slot_words;
    blk_cnt += (int64_t) blockIdx.y * (vb.slot_words / kWordsPerBlock);
  }
  const uint4* w = (const uint4*) (bitmap + (size_t) blockIdx.x * kWordsPerBlock) + threadIdx.x * 4;
  int cnt = 0;
  for (int k = 0; k < 4; k++)
  {
    const uint4 v = w[k];
    cnt += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  for (int o = 32; o > 0; o >>= 1)
    cnt += __shfl_down(cnt, o);
  __shared__ int s[4];
  if ((threadIdx.x & 63) == 0)
    s[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0)
    blk_cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__device__ void vox_totals(VoxDesc* d, const int* __restrict__ blk_prefix, long long total_v, VoxDesc* host_desc, int* cloud_off_out)
{
  const long long* total = &total_v;
  if (d->error)
  {
    d->n_vox[0] = d->n_vox[1] = 0;
    if (host_desc)
      *host_desc = *d;
    if (cloud_off_out)
      cloud_off_out[0] = cloud_off_out[1] = 0;
    return;
  }
  const long long first1 = d->word_ofs[1] / kWordsPerBlock < d->n_words / kWordsPerBlock
                             ? (long long) blk_prefix[d->word_ofs[1] / kWordsPerBlock]
                             : *total;
  d->n_vox[0] = first1;
  d->n_vox[1] = *total - first1;
  if (host_desc)
    *host_desc = *d;
  if (cloud_off_out)
  {
    cloud_off_out[0] = 0;
    cloud_off_out[1] = (int) *total;
  }
}

// a / b and a % b for a below 2^33 by way of b's double reciprocal: the quotient estimate is off by at most one and is corrected
// (k_vox_emit says why not three 64-bit integer divisions per voxel)
__device__ __forceinline__ void vox_divmod(unsigned long long a, unsigned long long b, double inv_b, unsigned long long& q,
  unsigned long long& r)
{
  q = (unsigned long long) ((double) a * inv_b);
  long long rr = (long long) a - (long long) (q * b);
  if (rr < 0)
  {
    q--;
    rr += (long long) b;
  }
  else if (rr >= (long long) b)
  {
    q++;
    rr -= (long long) b;
  }
  r = (unsigned long long) rr;
}

// agh_set_voxel_filter (include/agh.h; DESIGN.md, "Voxel filter"): the marked bitmap `src` without the voxels that have fewer than
// min_neighbors other set voxels of their own camera's lattice within the integer ball of `radius`, into `dst`.  Out of place: the
// support is counted on what k_vox_mark set, never on this kernel's output.  It works as k_vox_emit does, on a QUARTER of a
// 4096-word block per work-group (kPruneWords, a word quad per thread: a 3 mm capture's lattice is under 200 blocks, fewer than the
// CUs, and a voxel's count is a chain of dependent loads that only other work-groups hide): the quarter's set bits are listed in
// LDS and dealt to the lanes, a copy of its words in LDS loses the pruned bits, and EVERY word is written -- dst is never cleared,
// and the blocks beyond the lattice (all zero in src) come out zero.
// For a fixed (dx, dy) the ball is one z-run of 2 h + 1 <= 9 adjacent bits, h = floor(sqrt(r^2 - dx^2 - dy^2)): clipped
// to the row [0, nz) and to the lattice BEFORE its bit address is formed (the bits beside a row's end are another row's), read
// from at most two adjacent words.  A clipped run lies inside the camera's lattice, so inside the slot.
template <int R>
__global__ __launch_bounds__(256) void k_vox_prune(const unsigned* __restrict__ src, unsigned* __restrict__ dst, VoxDesc* d,
  int min_neighbors, VoxBatch vb)
{
  if (vb.cap)
  {
    src += (int64_t) blockIdx.y * vb.slot_words;
    dst += (int64_t) blockIdx.y * vb.slot_words;
    d = vb.desc + blockIdx.y;
  }
  constexpr int kListCap = 4096;
  __shared__ unsigned list[kListCap];
  __shared__ unsigned out[kPruneWords];
  __shared__ int wsum[4];
  __shared__ int s_pruned;
  const size_t wg0 = (size_t) blockIdx.x * kPruneWords;
  const size_t w0 = wg0 + (size_t) threadIdx.x * 4;
  uint4* dst16 = reinterpret_cast<uint4*>(dst + w0);
  const uint4 v = *reinterpret_cast<const uint4*>(src + w0);
  const unsigned w[4] = { v.x, v.y, v.z, v.w };
  const int cnt = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  int incl = cnt;
  for (int o = 1; o < 64; o <<= 1)
  {
    const int y = __shfl_up(incl, o);
    if ((int) (threadIdx.x & 63) >= o)
      incl += y;
  }
  if ((threadIdx.x & 63) == 63)
    wsum[threadIdx.x >> 6] = incl;
  if (threadIdx.x == 0)
    s_pruned = 0;
  __syncthreads();
  int loff = incl - cnt;
  for (int q = 0; q < (int) (threadIdx.x >> 6); q++)
    loff += wsum[q];
  const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (!total || d->error)  // (uniform: an empty block, or a lattice that does not fit -- nothing downstream reads bits then)
  {
    *dst16 = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  for (int j = 0; j < 4; j++)
    out[threadIdx.x * 4 + j] = w[j];
  const int c = wg0 >= d->word_ofs[1] ? 1 : 0;  // (camera 1 starts on a 4096-word boundary: a work-group is of one camera)
  const long long nx = d->dim[c][0], ny = d->dim[c][1], nz = d->dim[c][2];
  const double inv_nz = 1.0 / (double) nz, inv_ny = 1.0 / (double) ny;
  const unsigned* lat = src + d->word_ofs[c];  // the camera's lattice, bit 0
  const unsigned long long pos0 = ((unsigned long long) wg0 - d->word_ofs[c]) * 32ull;
  auto test = [&](unsigned rel_bit) {  // rel_bit: bit position inside the work-group's words
    unsigned long long t, uz, ux, uy;
    vox_divmod(pos0 + rel_bit, (unsigned long long) nz, inv_nz, t, uz);
    vox_divmod(t, (unsigned long long) ny, inv_ny, ux, uy);
    const long long ix = (long long) ux, iy = (long long) uy, iz = (long long) uz;
    int support = -1;  // (the run of dx = dy = 0 counts the voxel itself)
    // The planes in the order dx = 0, -1, 1, -2, 2, ...: a surface voxel reaches min_neighbors in the first one or two.  Both loops
    // are unrolled (R is the template's), so a plane's runs -- up to 2 R + 1 pairs of loads -- are in flight together; the loop
    // leaves between planes as soon as the count is reached.
#pragma unroll
    for (int i = 0; i <= 2 * R; i++)
    {
      const int dx = (i & 1) ? -((i + 1) / 2) : i / 2;
      const long long x = ix + dx;
      if (x < 0 || x >= nx)
        continue;
      int plane = 0;
#pragma unroll
      for (int dy = -R; dy <= R; dy++)
      {
        const int rem = R * R - dx * dx - dy * dy;
        const long long y = iy + dy;
        if (rem < 0 || y < 0 || y >= ny)
          continue;
        const int h = rem >= 16 ? 4 : rem >= 9 ? 3 : rem >= 4 ? 2 : rem >= 1 ? 1 : 0;
        const long long z0 = max(iz - h, 0ll), z1 = min(iz + h, nz - 1);
        const int len = (int) (z1 - z0) + 1;
        const unsigned long long b0 = (unsigned long long) ((x * ny + y) * nz + z0);
        const unsigned long long word = b0 >> 5;
        const unsigned sh = (unsigned) (b0 & 31ull);
        unsigned run = lat[word] >> sh;
        if (sh + (unsigned) len > 32u)  // (then sh > 0; the run's last bit is the lattice's: the next word is the camera's)
          run |= lat[word + 1] << (32u - sh);
        plane += __popc(run & ((1u << len) - 1u));
      }
      support += plane;
      if (support >= min_neighbors)
        break;
    }
    if (support < min_neighbors)
    {
      atomicAnd(&out[rel_bit >> 5], ~(1u << (rel_bit & 31u)));
      atomicAdd(&s_pruned, 1);
    }
  };
  if (total <= kListCap)
  {
    int q = loff;
    for (int j = 0; j < 4; j++)
    {
      unsigned bits = w[j];
      while (bits)
      {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        list[q++] = (unsigned) (threadIdx.x * 4 + j) * 32u + (unsigned) b;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += 256)
      test(list[i]);
  }
  else  // (a dense block: every thread walks its own words)
  {
    __syncthreads();
    for (int j = 0; j < 4; j++)
    {
      unsigned bits = w[j];
      while (bits)
      {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        test((unsigned) (threadIdx.x * 4 + j) * 32u + (unsigned) b);
      }
    }
  }
  __syncthreads();
  *dst16 = *reinterpret_cast<const uint4*>(out + threadIdx.x * 4);
  if (threadIdx.x == 0)  // one integer atomic per work-group and counter: order free
  {
    atomicAdd((unsigned long long*) &d->n_occupied[c], (unsigned long long) total);
    if (s_pruned)
      atomicAdd((unsigned long long*) &d->n_pruned[c], (unsigned long long) s_pruned);
  }
}

// (one instantiation per radius the setter admits)
static void vox_prune(dim3 grid, hipStream_t st, const unsigned* src, unsigned* dst, VoxDesc* d, const agh_voxel_filter_params& fp,
  const VoxBatch& vb)
{
  const int k = (int) fp.min_neighbors;
  grid.x *= kWordsPerBlock / kPruneWords;  // (grid: the 4096-word blocks, as for k_vox_popcount)
  switch (fp.radius)
  {
    case 1: hipLaunchKernelGGL(k_vox_prune<1>, grid, dim3(256), 0, st, src, dst, d, k, vb); break;
    case 2: hipLaunchKernelGGL(k_vox_prune<2>, grid, dim3(256), 0, st, src, dst, d, k, vb); break;
    case 3: hipLaunchKernelGGL(k_vox_prune<3>, grid, dim3(256), 0, st, src, dst, d, k, vb); break;
    default: hipLaunchKernelGGL(k_vox_prune<4>, grid, dim3(256), 0, st, src, dst, d, k, vb); break;
  }
}

// Emit the voxels in bitmap order = (camera, x, y, z) lexicographic order; coordinates as localization.cpp:313-324.
// vb (a batch): capture y's voxels go to the common array from cloud_off[y] on (k_vox_chain).
__global__ __launch_bounds__(256) void k_vox_emit(const unsigned* __restrict__ bitmap, const int* __restrict__ blk_prefix,
  const VoxDesc* __restrict__ d, double cell, float* __restrict__ out_xyz, int32_t* __restrict__ out_cam, VoxBatch vb,
  const int* __restrict__ cloud_off)
{
  int64_t out0 = 0;
  if (vb.cap)
  {
    bitmap += (int64_t) blockIdx.y * vb.slot_words;
    blk_prefix += (int64_t) blockIdx.y * (vb.slot_words / kWordsPerBlock);
    d = vb.desc + blockIdx.y;
    out0 = cloud_off[blockIdx.y];
  }
  const size_t w0 = (size_t) blockIdx.x * kWordsPerBlock + (size_t) threadIdx.x * 16;
  unsigned w[16];
  const uint4* src = (const uint4*) (bitmap + w0);
  int cnt = 0;
  for (int k = 0; k < 4; k++)
  {
    const uint4 v = src[k];
    w[4 * k] = v.x;
    w[4 * k + 1] = v.y;
    w[4 * k + 2] = v.z;
    w[4 * k + 3] = v.w;
    cnt += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  int incl = cnt;
  for (int o = 1; o < 64; o <<= 1)
  {
    const int y = __shfl_up(incl, o);
    if ((int) (threadIdx.x & 63) >= o)
      incl += y;
  }
  __shared__ int wsum[4];
  if ((threadIdx.x & 63) == 63)
    wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  int loff = incl - cnt;  // this thread's first voxel among the work-group's
  for (int q = 0; q < (int) (threadIdx.x >> 6); q++)
    loff += wsum[q];
  const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (!total || d->error)
    return;
  const int64_t k0 = out0 + (int64_t) blk_prefix[blockIdx.x];
  const size_t wg0 = (size_t) blockIdx.x * kWordsPerBlock;
  const int c = wg0 >= d->word_ofs[1] ? 1 : 0;  // (camera 1 starts on a block boundary: a work-group is of one camera)
  const unsigned long long ny = (unsigned long long) d->dim[c][1], nz = (unsigned long long) d->dim[c][2];
  const double m0 = d->mn[c][0], m1 = d->mn[c][1], m2 = d->mn[c][2];
  // (ix, iy, iz) of a bit position: two exact integer divisions by way of double reciprocals (positions are below 2^33, the
  // quotient estimate is off by at most one and is corrected) -- three 64-bit integer divisions per VOXEL, ~100 instructions
  // each on this part, made the kernel 52 us for 250k voxels
  const double inv_nz = 1.0 / (double) nz, inv_ny = 1.0 / (double) ny;
  auto emit = [&](unsigned rel_bit, int64_t k) {  // rel_bit: bit position inside the work-group's 4096 words
    const unsigned long long pos = ((unsigned long long) wg0 - d->word_ofs[c]) * 32ull + rel_bit;
    unsigned long long t, uz, ux, uy;
    vox_divmod(pos, nz, inv_nz, t, uz);
    vox_divmod(t, ny, inv_ny, ux, uy);
    const long long iz = (long long) uz, iy = (long long) uy, ix = (long long) ux;
    out_xyz[3 * k] = (float) ((double) ix * cell + 1.0 * m0);
    out_xyz[3 * k + 1] = (float) ((double) iy * cell + 1.0 * m1);
    out_xyz[3 * k + 2] = (float) ((double) iz * cell + 1.0 * m2);
    out_cam[k] = c;
  };
  // The lattice is sparse (about one bit in a hundred is set) and the set bits sit unevenly in the threads' words: a thread that
  // walked its own bits and stored its own voxels kept a wave waiting for its fullest lane and scattered 12-byte stores over the
  // output (47 us for 250k voxels).  The work-group's set bits are LISTED in LDS first, in bitmap order, and then emitted a
  // voxel per thread: every lane busy, consecutive lanes write consecutive voxels.
  constexpr int kListCap = 4096;
  __shared__ unsigned list[kListCap];
  if (total <= kListCap)
  {
    int q = loff;
    for (int j = 0; j < 16; j++)
    {
      unsigned bits = w[j];
      while (bits)
      {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        list[q++] = (unsigned) (threadIdx.x * 16 + j) * 32u + (unsigned) b;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += 256)
      emit(list[i], k0 + i);
    return;
  }
  // (a dense block -- more than a set bit per word on average: every thread walks its own words)
  int64_t k = k0 + loff;
  for (int j = 0; j < 16; j++)
  {
    unsigned bits = w[j];
    while (bits)
    {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      emit((unsigned) (threadIdx.x * 16 + j) * 32u + (unsigned) b, k);
      k++;
    }
  }
}

// agh_localize_batch: the batch's device-side cloud offsets from the captures' voxel counts (capture k = cloud k)
__global__ void k_vox_chain(const VoxDesc* __restrict__ d, int C, int* __restrict__ cloud_off)
{
  int off = 0;
  cloud_off[0] = 0;
  for (int k = 0; k < C; k++)
  {
    off += (int) (d[k].n_vox[0] + d[k].n_vox[1]);
    cloud_off[k + 1] = off;
  }
}

int vox_stage1(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, int64_t size_left, int dense,
  const double workspace[6], double cell, hipStream_t st, int64_t cap_words, VoxDesc* host_desc, bool with_lattice)
{
  VoxWorkspace ws;
  for (int a = 0; a < 3; a++)
  {
    ws.lo[a] = workspace[2 * a];
    ws.hi[a] = workspace[2 * a + 1];
  }
  const int64_t nb = (n + kPrePerBlock - 1) / kPrePerBlock;
  const bool scan_first = n > 0 && !dense;  // (then the descriptor's reset rides on that one-block scan)
  if (!scan_first)
    hipLaunchKernelGGL(k_vox_init, dim3(1), dim3(1), 0, st, c->d_vox_desc);
  if (n > 0)
  {
    if (!dense)
    {
      hipLaunchKernelGGL(k_vox_count, dim3((unsigned) nb), dim3(kPreBlock), 0, st, d_xyz, stride_floats, n, c->d_vox_blk, VoxBatch{});
      hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(1024), 0, st, c->d_vox_blk, nb, (long long*) nullptr, c->d_vox_desc,
        (VoxDesc*) nullptr, (VoxDesc*) nullptr, (int*) nullptr, VoxBatch{});
    }
    hipLaunchKernelGGL(k_vox_classify, dim3((unsigned) nb), dim3(kPreBlock), 0, st, d_xyz, stride_floats, n,
      dense ? (const int*) nullptr : (const int*) c->d_vox_blk, size_left, ws, c->d_vox_code, c->d_vox_desc, VoxBatch{});
  }
  if (with_lattice)  // (the speculative pass computes the lattice inside stage 2's first kernel)
    hipLaunchKernelGGL(k_vox_lattice, dim3(1), dim3(1), 0, st, c->d_vox_desc, cell, (unsigned long long) kVoxMaxWords,
      (unsigned long long) cap_words, host_desc, VoxBatch{});
  return hipGetLastError() == hipSuccess ? AGH_OK : AGH_ERR_HIP;
}

// n_words: the lattice's size, or any multiple of kWordsPerBlock above it that the bitmap has room for (the blocks beyond the
// lattice hold no bits and emit nothing)
int vox_stage2(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, double cell, int64_t n_words, hipStream_t st,
  VoxDesc* host_desc, bool with_lattice, int* cloud_off_out)
{
  const int64_t cap_words = n_words;
  c->vox_filter_captures = 0;
  if (c->voxel_filter_set)
  {
    // the second bitmap, of the first one's capacity (+ its slack): made on first use, regrown with the first
    if (!c->d_vox_pruned || c->vox_pruned_cap != cap_words)
    {
      c->vox_pruned_cap = 0;
      if (int rc = dev_alloc(c, &c->d_vox_pruned, (size_t) cap_words + 4096))
        return rc;
      c->vox_pruned_cap = cap_words;
    }
    c->vox_filter_captures = 1;
    c->vox_filter_mirror = host_desc;
  }
  if (n == 0)
    n_words = 0;  // (no point, no bit: nothing to clear, count or emit; the block counts are not even written)
  const int64_t nb2 = n_words / kWordsPerBlock;
  if (with_lattice)  // speculative pass: clear + lattice in one launch (n_words is a multiple of 4096 words)
    hipLaunchKernelGGL(k_vox_clear_lattice, dim3((unsigned) std::max<int64_t>(1, std::min<int64_t>(n_words / 4 / 256, 2048))), dim3(256), 0,
      st, reinterpret_cast<uint4*>(c->d_vox_bitmap), n_words / 4, c->d_vox_desc, cell, (unsigned long long) kVoxMaxWords,
      (unsigned long long) cap_words, host_desc, VoxBatch{});
  else if (hipMemsetAsync(c->d_vox_bitmap, 0, (size_t) n_words * 4, st) != hipSuccess)
    return AGH_ERR_HIP;
  if (n > 0 && n_words > 0)
  {
    hipLaunchKernelGGL(k_vox_mark, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, d_xyz, stride_floats, n,
      (const uint8_t*) c->d_vox_code, (const VoxDesc*) c->d_vox_desc, cell, c->d_vox_bitmap, VoxBatch{});
    if (c->voxel_filter_set)
    {
      // marked -> pruned, out of place; from here on "the" bitmap of the context is the pruned one (the next cloud clears and
      // marks it, and prunes into the other: both have the same capacity)
      vox_prune(dim3((unsigned) nb2), st, c->d_vox_bitmap, c->d_vox_pruned, c->d_vox_desc, c->voxel_filter, VoxBatch{});
      std::swap(c->d_vox_bitmap, c->d_vox_pruned);
    }
    hipLaunchKernelGGL(k_vox_popcount, dim3((unsigned) nb2), dim3(256), 0, st, (const unsigned*) c->d_vox_bitmap,
      c->d_vox_blk2, VoxBatch{});
  }
  hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(1024), 0, st, c->d_vox_blk2, nb2, c->d_vox_total, (VoxDesc*) nullptr, c->d_vox_desc,
    host_desc, cloud_off_out, VoxBatch{});  // (+ the voxel counts per camera, the host mirror, the device-side cloud offsets)
  if (n > 0 && n_words > 0)
    hipLaunchKernelGGL(k_vox_emit, dim3((unsigned) nb2), dim3(256), 0, st, (const unsigned*) c->d_vox_bitmap,
      (const int*) c->d_vox_blk2, (const VoxDesc*) c->d_vox_desc, cell, c->d_vox_xyz, c->d_vox_cam, VoxBatch{}, (const int*) nullptr);
  return hipGetLastError() == hipSuccess ? AGH_OK : AGH_ERR_HIP;
}

int vox_count_blocks(const unsigned* d_bitmap, int64_t n_blocks, int* d_blk, long long* d_total, hipStream_t st)
{
  if (n_blocks > 0)
    hipLaunchKernelGGL(k_vox_popcount, dim3((unsigned) n_blocks), dim3(256), 0, st, d_bitmap, d_blk, VoxBatch{});
  hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(1024), 0, st, d_blk, n_blocks, d_total, (VoxDesc*) nullptr, (VoxDesc*) nullptr,
    (VoxDesc*) nullptr, (int*) nullptr, VoxBatch{});
  return hipGetLastError() == hipSuccess ? AGH_OK : AGH_ERR_HIP;
}

int vox_count_blocks_batch(const VoxBatch& vb, int C, const unsigned* d_bitmap, int* d_blk, hipStream_t st)
{
  if (vb.slot_words > 0)
    hipLaunchKernelGGL(k_vox_popcount, dim3((unsigned) (vb.slot_words / kWordsPerBlock), (unsigned) C), dim3(256), 0, st, d_bitmap,
      d_blk, vb);
  return hipGetLastError() == hipSuccess ? AGH_OK : AGH_ERR_HIP;
}

// agh_localize_batch: the preprocessing of C captures, one launch per stage, capture = blockIdx.y (see VoxBatch).  Stage 1 (finite
// counts, their scan with the descriptors' reset, camera ids, workspace, extrema); with probe, the lattices next (the caller waits
// for them and sizes the slots); otherwise the speculative stage 2 on slots of vb.slot_words words: clear + lattice, mark,
// popcount, scan + counts, the batch's cloud offsets into cloud_off, emit into out_xyz / out_cam.  blk: the raw block counts,
// blk2: C x slot_words / kWordsPerBlock popcounts; nb_max, n_max: the largest capture's raw blocks and points.  filter
// (agh_set_voxel_filter; nullptr: none): k_vox_prune behind the mark, from bitmap into `pruned`, slots of the same layout, which
// everything after it reads -- the caller swaps its two pointers once this is queued.
int vox_batch(const VoxBatch& vb, int C, int64_t nb_max, int64_t n_max, bool any_finite_scan, double cell, bool probe,
  unsigned* bitmap, int* blk, int* blk2, uint8_t* code, float* out_xyz, int32_t* out_cam, int* cloud_off, hipStream_t st,
  unsigned* pruned, const agh_voxel_filter_params* filter)
{
  const unsigned Cy = (unsigned) C;
  if (nb_max > 0 && any_finite_scan)
    hipLaunchKernelGGL(k_vox_count, dim3((unsigned) nb_max, Cy), dim3(kPreBlock), 0, st, (const float*) nullptr, (int64_t) 0,
      (int64_t) 0, blk, vb);
  hipLaunchKernelGGL(k_vox_scan, dim3(1, Cy), dim3(1024), 0, st, blk, (int64_t) 0, (long long*) nullptr, vb.desc, (VoxDesc*) nullptr,
    (VoxDesc*) nullptr, (int*) nullptr, vb);
  if (nb_max > 0)
    hipLaunchKernelGGL(k_vox_classify, dim3((unsigned) nb_max, Cy), dim3(kPreBlock), 0, st, (const float*) nullptr, (int64_t) 0,
      (int64_t) 0, (const int*) blk, (int64_t) 0, VoxWorkspace{}, code, vb.desc, vb);
  if (probe)
  {
    hipLaunchKernelGGL(k_vox_lattice, dim3(1, Cy), dim3(1), 0, st, vb.desc, cell, (unsigned long long) kVoxMaxWords,
      (unsigned long long) kVoxMaxWords, vb.host_desc, vb);
    return hipGetLastError() == hipSuccess ? AGH_OK : AGH_ERR_HIP;
  }
  const int64_t W = vb.slot_words, nb2 = W / kWordsPerBlock;
  hipLaunchKernelGGL(k_vox_clear_lattice, dim3((unsigned) std::max<int64_t>(1, std::min<int64_t>(W / 4 / 256, 2048)), Cy), dim3(256), 0,
    st, reinterpret_cast<uint4*>(bitmap), W / 4, vb.desc, cell, (unsigned long long) kVoxMaxWords, (unsigned long long) W,
    vb.host_desc, vb);
  if (n_max > 0)
    hipLaunchKernelGGL(k_vox_mark, dim3((unsigned) ((n_max + 255) / 256), Cy), dim3(256), 0, st, (const float*) nullptr, (int64_t) 0,
      (int64_t) 0, (const uint8_t*) code, (const VoxDesc*) vb.desc, cell, bitmap, vb);
  if (filter)  // (every slot, also with n_max == 0: the pruned slots are never cleared)
  {
    vox_prune(dim3((unsigned) nb2, Cy), st, bitmap, pruned, vb.desc, *filter, vb);
    bitmap = pruned;
  }
  hipLaunchKernelGGL(k_vox_popcount, dim3((unsigned) nb2, Cy), dim3(256), 0, st, (const unsigned*) bitmap, blk2, vb);
  hipLaunchKernelGGL(k_vox_scan, dim3(1, Cy), dim3(1024), 0, st, blk2, (int64_t) 0, (long long*) nullptr, (VoxDesc*) nullptr,
    vb.desc, vb.host_desc, (int*) nullptr, vb);
  hipLaunchKernelGGL(k_vox_chain, dim3(1), dim3(1), 0, st, (const VoxDesc*) vb.desc, C, cloud_off);
  hipLaunchKernelGGL(k_vox_emit, dim3((unsigned) nb2, Cy), dim3(256), 0, st, (const unsigned*) bitmap, (const int*) blk2,
    (const VoxDesc*) vb.desc, cell, out_xyz, out_cam, vb, (const int*) cloud_off);
  return hipGetLastError() == hipSuccess ? AGH_OK : AGH_ERR_HIP;
}

}  // namespace agh

using namespace agh;

extern "C" {

// ---- the voxel filter's setting (include/agh.h): host-side, the two ints travel as k_vox_prune's arguments ----
void agh_default_voxel_filter_params(agh_voxel_filter_params* p)
{
  if (!p)
    return;
  p->radius = 2;
  p->min_neighbors = 4;
}

int agh_set_voxel_filter(agh_ctx* ctx, const agh_voxel_filter_params* fp)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_set_voxel_filter"))
    return AGH_ERR_STATE;
  if (!fp)
  {
    c->voxel_filter_set = false;
    return AGH_OK;
  }
  auto bad = [c](const char* what) {
    c->err = std::string("agh_set_voxel_filter: ") + what;
    return AGH_ERR_INVALID_ARGUMENT;
  };
  if (fp->radius < 1 || fp->radius > 4)
    return bad("radius must be 1 .. 4");
  static const int ball[5] = { 1, 7, 33, 123, 257 };  // positions of the integer ball, its centre among them
  if (fp->min_neighbors < 1 || fp->min_neighbors > ball[fp->radius] - 1)
    return bad("min_neighbors must be 1 .. B(radius) - 1 (B = 7, 33, 123, 257)");
  c->voxel_filter = *fp;
  c->voxel_filter_set = true;
  return AGH_OK;
}

int agh_get_voxel_filter(agh_ctx* ctx, agh_voxel_filter_params* out)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;  // (host-side: allowed while a localize chain is in flight)
  if (!c->voxel_filter_set)
    return 0;
  if (!out)
  {
    c->err = "agh_get_voxel_filter: out is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  *out = c->voxel_filter;
  return 1;
}

int agh_get_voxel_filter_counts(agh_ctx* ctx, agh_voxel_filter_counts* out, int32_t cap_captures)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_voxel_filter_counts"))
    return AGH_ERR_STATE;
  if (c->vox_filter_captures == 0)
    return 0;
  if (cap_captures < c->vox_filter_captures || !out)
  {
    c->err = "agh_get_voxel_filter_counts: room for " + std::to_string(c->vox_filter_captures) + " captures is needed";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  AGH_HIPCHK(c, hipStreamSynchronize(c->stream));  // (the mirrors are written by the voxeliser's second scan)
  for (int k = 0; k < c->vox_filter_captures; k++)
  {
    const VoxDesc& h = c->vox_filter_mirror[k];
    for (int cam = 0; cam < 2; cam++)
    {
      out[k].n_occupied[cam] = (int64_t) h.n_occupied[cam];
      out[k].n_pruned[cam] = (int64_t) h.n_pruned[cam];
      out[k].n_kept[cam] = (int64_t) h.n_vox[cam];
    }
  }
  return c->vox_filter_captures;
}

}  // extern "C"
