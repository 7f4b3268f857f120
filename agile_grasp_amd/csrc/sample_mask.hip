// sample_mask.hip -- the sample list of a masked chain (include/agh.h, agh_localize_masked*; DESIGN.md, "Sample masks").
//
// The whole cloud stays in the search; only WHERE the samples are drawn is restricted: to the voxels that hold at least one kept
// raw point with a non-zero mask byte.  The voxeliser (voxelize.hip) has left on the device what that takes: the per-raw-point
// code[] (kept flag, camera id), the descriptor of the two lattices, the voxel bitmap and the exclusive scan of its 4096-word
// blocks.  A second bitmap of the same layout takes the masked kept points (k_mask_mark); a bit set there is set in the voxel
// bitmap too, and its rank among the voxel bits IS its index in the voxelised cloud (k_mask_emit); the list of those indices, E,
// is ascending by construction, and the samples are draw_stratum's strata over it (k_draw_samples_masked).  Everything is queued
// on the chain's stream behind the voxeliser: no synchronisation is added.
#include "agh_internal.h"

#include <algorithm>

namespace agh
{

constexpr int kMaskWordsPerBlock = 4096;  // voxelize.hip's kWordsPerBlock: 16 words per thread of 256

// Raw point i with mask[i] != 0 and code[i] != 0 sets the bit k_vox_mark set for it (vox_bit), in the eligibility bitmap.
// vox (agh_set_voxel_filter; nullptr without a filter, when every such bit is set in the voxel bitmap): the pruned voxel bitmap --
// a point whose own voxel was taken out marks nothing, or its bit would count as the next surviving voxel's.
// A thread takes the four mask bytes of one ALIGNED 32-bit word: with the base `a` bytes into a word, word w holds the points
// 4 w - a .. 4 w - a + 3; the words that straddle either end of the mask are read a byte at a time.
__global__ __launch_bounds__(256) void k_mask_mark(const float* __restrict__ xyz, int64_t stride, int64_t n,
  const uint8_t* __restrict__ code, const uint8_t* __restrict__ mask, const VoxDesc* __restrict__ d, double cell,
  unsigned* __restrict__ elig, const unsigned* __restrict__ vox)
{
  const int64_t a = (int64_t) (reinterpret_cast<uintptr_t>(mask) & 3u);
  const int64_t i0 = 4 * ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) - a;
  if (i0 >= n || d->error)
    return;
  unsigned m = 0;
  if (i0 >= 0 && i0 + 3 < n)
    m = *reinterpret_cast<const unsigned*>(mask + i0);
  else
    for (int b = 0; b < 4; b++)
      if (i0 + b >= 0 && i0 + b < n)
        m |= (unsigned) mask[i0 + b] << (8 * b);
  if (!m)
    return;
  for (int b = 0; b < 4; b++)
  {
    if (!((m >> (8 * b)) & 0xffu))
      continue;
    const int64_t i = i0 + b;
    const unsigned cd = code[i];
    if (!cd)
      continue;
    const int c = (int) (cd >> 1);
    const unsigned long long pos = vox_bit(d, c, xyz + i * stride, cell);
    const unsigned long long w = d->word_ofs[c] + (pos >> 5);
    const unsigned bit = 1u << (unsigned) (pos & 31ull);
    if (vox && !(vox[w] & bit))  // (agh_set_voxel_filter: the point's voxel was pruned)
      continue;
    atomicOr(&elig[w], bit);
  }
}

// One work-group per block of 4096 words, a thread holding its 16 words of BOTH bitmaps.  An eligible bit's voxel index is the
// block's voxel prefix + the voxel bits before it in the block (camera 1 starts on a block boundary: its offset is in the
// prefix); it goes to E at the block's eligible prefix + the eligible bits before it in the block.
__global__ __launch_bounds__(256) void k_mask_emit(const unsigned* __restrict__ vox, const unsigned* __restrict__ elig,
  const int* __restrict__ vox_prefix, const int* __restrict__ elig_prefix, const VoxDesc* __restrict__ d, int32_t* __restrict__ E)
{
  const size_t w0 = (size_t) blockIdx.x * kMaskWordsPerBlock + (size_t) threadIdx.x * 16;
  unsigned v[16], e[16];
  const uint4* vs = reinterpret_cast<const uint4*>(vox + w0);
  const uint4* es = reinterpret_cast<const uint4*>(elig + w0);
  int vcnt = 0, ecnt = 0;
  for (int k = 0; k < 4; k++)
  {
    const uint4 x = vs[k], y = es[k];
    v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
    e[4 * k] = y.x, e[4 * k + 1] = y.y, e[4 * k + 2] = y.z, e[4 * k + 3] = y.w;
    vcnt += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
    ecnt += __popc(y.x) + __popc(y.y) + __popc(y.z) + __popc(y.w);
  }
  int vincl = vcnt, eincl = ecnt;
  for (int o = 1; o < 64; o <<= 1)
  {
    const int a = __shfl_up(vincl, o), b = __shfl_up(eincl, o);
    if ((int) (threadIdx.x & 63) >= o)
    {
      vincl += a;
      eincl += b;
    }
  }
  __shared__ int vsum[4], esum[4];
  if ((threadIdx.x & 63) == 63)
  {
    vsum[threadIdx.x >> 6] = vincl;
    esum[threadIdx.x >> 6] = eincl;
  }
  __syncthreads();
  if (!(esum[0] + esum[1] + esum[2] + esum[3]) || d->error)  // (most blocks of an object mask)
    return;
  int vr = vox_prefix[blockIdx.x] + vincl - vcnt, er = elig_prefix[blockIdx.x] + eincl - ecnt;
  for (int q = 0; q < (int) (threadIdx.x >> 6); q++)
  {
    vr += vsum[q];
    er += esum[q];
  }
  for (int j = 0; j < 16; j++)
  {
    unsigned bits = e[j];
    while (bits)
    {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      E[er++] = (int32_t) (vr + __popc(v[j] & ((1u << b) - 1u)));
    }
    vr += __popc(v[j]);
  }
}

// Sample k of S over the M eligible voxels: E[draw_stratum(M, S, k, seed)], and with M < S the list itself, then kSampleSkip
// (agh_internal.h).  Written to the device list and to its pinned mirror as k_draw_samples does; M goes to the pinned header.
__global__ void k_draw_samples_masked(const int32_t* __restrict__ E, const long long* __restrict__ total, int S,
  unsigned long long seed, int32_t* __restrict__ out, int32_t* __restrict__ host_out, long long* __restrict__ host_count)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const long long M = *total;
  if (k == 0 && host_count)
    *host_count = M;
  if (k >= S)
    return;
  int32_t v = draw_stratum(M, S, k, seed);
  if (v != kSampleSkip)
    v = E[v];
  out[k] = v;
  if (host_out)
    host_out[k] = v;
}

int sample_mask_stage(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, const uint8_t* d_mask, double cell, int64_t S,
  unsigned long long seed, int32_t* d_out, int32_t* h_out, long long* h_count, hipStream_t st)
{
  int rc;
  // (the voxel bitmap exists: the preprocessing queued in front of this stage sized or kept it)
  const int64_t words = c->vox_bitmap_cap;
  if (!c->d_mask_blk)
  {
    if ((rc = dev_alloc(c, &c->d_mask_blk, (size_t) (kVoxMaxWords / kMaskWordsPerBlock) + 1)) ||
        (rc = dev_alloc(c, &c->d_mask_total, 1)))
      return rc;
  }
  if (words > c->mask_bitmap_cap || !c->d_mask_bitmap)
  {
    c->mask_bitmap_cap = 0;
    if ((rc = dev_alloc(c, &c->d_mask_bitmap, (size_t) words + kMaskWordsPerBlock)))
      return rc;
    c->mask_bitmap_cap = words;
  }
  if (n > c->mask_list_cap || !c->d_mask_list)  // (M <= the voxel count <= n)
  {
    c->mask_list_cap = 0;
    if ((rc = dev_alloc(c, &c->d_mask_list, (size_t) std::max<int64_t>(n, 1024))))
      return rc;
    c->mask_list_cap = std::max<int64_t>(n, 1024);
  }
  const int64_t nb = n > 0 ? words / kMaskWordsPerBlock : 0;  // (no point, no bit: vox_stage2 wrote no block counts either)
  if (nb > 0)
  {
    AGH_HIPCHK(c, hipMemsetAsync(c->d_mask_bitmap, 0, (size_t) words * 4, st));
    const int64_t mask_words = (n + 3 + 3) / 4;  // (aligned words that a base up to 3 bytes into one can touch)
    hipLaunchKernelGGL(k_mask_mark, dim3((unsigned) ((mask_words + 255) / 256)), dim3(256), 0, st, d_xyz, stride_floats, n,
      (const uint8_t*) c->d_vox_code, d_mask, (const VoxDesc*) c->d_vox_desc, cell, c->d_mask_bitmap,
      c->voxel_filter_set ? (const unsigned*) c->d_vox_bitmap : (const unsigned*) nullptr);
  }
  if ((rc = vox_count_blocks(c->d_mask_bitmap, nb, c->d_mask_blk, c->d_mask_total, st)) != AGH_OK)
  {
    c->err = "sample mask launch failed";
    return rc;
  }
  if (nb > 0)
    hipLaunchKernelGGL(k_mask_emit, dim3((unsigned) nb), dim3(256), 0, st, (const unsigned*) c->d_vox_bitmap,
      (const unsigned*) c->d_mask_bitmap, (const int*) c->d_vox_blk2, (const int*) c->d_mask_blk, (const VoxDesc*) c->d_vox_desc,
      c->d_mask_list);
  hipLaunchKernelGGL(k_draw_samples_masked, dim3((unsigned) std::max<int64_t>(1, (S + 255) / 256)), dim3(256), 0, st,
    (const int32_t*) c->d_mask_list, (const long long*) c->d_mask_total, (int) S, seed, d_out, h_out, h_count);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "sample mask launch failed";
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}

// ---- the same stage for a batch chain (include/agh.h, agh_localize_batch_masked*; DESIGN.md, "Sample masks in the batch
// chains"): one launch per step for all captures, capture = blockIdx.y as in vox_batch, each capture with its own points,
// descriptor, mask, slot of the eligibility bitmap (the voxel slots' layout) and stretch of the common list ----

// k_mask_mark's loop for capture blockIdx.y.  The aligned-word trick is the capture's own: `a` is its mask's offset in a word, and
// a word that straddles either end of ITS n bytes is read a byte at a time -- in a packed buffer the bytes beside them are a
// neighbour capture's.
__global__ __launch_bounds__(256) void k_mask_mark_batch(VoxBatch vb, const uint8_t* __restrict__ code,
  const uint8_t* const* __restrict__ masks, double cell, unsigned* __restrict__ elig, const unsigned* __restrict__ vox)
{
  const VoxCapture* q = vb.cap + blockIdx.y;
  const VoxDesc* d = vb.desc + blockIdx.y;
  const uint8_t* mask = masks[blockIdx.y];
  const int64_t n = q->n;
  const int64_t a = (int64_t) (reinterpret_cast<uintptr_t>(mask) & 3u);
  const int64_t i0 = 4 * ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) - a;
  if (i0 >= n || d->error)  // (a launch is sized for the largest capture; a lattice that outgrew its slot marks nothing)
    return;
  unsigned m = 0;
  if (i0 >= 0 && i0 + 3 < n)
    m = *reinterpret_cast<const unsigned*>(mask + i0);
  else
    for (int b = 0; b < 4; b++)
      if (i0 + b >= 0 && i0 + b < n)
        m |= (unsigned) mask[i0 + b] << (8 * b);
  if (!m)
    return;
  const float* xyz = q->xyz;
  const int64_t stride = q->stride;
  code += q->code_off;
  elig += (int64_t) blockIdx.y * vb.slot_words;
  if (vox)
    vox += (int64_t) blockIdx.y * vb.slot_words;
  for (int b = 0; b < 4; b++)
  {
    if (!((m >> (8 * b)) & 0xffu))
      continue;
    const int64_t i = i0 + b;
    const unsigned cd = code[i];
    if (!cd)
      continue;
    const int c = (int) (cd >> 1);
    const unsigned long long pos = vox_bit(d, c, xyz + i * stride, cell);
    const unsigned long long w = d->word_ofs[c] + (pos >> 5);
    const unsigned bit = 1u << (unsigned) (pos & 31ull);
    if (vox && !(vox[w] & bit))  // (agh_set_voxel_filter: the point's voxel was pruned)
      continue;
    atomicOr(&elig[w], bit);
  }
}

// Exclusive scan, in place, of slot blockIdx.x's nb block counts; the slot's total, M, to total[blockIdx.x].  (k_vox_scan's loop;
// its batch mode also writes the captures' descriptors, which are the voxeliser's.)
__global__ __launch_bounds__(1024) void k_mask_scan_batch(int* __restrict__ blk, int64_t nb, long long* __restrict__ total)
{
  int* v = blk + (int64_t) blockIdx.x * nb;
  __shared__ long long carry;
  __shared__ int wsum[16];
  if (threadIdx.x == 0)
    carry = 0;
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
      v[i] = (int) (carry + wbase + incl - x);
    __syncthreads();
    if (threadIdx.x == 1023)
      carry += wbase + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0)
    total[blockIdx.x] = carry;
}

// k_mask_emit for slot blockIdx.y: both prefixes are capture-local (the voxel one is vox_batch's d_blk2), so the indices written
// are capture-local too; capture k's list starts at its code_off in the common buffer (M_k <= n[k]).
__global__ __launch_bounds__(256) void k_mask_emit_batch(VoxBatch vb, const unsigned* __restrict__ vox,
  const unsigned* __restrict__ elig, const int* __restrict__ vox_prefix, const int* __restrict__ elig_prefix, int32_t* __restrict__ E)
{
  const int64_t slot0 = (int64_t) blockIdx.y * vb.slot_words, blk0 = (int64_t) blockIdx.y * (vb.slot_words / kMaskWordsPerBlock);
  const size_t w0 = (size_t) slot0 + (size_t) blockIdx.x * kMaskWordsPerBlock + (size_t) threadIdx.x * 16;
  unsigned v[16], e[16];
  const uint4* vs = reinterpret_cast<const uint4*>(vox + w0);
  const uint4* es = reinterpret_cast<const uint4*>(elig + w0);
  int vcnt = 0, ecnt = 0;
  for (int k = 0; k < 4; k++)
  {
    const uint4 x = vs[k], y = es[k];
    v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
    e[4 * k] = y.x, e[4 * k + 1] = y.y, e[4 * k + 2] = y.z, e[4 * k + 3] = y.w;
    vcnt += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
    ecnt += __popc(y.x) + __popc(y.y) + __popc(y.z) + __popc(y.w);
  }
  int vincl = vcnt, eincl = ecnt;
  for (int o = 1; o < 64; o <<= 1)
  {
    const int a = __shfl_up(vincl, o), b = __shfl_up(eincl, o);
    if ((int) (threadIdx.x & 63) >= o)
    {
      vincl += a;
      eincl += b;
    }
  }
  __shared__ int vsum[4], esum[4];
  if ((threadIdx.x & 63) == 63)
  {
    vsum[threadIdx.x >> 6] = vincl;
    esum[threadIdx.x >> 6] = eincl;
  }
  __syncthreads();
  if (!(esum[0] + esum[1] + esum[2] + esum[3]) || vb.desc[blockIdx.y].error)
    return;
  int vr = vox_prefix[blk0 + blockIdx.x] + vincl - vcnt, er = elig_prefix[blk0 + blockIdx.x] + eincl - ecnt;
  for (int q = 0; q < (int) (threadIdx.x >> 6); q++)
  {
    vr += vsum[q];
    er += esum[q];
  }
  E += vb.cap[blockIdx.y].code_off;
  for (int j = 0; j < 16; j++)
  {
    unsigned bits = e[j];
    while (bits)
    {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      E[er++] = (int32_t) (vr + __popc(v[j] & ((1u << b) - 1u)));
    }
    vr += __popc(v[j]);
  }
}

// The batch's sample list under its masks: position j belongs to the capture whose span holds it (as k_batch_samples finds it),
// and is E_k[draw_stratum(M_k, S_k, t, seed_k)] -- capture-local to the pinned list, + cloud_off[k] to the search's -- or
// kSampleSkip.  The first C threads write the M_k to the pinned table (the kernel runs for S_tot = 0 too).
__global__ void k_batch_samples_masked(const BatchCapture* __restrict__ tab, const VoxCapture* __restrict__ cap, int C, int64_t S_tot,
  const int* __restrict__ cloud_off, const int32_t* __restrict__ E, const long long* __restrict__ total, int32_t* __restrict__ out,
  int32_t* __restrict__ host_out, long long* __restrict__ host_total)
{
  const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (j < C)
    host_total[j] = total[j];
  if (j >= S_tot)
    return;
  int k = 0;
  for (int q = 1; q < C; q++)  // (the last capture whose span starts at or before j and is not empty)
    if (tab[q].soff <= j && tab[q].S > 0)
      k = q;
  const int64_t t = j - tab[k].soff;
  int32_t v = draw_stratum(total[k], tab[k].S, (long long) t, tab[k].seed);
  if (v != kSampleSkip)
    v = E[cap[k].code_off + v];
  host_out[j] = v;
  out[j] = v == kSampleSkip ? v : (int32_t) (v + cloud_off[k]);
}

int sample_mask_stage_batch(Ctx* c, const BatchMaskStage& m, hipStream_t st)
{
  const int64_t W = m.vb.slot_words, nb = W / kMaskWordsPerBlock;
  const unsigned Cy = (unsigned) m.C;
  AGH_HIPCHK(c, hipMemsetAsync(m.elig, 0, (size_t) m.C * (size_t) W * 4, st));
  if (m.n_max > 0)
  {
    const int64_t mask_words = (m.n_max + 3 + 3) / 4;  // (aligned words that a base up to 3 bytes into one can touch)
    hipLaunchKernelGGL(k_mask_mark_batch, dim3((unsigned) ((mask_words + 255) / 256), Cy), dim3(256), 0, st, m.vb, m.code, m.mask,
      m.cell, m.elig, c->voxel_filter_set ? m.bitmap : (const unsigned*) nullptr);
  }
  int rc = vox_count_blocks_batch(m.vb, m.C, m.elig, m.eblk, st);
  if (rc == AGH_OK)
  {
    hipLaunchKernelGGL(k_mask_scan_batch, dim3(Cy), dim3(1024), 0, st, m.eblk, nb, m.total);
    if (m.n_max > 0)
      hipLaunchKernelGGL(k_mask_emit_batch, dim3((unsigned) nb, Cy), dim3(256), 0, st, m.vb, m.bitmap, (const unsigned*) m.elig,
        m.blk2, (const int*) m.eblk, m.list);
    const int64_t threads = std::max<int64_t>(m.S_tot, m.C);
    hipLaunchKernelGGL(k_batch_samples_masked, dim3((unsigned) ((threads + 255) / 256)), dim3(256), 0, st, m.tab, m.vb.cap, m.C,
      m.S_tot, m.cloud_off, (const int32_t*) m.list, (const long long*) m.total, m.d_out, m.h_out, m.h_total);
    if (hipGetLastError() != hipSuccess)
      rc = AGH_ERR_HIP;
  }
  if (rc != AGH_OK)
    c->err = "sample mask launch failed";
  return rc;
}

}  // namespace agh
