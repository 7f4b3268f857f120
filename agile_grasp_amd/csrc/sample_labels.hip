// sample_labels.hip -- the sample lists of a labelled chain (include/agh.h, agh_localize_labeled*; DESIGN.md, "Label images").
//
// One label byte per raw point names the object the point belongs to (0: none, j + 1: object j of K <= 64).  A voxel is eligible
// for object j iff a kept raw point with label j + 1 falls into it (sample_mask.hip's rule, per object); object j's samples are
// draw_stratum's strata over E_j, the ascending list of its eligible voxel indices.  K eligibility bitmaps of the lattice's size
// would cost K x the lattice; instead every VOXEL gets one 64-bit set of the objects seen in it:
//   k_vox_word_rank   the voxel bits before each bitmap word inside its 4096-word block, so that a raw point finds the INDEX of
//                     its voxel (block prefix + word rank + bits below its own) without a search;
//   k_label_mark      raw point -> atomicOr of its object's bit into objset[voxel index];
//   k_label_count / k_label_scan / k_label_emit
//                     a stream compaction of the voxel indices per object: per wave one ballot per object PRESENT in the wave,
//                     the waves' counts carried through LDS, the work-groups' counts scanned by one wave per object;
//   k_draw_samples_labeled   sample k of object j = E_j[stratum], to the device list and the pinned mirrors.
// The lists share one buffer of n entries (a raw point adds at most one (voxel, object) pair), object after object.  Launches are
// sized from the raw point count; the voxel count is read on the device.  Everything is queued on the chain's stream behind the
// voxeliser: no synchronisation is added.
//
// The batch forms (include/agh.h, agh_localize_batch_labeled*; DESIGN.md, "Label images in the batch chains") run the same steps
// once for all captures, capture = blockIdx.y as in vox_batch: k_vox_word_rank_batch over the bitmap slots, k_label_mark_batch
// into one object set per voxel of the COMMON voxel array (bit j = the capture-local object: a voxel belongs to one capture),
// k_label_count_batch / k_label_scan / k_label_emit_batch with one row of group counts per LIST (capture k's object j is list
// first_list[k] + j), and k_batch_samples_labeled.  Capture k's lists lie inside [raw_off[k], raw_off[k] + n[k]) of the one buffer.
#include "agh_internal.h"

#include <algorithm>

namespace agh
{

constexpr int kLabelWordsPerBlock = 4096;  // voxelize.hip's kWordsPerBlock: 16 words per thread of 256

// One work-group per block of 4096 bitmap words, a thread holding its 16: rank[w] = the voxel bits of the block in front of w.
// (the block of 4096 words at w0 - 16 * threadIdx.x; the whole work-group comes here)
__device__ __forceinline__ void vox_word_rank_block(const unsigned* __restrict__ vox, unsigned* __restrict__ rank, size_t w0)
{
  unsigned v[16];
  const uint4* vs = reinterpret_cast<const uint4*>(vox + w0);
  int cnt = 0;
  for (int k = 0; k < 4; k++)
  {
    const uint4 x = vs[k];
    v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
    cnt += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
  }
  int incl = cnt;
  for (int o = 1; o < 64; o <<= 1)
  {
    const int a = __shfl_up(incl, o);
    if ((int) (threadIdx.x & 63) >= o)
      incl += a;
  }
  __shared__ int wsum[4];
  if ((threadIdx.x & 63) == 63)
    wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned r = (unsigned) (incl - cnt);
  for (int q = 0; q < (int) (threadIdx.x >> 6); q++)
    r += (unsigned) wsum[q];
  unsigned out[16];
  for (int j = 0; j < 16; j++)
  {
    out[j] = r;
    r += (unsigned) __popc(v[j]);
  }
  uint4* rs = reinterpret_cast<uint4*>(rank + w0);
  for (int k = 0; k < 4; k++)
    rs[k] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
}

__global__ __launch_bounds__(256) void k_vox_word_rank(const unsigned* __restrict__ vox, const VoxDesc* __restrict__ d,
  unsigned* __restrict__ rank)
{
  if (d->error || (unsigned long long) blockIdx.x >= d->n_words / kLabelWordsPerBlock)
    return;
  vox_word_rank_block(vox, rank, (size_t) blockIdx.x * kLabelWordsPerBlock + (size_t) threadIdx.x * 16);
}

// ... and over the bitmap slots of a batch, slot blockIdx.y (VoxBatch::slot_words words, a multiple of the block): the ranks are
// inside the block, so they go with the capture-local block prefixes of vox_batch (d_blk2) as they are
__global__ __launch_bounds__(256) void k_vox_word_rank_batch(VoxBatch vb, const unsigned* __restrict__ vox, unsigned* __restrict__ rank)
{
  const VoxDesc* d = vb.desc + blockIdx.y;
  if (d->error || (unsigned long long) blockIdx.x * kLabelWordsPerBlock >= d->n_words)  // (the slot beyond the lattice holds no bit)
    return;
  vox_word_rank_block(vox, rank,
    (size_t) blockIdx.y * (size_t) vb.slot_words + (size_t) blockIdx.x * kLabelWordsPerBlock + (size_t) threadIdx.x * 16);
}

// Raw point i with label 1..K and code[i] != 0: its object's bit into the set of its voxel.  A thread takes the four label bytes
// of one ALIGNED 32-bit word, the words that straddle either end a byte at a time (k_mask_mark, sample_mask.hip).  vox, rank: the
// cloud's bitmap (slot); vox_prefix: its block prefixes; objset: the sets of ITS voxels.
__device__ __forceinline__ void label_mark_points(const float* __restrict__ xyz, int64_t stride, int64_t n,
  const uint8_t* __restrict__ code, const uint8_t* __restrict__ labels, int K, const VoxDesc* __restrict__ d, double cell,
  const unsigned* __restrict__ vox, const int* __restrict__ vox_prefix, const unsigned* __restrict__ rank,
  unsigned long long* __restrict__ objset)
{
  const int64_t a = (int64_t) (reinterpret_cast<uintptr_t>(labels) & 3u);
  const int64_t i0 = 4 * ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) - a;
  if (i0 >= n || d->error)
    return;
  unsigned m = 0;
  if (i0 >= 0 && i0 + 3 < n)
    m = *reinterpret_cast<const unsigned*>(labels + i0);
  else
    for (int b = 0; b < 4; b++)
      if (i0 + b >= 0 && i0 + b < n)
        m |= (unsigned) labels[i0 + b] << (8 * b);
  if (!m)
    return;
  for (int b = 0; b < 4; b++)
  {
    const int label = (int) ((m >> (8 * b)) & 0xffu);
    if (label < 1 || label > K)
      continue;
    const int64_t i = i0 + b;
    const unsigned cd = code[i];
    if (!cd)
      continue;
    const int c = (int) (cd >> 1);
    const unsigned long long pos = vox_bit(d, c, xyz + i * stride, cell);
    const unsigned long long w = d->word_ofs[c] + (pos >> 5);
    const unsigned word = vox[w], bit = 1u << (unsigned) (pos & 31ull);
    if (!(word & bit))  // (agh_set_voxel_filter: the point's voxel was pruned -- the index below would be its neighbour's)
      continue;
    const unsigned below = word & (bit - 1u);
    const int64_t v = (int64_t) vox_prefix[w >> 12] + (int64_t) rank[w] + __popc(below);
    if (v < n)  // (the voxel count is at most the kept points': always)
      atomicOr(&objset[v], 1ull << (label - 1));
  }
}

__global__ __launch_bounds__(256) void k_label_mark(const float* __restrict__ xyz, int64_t stride, int64_t n,
  const uint8_t* __restrict__ code, const uint8_t* __restrict__ labels, int K, const VoxDesc* __restrict__ d, double cell,
  const unsigned* __restrict__ vox, const int* __restrict__ vox_prefix, const unsigned* __restrict__ rank,
  unsigned long long* __restrict__ objset)
{
  label_mark_points(xyz, stride, n, code, labels, K, d, cell, vox, vox_prefix, rank, objset);
}

// k_label_mark's loop for capture blockIdx.y: its points, codes (code_off), labels (a table of pointers, any byte alignment --
// the straddling words are the capture's own, see k_mask_mark_batch), bitmap slot and block prefixes; its voxels' sets start at
// cloud_off[capture] of the common array, which lies at or below the capture's first raw point: a voxel index below the
// capture's n stays inside the array's one entry per raw point.
__global__ __launch_bounds__(256) void k_label_mark_batch(VoxBatch vb, const uint8_t* __restrict__ code,
  const uint8_t* const* __restrict__ labels, const LabelCapture* __restrict__ lc, double cell, const unsigned* __restrict__ vox,
  const int* __restrict__ vox_prefix, const unsigned* __restrict__ rank, const int* __restrict__ cloud_off,
  unsigned long long* __restrict__ objset)
{
  const VoxCapture* q = vb.cap + blockIdx.y;
  const int64_t slot0 = (int64_t) blockIdx.y * vb.slot_words;
  // (a capture whose descriptor carries an error has no voxels: label_mark_points returns at once)
  label_mark_points(q->xyz, q->stride, q->n, code + q->code_off, labels[blockIdx.y], lc[blockIdx.y].K, vb.desc + blockIdx.y, cell,
    vox + slot0, vox_prefix + slot0 / kLabelWordsPerBlock, rank + slot0, objset + cloud_off[blockIdx.y]);
}

// One wave's share of the compaction: lane = voxel, set = its objects.  For each object present in the wave one ballot; f(j,
// ballot) sees every object once, in every lane.
template <typename F>
__device__ __forceinline__ void label_wave_objects(unsigned long long set, F f)
{
  unsigned long long present = set;
  for (int o = 32; o > 0; o >>= 1)
    present |= __shfl_xor(present, o);
  while (present)  // (wave-uniform)
  {
    const int j = __ffsll((long long) present) - 1;
    present &= present - 1ull;
    f(j, (unsigned long long) __ballot((int) ((set >> j) & 1ull)));
  }
}

// counts[j * n_groups + g]: the voxels of work-group g (256 voxel indices) that are eligible for object j.  (The whole
// work-group comes here; objset: the sets of the cloud's nv voxels.)
__device__ __forceinline__ void label_count_group(const unsigned long long* __restrict__ objset, int64_t nv, int K, int64_t n_groups,
  int* __restrict__ counts)
{
  __shared__ int cnt[4][64];
  const int tid = threadIdx.x, wave = tid >> 6;
  cnt[wave][tid & 63] = 0;
  __syncthreads();
  const int64_t v = (int64_t) blockIdx.x * kLabelGroup + tid;
  const unsigned long long set = v < nv ? objset[v] : 0ull;
  label_wave_objects(set, [&](int j, unsigned long long ballot) {
    if ((tid & 63) == 0)
      cnt[wave][j] = __popcll(ballot);
  });
  __syncthreads();
  if (tid < K)
    counts[(int64_t) tid * n_groups + blockIdx.x] = cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
}

__global__ __launch_bounds__(kLabelGroup) void k_label_count(const unsigned long long* __restrict__ objset,
  const VoxDesc* __restrict__ d, int64_t n, int K, int64_t n_groups, int* __restrict__ counts)
{
  label_count_group(objset, label_voxels(d, n), K, n_groups, counts);
}

// ... for capture blockIdx.y of a batch: its voxels' sets at cloud_off, its objects' rows first_list .. first_list + K - 1 of the
// call's L rows.  n_groups is sized for the largest capture, so every row is written whole.
__global__ __launch_bounds__(kLabelGroup) void k_label_count_batch(VoxBatch vb, const unsigned long long* __restrict__ objset,
  const LabelCapture* __restrict__ lc, const int* __restrict__ cloud_off, int64_t n_groups, int* __restrict__ counts)
{
  const int64_t nv = label_voxels(vb.desc + blockIdx.y, vb.cap[blockIdx.y].n);  // (0 for a capture with an error)
  label_count_group(objset + cloud_off[blockIdx.y], nv, lc[blockIdx.y].K, n_groups,
    counts + (int64_t) lc[blockIdx.y].first_list * n_groups);
}

// One wave per object: its work-groups' counts become their exclusive scan, in place; the sum is M_j.
__global__ __launch_bounds__(64) void k_label_scan(int* __restrict__ counts, int64_t n_groups, long long* __restrict__ totals)
{
  int* row = counts + (int64_t) blockIdx.x * n_groups;
  const int lane = threadIdx.x;
  long long run = 0;
  for (int64_t g0 = 0; g0 < n_groups; g0 += 64)
  {
    const int64_t g = g0 + lane;
    const int x = g < n_groups ? row[g] : 0;
    int incl = x;
    for (int o = 1; o < 64; o <<= 1)
    {
      const int a = __shfl_up(incl, o);
      if (lane >= o)
        incl += a;
    }
    if (g < n_groups)
      row[g] = (int) run + incl - x;
    run += __shfl(incl, 63);
  }
  if (lane == 0)
    totals[blockIdx.x] = run;
}

// base[j], the start of E_j in the shared list: the exclusive scan of the M_j (K <= 64 terms, by the first K threads)
__device__ __forceinline__ void label_bases(const long long* __restrict__ totals, int K, long long* base)
{
  if ((int) threadIdx.x < K)
  {
    long long s = 0;
    for (int q = 0; q < (int) threadIdx.x; q++)
      s += totals[q];
    base[threadIdx.x] = s;
  }
}

// E[base_j + the work-group's offset + the waves in front + the lanes in front] = the voxel index: ascending per object.  (The
// whole work-group comes here; objset, offsets, totals, E: the cloud's own, E with room for `room` entries.)
__device__ __forceinline__ void label_emit_group(const unsigned long long* __restrict__ objset, int64_t nv, int64_t room, int K,
  int64_t n_groups, const int* __restrict__ offsets, const long long* __restrict__ totals, int32_t* __restrict__ E)
{
  __shared__ int cnt[4][64];
  __shared__ long long base[64];
  if ((int64_t) blockIdx.x * kLabelGroup >= nv)  // (uniform over the work-group)
    return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  cnt[wave][lane] = 0;
  label_bases(totals, K, base);
  __syncthreads();
  const int64_t v = (int64_t) blockIdx.x * kLabelGroup + tid;
  const unsigned long long set = v < nv ? objset[v] : 0ull;
  label_wave_objects(set, [&](int j, unsigned long long ballot) {
    if (lane == 0)
      cnt[wave][j] = __popcll(ballot);
  });
  __syncthreads();
  label_wave_objects(set, [&](int j, unsigned long long ballot) {
    if (!((set >> j) & 1ull))
      return;
    int64_t at = base[j] + offsets[(int64_t) j * n_groups + blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
    for (int q = 0; q < wave; q++)
      at += cnt[q][j];
    if (at < room)  // (the pairs are at most the raw points: always)
      E[at] = (int32_t) v;
  });
}

__global__ __launch_bounds__(kLabelGroup) void k_label_emit(const unsigned long long* __restrict__ objset,
  const VoxDesc* __restrict__ d, int64_t n, int K, int64_t n_groups, const int* __restrict__ offsets,
  const long long* __restrict__ totals, int32_t* __restrict__ E)
{
  label_emit_group(objset, label_voxels(d, n), n, K, n_groups, offsets, totals, E);
}

// ... for capture blockIdx.y of a batch: the indices written are capture-local, its lists start at its code_off of the common
// buffer, object after object, and hold at most its n entries
__global__ __launch_bounds__(kLabelGroup) void k_label_emit_batch(VoxBatch vb, const unsigned long long* __restrict__ objset,
  const LabelCapture* __restrict__ lc, const int* __restrict__ cloud_off, int64_t n_groups, const int* __restrict__ offsets,
  const long long* __restrict__ totals, int32_t* __restrict__ E)
{
  const VoxCapture* q = vb.cap + blockIdx.y;
  const int first = lc[blockIdx.y].first_list;
  label_emit_group(objset + cloud_off[blockIdx.y], label_voxels(vb.desc + blockIdx.y, q->n), q->n, lc[blockIdx.y].K, n_groups,
    offsets + (int64_t) first * n_groups, totals + first, E + q->code_off);
}

// Sample k of object j: position j * S + k of the call's list.  E_j[draw_stratum(M_j, S, k, seed)], and with M_j < S the list
// itself, then kSampleSkip -- to the device list and its pinned mirror; the M_j go to the pinned table.
__global__ __launch_bounds__(256) void k_draw_samples_labeled(const int32_t* __restrict__ E, const long long* __restrict__ totals,
  int K, int S, unsigned long long seed, int32_t* __restrict__ out, int32_t* __restrict__ host_out, long long* __restrict__ host_counts)
{
  __shared__ long long base[64];
  label_bases(totals, K, base);
  __syncthreads();
  const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (t < K)
    host_counts[t] = totals[t];
  if (t >= (int64_t) K * S)
    return;
  const int j = (int) (t / S), k = (int) (t % S);
  int32_t v = draw_stratum(totals[j], S, k, seed);
  if (v != kSampleSkip)
    v = E[base[j] + v];
  out[t] = v;
  host_out[t] = v;
}

// The batch's sample lists under its labels: position p belongs to the list whose span holds it (as k_batch_samples finds the
// capture), list l = object j of capture k, and is E_{k,j}[draw_stratum(M_l, S_k, t, seed_k)] -- capture-local to the pinned
// list, + cloud_off[k] to the search's -- or kSampleSkip.  The first L threads write the M_l to the pinned table (the kernel runs
// for S_tot = 0 too).
__global__ __launch_bounds__(256) void k_batch_samples_labeled(const BatchCapture* __restrict__ tab, const VoxCapture* __restrict__ cap,
  const LabelCapture* __restrict__ lc, int L, int64_t S_tot, const int* __restrict__ cloud_off, const int32_t* __restrict__ E,
  const long long* __restrict__ totals, int32_t* __restrict__ out, int32_t* __restrict__ host_out, long long* __restrict__ host_counts)
{
  const int64_t p = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (p < L)
    host_counts[p] = totals[p];
  if (p >= S_tot)
    return;
  int l = 0;
  for (int q = 1; q < L; q++)  // (the last list whose span starts at or before p and is not empty)
    if (tab[q].soff <= p && tab[q].S > 0)
      l = q;
  const int k = tab[l].capture, j = tab[l].object;
  int32_t v = draw_stratum(totals[l], tab[l].S, (long long) (p - tab[l].soff), tab[l].seed);
  if (v != kSampleSkip)
  {
    long long at = cap[k].code_off + v;
    for (int q = 0; q < j; q++)  // (E_{k,j} lies behind the capture's lists in front of it)
      at += totals[lc[k].first_list + q];
    v = E[at];
  }
  host_out[p] = v;
  out[p] = v == kSampleSkip ? v : (int32_t) (v + cloud_off[k]);
}

// the buffers of the stage, for a bitmap of `words` words, n raw points and `groups` group counts: kept and grown by the context
int ensure_label_buffers(Ctx* c, int64_t words, int64_t n, int64_t groups)
{
  int rc;
  if (!c->d_label_totals)
  {
    if ((rc = dev_alloc(c, &c->d_label_totals, (size_t) kMaxClouds)))
      return rc;
    if (hipHostMalloc((void**) &c->h_label_counts, sizeof(long long) * kMaxClouds, hipHostMallocDefault) != hipSuccess)
    {
      c->h_label_counts = nullptr;
      c->err = "hipHostMalloc failed (label counts)";
      return AGH_ERR_HIP;
    }
  }
  if (words > c->label_rank_cap || !c->d_label_rank)
  {
    c->label_rank_cap = 0;
    if ((rc = dev_alloc(c, &c->d_label_rank, (size_t) words + kLabelWordsPerBlock)))
      return rc;
    c->label_rank_cap = words;
  }
  if (n > c->label_set_cap || !c->d_label_set)
  {
    c->label_set_cap = 0;
    if ((rc = dev_alloc(c, &c->d_label_set, (size_t) std::max<int64_t>(n, 1024))))
      return rc;
    c->label_set_cap = std::max<int64_t>(n, 1024);
  }
  if (n > c->mask_list_cap || !c->d_mask_list)  // (the lists share sample_mask.hip's: their entries are at most n in all)
  {
    c->mask_list_cap = 0;
    if ((rc = dev_alloc(c, &c->d_mask_list, (size_t) std::max<int64_t>(n, 1024))))
      return rc;
    c->mask_list_cap = std::max<int64_t>(n, 1024);
  }
  if (groups > c->label_group_cap || !c->d_label_groups)
  {
    c->label_group_cap = 0;
    if ((rc = dev_alloc(c, &c->d_label_groups, (size_t) std::max<int64_t>(groups, 1024))))
      return rc;
    c->label_group_cap = std::max<int64_t>(groups, 1024);
  }
  return AGH_OK;
}

// The stage's first part for a label image: the object sets of the voxels (any: there is a point, hence a bitmap block).
int sample_label_stage(Ctx* c, const float* d_xyz, int64_t stride_floats, int64_t n, const uint8_t* d_labels, int K, double cell,
  int64_t S, unsigned long long seed, int32_t* d_out, int32_t* h_out, hipStream_t st)
{
  int rc;
  // (the voxel bitmap exists: the preprocessing queued in front of this stage sized or kept it)
  const int64_t words = c->vox_bitmap_cap;
  const int64_t n_groups = (n + kLabelGroup - 1) / kLabelGroup;
  if ((rc = ensure_label_buffers(c, words, n, (int64_t) K * n_groups)) != AGH_OK)
    return rc;
  const VoxDesc* desc = (const VoxDesc*) c->d_vox_desc;
  const int64_t nb = n > 0 ? words / kLabelWordsPerBlock : 0;  // (no point, no bit: vox_stage2 wrote no block counts either)
  if (nb > 0)
  {
    AGH_HIPCHK(c, hipMemsetAsync(c->d_label_set, 0, (size_t) n * 8, st));
    hipLaunchKernelGGL(k_vox_word_rank, dim3((unsigned) nb), dim3(256), 0, st, (const unsigned*) c->d_vox_bitmap, desc,
      c->d_label_rank);
    const int64_t label_words = (n + 3 + 3) / 4;  // (aligned words that a base up to 3 bytes into one can touch)
    hipLaunchKernelGGL(k_label_mark, dim3((unsigned) ((label_words + 255) / 256)), dim3(256), 0, st, d_xyz, stride_floats, n,
      (const uint8_t*) c->d_vox_code, d_labels, K, desc, cell, (const unsigned*) c->d_vox_bitmap, (const int*) c->d_vox_blk2,
      (const unsigned*) c->d_label_rank, c->d_label_set);
  }
  return label_compact_stage(c, n, K, nb > 0, S, seed, d_out, h_out, st);
}

// ... and its second, shared with the clustered chain (sample_cluster.hip), whose object sets come from the cloud: the
// compaction of c->d_label_set into the lists and the draw (any == false: no voxel, every list is empty).  The label buffers
// are there (ensure_label_buffers).
int label_compact_stage(Ctx* c, int64_t n, int K, bool any, int64_t S, unsigned long long seed, int32_t* d_out, int32_t* h_out,
  hipStream_t st)
{
  const VoxDesc* desc = (const VoxDesc*) c->d_vox_desc;
  const int64_t n_groups = (n + kLabelGroup - 1) / kLabelGroup;
  if (any)
  {
    hipLaunchKernelGGL(k_label_count, dim3((unsigned) n_groups), dim3(kLabelGroup), 0, st,
      (const unsigned long long*) c->d_label_set, desc, n, K, n_groups, c->d_label_groups);
    hipLaunchKernelGGL(k_label_scan, dim3((unsigned) K), dim3(64), 0, st, c->d_label_groups, n_groups, c->d_label_totals);
    hipLaunchKernelGGL(k_label_emit, dim3((unsigned) n_groups), dim3(kLabelGroup), 0, st,
      (const unsigned long long*) c->d_label_set, desc, n, K, n_groups, (const int*) c->d_label_groups,
      (const long long*) c->d_label_totals, c->d_mask_list);
  }
  else
    AGH_HIPCHK(c, hipMemsetAsync(c->d_label_totals, 0, sizeof(long long) * kMaxClouds, st));
  hipLaunchKernelGGL(k_draw_samples_labeled, dim3((unsigned) std::max<int64_t>(1, ((int64_t) K * S + 255) / 256)), dim3(256), 0, st,
    (const int32_t*) c->d_mask_list, (const long long*) c->d_label_totals, K, (int) S, seed, d_out, h_out, c->h_label_counts);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "sample label launch failed";
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}

// The stage over a batch (BatchLabelStage, agh_internal.h): one launch per step, none that depends on n_captures or L.
int sample_label_stage_batch(Ctx* c, const BatchLabelStage& m, hipStream_t st)
{
  int rc;
  const int64_t W = m.vb.slot_words, nb = W / kLabelWordsPerBlock;
  const int64_t n_groups = (m.n_max + kLabelGroup - 1) / kLabelGroup;
  if ((rc = ensure_label_buffers(c, (int64_t) m.C * W, m.n_tot, (int64_t) m.L * n_groups)) != AGH_OK)
    return rc;
  const unsigned Cy = (unsigned) m.C;
  const bool any = m.n_max > 0 && nb > 0;
  if (any)
  {
    AGH_HIPCHK(c, hipMemsetAsync(c->d_label_set, 0, (size_t) m.n_tot * 8, st));
    hipLaunchKernelGGL(k_vox_word_rank_batch, dim3((unsigned) nb, Cy), dim3(256), 0, st, m.vb, m.bitmap, c->d_label_rank);
    const int64_t label_words = (m.n_max + 3 + 3) / 4;  // (aligned words that a base up to 3 bytes into one can touch)
    hipLaunchKernelGGL(k_label_mark_batch, dim3((unsigned) ((label_words + 255) / 256), Cy), dim3(256), 0, st, m.vb, m.code, m.labels,
      m.lists, m.cell, m.bitmap, m.blk2, (const unsigned*) c->d_label_rank, m.cloud_off, c->d_label_set);
  }
  return label_compact_stage_batch(c, m, any, st);
}

// ... and its second part, shared with the clustered batch (sample_cluster.hip, sample_cluster_stage_batch), whose object sets
// come from the clouds: the compaction of c->d_label_set into the L lists and the draw (any == false: no voxel, every list is
// empty).  The label buffers are there (ensure_label_buffers).
int label_compact_stage_batch(Ctx* c, const BatchLabelStage& m, bool any, hipStream_t st)
{
  const int64_t n_groups = (m.n_max + kLabelGroup - 1) / kLabelGroup;
  const unsigned Cy = (unsigned) m.C;
  const LabelCapture* lc = m.lists;
  if (any)
  {
    hipLaunchKernelGGL(k_label_count_batch, dim3((unsigned) n_groups, Cy), dim3(kLabelGroup), 0, st, m.vb,
      (const unsigned long long*) c->d_label_set, lc, m.cloud_off, n_groups, c->d_label_groups);
    hipLaunchKernelGGL(k_label_scan, dim3((unsigned) m.L), dim3(64), 0, st, c->d_label_groups, n_groups, c->d_label_totals);
    hipLaunchKernelGGL(k_label_emit_batch, dim3((unsigned) n_groups, Cy), dim3(kLabelGroup), 0, st, m.vb,
      (const unsigned long long*) c->d_label_set, lc, m.cloud_off, n_groups, (const int*) c->d_label_groups,
      (const long long*) c->d_label_totals, c->d_mask_list);
  }
  else
    AGH_HIPCHK(c, hipMemsetAsync(c->d_label_totals, 0, sizeof(long long) * kMaxClouds, st));
  const int64_t threads = std::max<int64_t>(m.S_tot, m.L);
  hipLaunchKernelGGL(k_batch_samples_labeled, dim3((unsigned) ((threads + 255) / 256)), dim3(256), 0, st, m.tab, m.vb.cap, lc, m.L,
    m.S_tot, m.cloud_off, (const int32_t*) c->d_mask_list, (const long long*) c->d_label_totals, m.d_out, m.h_out, c->h_label_counts);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "sample label launch failed";
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}

}  // namespace agh
