// depth.hip -- the localize chain's third source kind (include/agh.h, agh_localize_depth*): a capture as the sensor's driver hands it
// over, one depth image per camera, back-projected on the device into the raw buffer an upload of points would have filled.
// k_deproject and its launch, the argument rules, the context's two depth buffers (this capture's images and the staged next
// ones), agh_deproject and agh_localize_depth_stage; the chain itself is localize.hip's.  The depth filter (agh_set_depth_filter):
// its setting, k_deproject_filtered / k_deproject_filtered_batch, which take the plain kernels' place while a filter is set, and
// their per-view counters.  depth_fuse.hip (agh_fuse_depth: a burst of frames fused into one device image ahead of all this) is included
// at the end.
#include "agh_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

using namespace agh;

namespace
{
constexpr int kRun = 4;       // consecutive pixels of one row per lane: 8 (U16) or 16 (F32) bytes in, 48 bytes = three 16-byte stores out
constexpr int kDeprojBlock = 256;
constexpr int kMaxDepthViews = 2 * kMaxClouds;  // k_deproject_batch's table: two images for each of a batch's captures

typedef __attribute__((address_space(1))) uint8_t GlobalBytes;
typedef uint32_t U32x2 __attribute__((ext_vector_type(2)));
typedef float F32x4 __attribute__((ext_vector_type(4)));

struct DepthView
{
  const uint8_t* data;   // row v at data + v * stride
  int64_t stride;        // bytes
  int64_t base;          // index of pixel (0, 0)'s point in the output
  int32_t w, h, fmt;
  int32_t runs;          // per row: ceil(w / kRun)
  uint32_t first_block;  // of the launch: the image's blocks are [first_block, next image's first_block)
  float scale, kx, ky, cx, cy;
  float p[12];
};
struct DepthArgs
{
  DepthView v[2];
};

// One lane = kRun consecutive pixels of one row of one image (a block belongs to ONE image, so the view is read with scalar loads):
// run g of the view `im`, runs row-major, im.runs per row.  The one copy of the per-run body, k_deproject's and k_deproject_batch's.
// The contract's arithmetic (include/agh.h): float32, left to right, not contracted (-ffp-contract=off is the build's).
// Wide accesses where the addresses allow them -- an 8-byte (U16) or 16-byte (F32) load of the run, three 16-byte stores of its
// twelve floats -- element accesses on unaligned rows, on row tails and where the run's first point is not a multiple of four
// points into the output.  Plain vector stores: the voxeliser reads the array next, from the L2.
__device__ __forceinline__ void deproject_run(const DepthView& im, int64_t g, float* __restrict__ out)
{
  if (g >= (int64_t) im.runs * im.h)
    return;
  const int v = (int) (g / im.runs);
  const int u0 = (int) (g - (int64_t) v * im.runs) * kRun;
  const int cnt = min(kRun, im.w - u0);
  // (global, not flat, loads also where the pointer comes from the table and not from the kernel's arguments)
  const GlobalBytes* row = (const GlobalBytes*) im.data + (int64_t) v * im.stride;
  float z[kRun];
  bool ok[kRun];
  if (im.fmt == AGH_DEPTH_U16)
  {
    const __attribute__((address_space(1))) uint16_t* p = (const __attribute__((address_space(1))) uint16_t*) row + u0;
    uint32_t raw[kRun] = { 0, 0, 0, 0 };
    if (cnt == kRun && ((uintptr_t) p & 7) == 0)
    {
      const U32x2 q = *(const __attribute__((address_space(1))) U32x2*) p;
      raw[0] = q.x & 0xffffu;
      raw[1] = q.x >> 16;
      raw[2] = q.y & 0xffffu;
      raw[3] = q.y >> 16;
    }
    else
    {
#pragma unroll
      for (int j = 0; j < kRun; j++)
        if (j < cnt)
          raw[j] = p[j];
    }
#pragma unroll
    for (int j = 0; j < kRun; j++)
    {
      z[j] = (float) raw[j] * im.scale;
      ok[j] = raw[j] != 0;
    }
  }
  else
  {
    const __attribute__((address_space(1))) float* p = (const __attribute__((address_space(1))) float*) row + u0;
    if (cnt == kRun && ((uintptr_t) p & 15) == 0)
    {
      const F32x4 q = *(const __attribute__((address_space(1))) F32x4*) p;
      z[0] = q.x;
      z[1] = q.y;
      z[2] = q.z;
      z[3] = q.w;
    }
    else
    {
#pragma unroll
      for (int j = 0; j < kRun; j++)
        z[j] = j < cnt ? p[j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kRun; j++)
      ok[j] = z[j] > 0.0f && z[j] < __builtin_huge_valf();
  }
  const float qnan = __builtin_nanf("");
  const float fv = (float) v;
  float o[3 * kRun];
#pragma unroll
  for (int j = 0; j < kRun; j++)
  {
    const float x = (((float) (u0 + j) - im.cx) * z[j]) * im.kx;
    const float y = ((fv - im.cy) * z[j]) * im.ky;
    o[3 * j + 0] = ok[j] ? ((im.p[0] * x + im.p[1] * y) + im.p[2] * z[j]) + im.p[3] : qnan;
    o[3 * j + 1] = ok[j] ? ((im.p[4] * x + im.p[5] * y) + im.p[6] * z[j]) + im.p[7] : qnan;
    o[3 * j + 2] = ok[j] ? ((im.p[8] * x + im.p[9] * y) + im.p[10] * z[j]) + im.p[11] : qnan;
  }
  const int64_t idx = im.base + (int64_t) v * im.w + u0;
  float* dst = out + 3 * idx;
  if (cnt == kRun && (idx & 3) == 0)  // (out is at least 16-byte aligned: 12 * idx is then a multiple of 16)
  {
    float4* d4 = reinterpret_cast<float4*>(dst);
    d4[0] = make_float4(o[0], o[1], o[2], o[3]);
    d4[1] = make_float4(o[4], o[5], o[6], o[7]);
    d4[2] = make_float4(o[8], o[9], o[10], o[11]);
  }
  else
  {
#pragma unroll
    for (int j = 0; j < kRun; j++)
      if (j < cnt)
      {
        dst[3 * j + 0] = o[3 * j + 0];
        dst[3 * j + 1] = o[3 * j + 1];
        dst[3 * j + 2] = o[3 * j + 2];
      }
  }
}

extern "C" __global__ __launch_bounds__(kDeprojBlock) void k_deproject(DepthArgs a, int n_images, float* __restrict__ out)
{
  const int k = (n_images > 1 && blockIdx.x >= a.v[1].first_block) ? 1 : 0;
  const DepthView& im = a.v[k];
  deproject_run(im, (int64_t) (blockIdx.x - im.first_block) * kDeprojBlock + threadIdx.x, out);
}

// Every image of every capture of a batch in one launch: the views (up to kMaxDepthViews, more than kernel arguments hold) are a
// device table in launch order, `base` the index of the view's first point in the whole batch's array.  A work-group finds its
// view with a uniform bisection over first_block -- the last view whose first block is at or before this one; every view has at
// least one block -- and reads the record with scalar loads, as k_deproject reads its arguments.
extern "C" __global__ __launch_bounds__(kDeprojBlock) void k_deproject_batch(const DepthView* __restrict__ views, int n_views,
  float* __restrict__ out)
{
  int lo = 0, hi = n_views - 1;
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (views[mid].first_block <= blockIdx.x)
      lo = mid;
    else
      hi = mid - 1;
  }
  const DepthView& im = views[lo];
  deproject_run(im, (int64_t) (blockIdx.x - im.first_block) * kDeprojBlock + threadIdx.x, out);
}

// ---- the depth filter (include/agh.h, agh_set_depth_filter): k_deproject with a look at every pixel's neighbours ----
// A work-group owns one tile of kTileW x kTileH pixels of ONE image (first_block counts tiles here), lane t the run of kRun pixels
// at row t / 16, columns 4 (t % 16)...: the lanes 16r..16r+15 hold one row of the tile.  The tile's depths and a halo of `radius`
// rows and columns go into LDS as float32, NaN for every pixel that is outside the image, invalid or out of range -- so the one
// comparison fabsf(z_q - z_p) <= tol decides support, NaN comparing false.
// The LDS image: row y of the tile at row y + kHaloMax, column x at word kTileCol0 + x of the row, so that a lane's own run, the
// run to its left and the run to its right are three aligned 16-byte reads.  The row pitch is 128 words, a multiple of the 64 banks:
// a 16-byte read's lane groups ({0-3, 12-15, 20-27}, ...) then take 64 consecutive words of two rows at the same columns modulo
// 64 -- words 0..15 and 48..63 of one row, 16..47 of the next -- which are 64 distinct banks ("Depth filter").
constexpr int kTileW = 64, kTileH = 16;
constexpr int kHaloMax = 2;      // the largest radius
constexpr int kTileCol0 = 4;     // the word of tile column 0 in an LDS row: the left halo lies in the run before it
constexpr int kTilePitch = 128;  // words
constexpr int kTileRows = kTileH + 2 * kHaloMax;
constexpr int kFilterCounters = 4;  // agh_depth_filter_counts: n_valid, n_out_of_range, n_unsupported, n_kept
static_assert(kTileW * kTileH == kRun * kDeprojBlock && kTileW == 16 * kRun, "a lane's run is one of its tile's");
static_assert(kTileCol0 + kTileW + kRun <= kTilePitch && kTileCol0 >= kHaloMax && kRun >= kHaloMax, "the three reads stay in the row");

typedef __attribute__((address_space(3))) F32x4 LdsF32x4;

struct DepthFilterArgs
{
  int32_t radius, min_support;
  float ja, jr, zlo, zhi;
};

// The depths of the run at row v, columns u0.. of `im`, by deproject_run's loads and its arithmetic: z[j] and the format's
// validity.  A run (or its tail) outside the image is invalid and is not read.
__device__ __forceinline__ void filter_load_run(const DepthView& im, int v, int u0, float z[kRun], bool ok[kRun])
{
#pragma unroll
  for (int j = 0; j < kRun; j++)
  {
    z[j] = 0.0f;
    ok[j] = false;
  }
  if (v < 0 || v >= im.h || u0 < 0 || u0 >= im.w)
    return;
  const int cnt = min(kRun, im.w - u0);
  const GlobalBytes* row = (const GlobalBytes*) im.data + (int64_t) v * im.stride;
  if (im.fmt == AGH_DEPTH_U16)
  {
    const __attribute__((address_space(1))) uint16_t* p = (const __attribute__((address_space(1))) uint16_t*) row + u0;
    uint32_t raw[kRun] = { 0, 0, 0, 0 };
    if (cnt == kRun && ((uintptr_t) p & 7) == 0)
    {
      const U32x2 q = *(const __attribute__((address_space(1))) U32x2*) p;
      raw[0] = q.x & 0xffffu;
      raw[1] = q.x >> 16;
      raw[2] = q.y & 0xffffu;
      raw[3] = q.y >> 16;
    }
    else
    {
#pragma unroll
      for (int j = 0; j < kRun; j++)
        if (j < cnt)
          raw[j] = p[j];
    }
#pragma unroll
    for (int j = 0; j < kRun; j++)
    {
      z[j] = (float) raw[j] * im.scale;
      ok[j] = raw[j] != 0;
    }
  }
  else
  {
    const __attribute__((address_space(1))) float* p = (const __attribute__((address_space(1))) float*) row + u0;
    if (cnt == kRun && ((uintptr_t) p & 15) == 0)
    {
      const F32x4 q = *(const __attribute__((address_space(1))) F32x4*) p;
      z[0] = q.x;
      z[1] = q.y;
      z[2] = q.z;
      z[3] = q.w;
    }
    else
    {
#pragma unroll
      for (int j = 0; j < kRun; j++)
        z[j] = j < cnt ? p[j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kRun; j++)
      ok[j] = z[j] > 0.0f && z[j] < __builtin_huge_valf();
  }
}

// one pixel of the halo's side columns: its depth if it is inside the image, valid and in range, else NaN
__device__ __forceinline__ float filter_load_pixel(const DepthView& im, int v, int u, const DepthFilterArgs& f)
{
  const float qnan = __builtin_nanf("");
  if (v < 0 || v >= im.h || u < 0 || u >= im.w)
    return qnan;
  const GlobalBytes* row = (const GlobalBytes*) im.data + (int64_t) v * im.stride;
  float z;
  bool ok;
  if (im.fmt == AGH_DEPTH_U16)
  {
    const uint32_t raw = ((const __attribute__((address_space(1))) uint16_t*) row)[u];
    z = (float) raw * im.scale;
    ok = raw != 0;
  }
  else
  {
    z = ((const __attribute__((address_space(1))) float*) row)[u];
    ok = z > 0.0f && z < __builtin_huge_valf();
  }
  return ok && z >= f.zlo && z <= f.zhi ? z : qnan;
}

// Tile `tile` of `im` (tiles row-major, ceil(w / kTileW) per row): the one copy of the body, k_deproject_filtered's and
// k_deproject_filtered_batch's, for radius R.  Every lane reaches both barriers; lanes whose run lies outside the image stage NaNs
// and write nothing.  cnt: the view's four counters.
template <int R>
__device__ __forceinline__ void deproject_filtered_tile(const DepthView& im, uint32_t tile, const DepthFilterArgs& f,
  float* __restrict__ out, unsigned long long* __restrict__ cnt, float* s_z, unsigned* s_cnt)
{
  const float qnan = __builtin_nanf("");
  const int tiles_x = (im.w + kTileW - 1) / kTileW;
  const int ty = (int) (tile / (uint32_t) tiles_x);
  const int x0 = (int) (tile - (uint32_t) ty * (uint32_t) tiles_x) * kTileW, y0 = ty * kTileH;
  const int t = threadIdx.x;
  const int r = t >> 4, cg = t & 15;
  const int v = y0 + r, u0 = x0 + kRun * cg;
  // ---- 1. the lane's own run, and one piece of the halo: a run of the rows above and below (lanes 0 .. 32 R - 1), or one pixel of
  // the columns left and right of the tile and of the halo's corners (the next (kTileH + 2 R) x 2 R lanes) ----
  float z[kRun];
  bool valid[kRun], inr[kRun];
  filter_load_run(im, v, u0, z, valid);
  {
    float zs[kRun];
#pragma unroll
    for (int j = 0; j < kRun; j++)
    {
      inr[j] = valid[j] && z[j] >= f.zlo && z[j] <= f.zhi;
      zs[j] = inr[j] ? z[j] : qnan;
    }
    *reinterpret_cast<float4*>(&s_z[(r + kHaloMax) * kTilePitch + kTileCol0 + kRun * cg]) = make_float4(zs[0], zs[1], zs[2], zs[3]);
  }
  constexpr int kRowRuns = 2 * R * (kTileW / kRun);
  constexpr int kSidePixels = (kTileH + 2 * R) * 2 * R;
  static_assert(kRowRuns + kSidePixels <= kDeprojBlock, "one halo piece per lane");
  if (t < kRowRuns)
  {
    const int j = t >> 4;
    const int yoff = j < R ? j - R : kTileH + (j - R);
    float hz[kRun];
    bool hok[kRun];
    filter_load_run(im, y0 + yoff, u0, hz, hok);
#pragma unroll
    for (int q = 0; q < kRun; q++)
      hz[q] = hok[q] && hz[q] >= f.zlo && hz[q] <= f.zhi ? hz[q] : qnan;
    *reinterpret_cast<float4*>(&s_z[(yoff + kHaloMax) * kTilePitch + kTileCol0 + kRun * cg]) = make_float4(hz[0], hz[1], hz[2], hz[3]);
  }
  else if (t < kRowRuns + kSidePixels)
  {
    const int s = t - kRowRuns;
    const int yoff = s / (2 * R) - R;
    const int k = s % (2 * R);
    const int xoff = k < R ? k - R : kTileW + (k - R);
    s_z[(yoff + kHaloMax) * kTilePitch + kTileCol0 + xoff] = filter_load_pixel(im, y0 + yoff, x0 + xoff, f);
  }
  __syncthreads();
  // ---- 2. support, counted on the in-range set: per window row the run to the left, the lane's own and the run to the right ----
  float tol[kRun];
  int sup[kRun];
#pragma unroll
  for (int j = 0; j < kRun; j++)
  {
    tol[j] = f.ja + (f.jr * z[j]);
    sup[j] = 0;
  }
#pragma unroll
  for (int dy = -R; dy <= R; dy++)
  {
    // (volatile: three whole 16-byte reads, conflict-free at this pitch; left to itself the compiler reads only the words the
    // radius needs, with 4-byte pairs whose lanes share banks)
    const volatile LdsF32x4* rp = (const volatile LdsF32x4*) &s_z[(r + kHaloMax + dy) * kTilePitch + kRun * cg];
    const F32x4 a = rp[0], b = rp[1], c = rp[2];
    const float w[3 * kRun] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
#pragma unroll
    for (int j = 0; j < kRun; j++)
#pragma unroll
      for (int dx = -R; dx <= R; dx++)
        if (dy != 0 || dx != 0)
          sup[j] += fabsf(w[kRun + j + dx] - z[j]) <= tol[j] ? 1 : 0;
  }
  bool keep[kRun];
#pragma unroll
  for (int j = 0; j < kRun; j++)
    keep[j] = inr[j] && sup[j] >= f.min_support;
  // ---- 3. the points, deproject_run's expression and stores ----
  if (v < im.h && u0 < im.w)
  {
    const int cntp = min(kRun, im.w - u0);
    const float fv = (float) v;
    float o[3 * kRun];
#pragma unroll
    for (int j = 0; j < kRun; j++)
    {
      const float x = (((float) (u0 + j) - im.cx) * z[j]) * im.kx;
      const float y = ((fv - im.cy) * z[j]) * im.ky;
      o[3 * j + 0] = keep[j] ? ((im.p[0] * x + im.p[1] * y) + im.p[2] * z[j]) + im.p[3] : qnan;
      o[3 * j + 1] = keep[j] ? ((im.p[4] * x + im.p[5] * y) + im.p[6] * z[j]) + im.p[7] : qnan;
      o[3 * j + 2] = keep[j] ? ((im.p[8] * x + im.p[9] * y) + im.p[10] * z[j]) + im.p[11] : qnan;
    }
    const int64_t idx = im.base + (int64_t) v * im.w + u0;
    float* dst = out + 3 * idx;
    if (cntp == kRun && (idx & 3) == 0)
    {
      float4* d4 = reinterpret_cast<float4*>(dst);
      d4[0] = make_float4(o[0], o[1], o[2], o[3]);
      d4[1] = make_float4(o[4], o[5], o[6], o[7]);
      d4[2] = make_float4(o[8], o[9], o[10], o[11]);
    }
    else
    {
#pragma unroll
      for (int j = 0; j < kRun; j++)
        if (j < cntp)
        {
          dst[3 * j + 0] = o[3 * j + 0];
          dst[3 * j + 1] = o[3 * j + 1];
          dst[3 * j + 2] = o[3 * j + 2];
        }
    }
  }
  // ---- 4. the view's counters: ballots per wave, the waves' sums through LDS, one atomic per counter and work-group ----
  unsigned n[kFilterCounters] = { 0, 0, 0, 0 };
#pragma unroll
  for (int j = 0; j < kRun; j++)
  {
    n[0] += (unsigned) __popcll(__ballot(valid[j]));
    n[1] += (unsigned) __popcll(__ballot(valid[j] && !inr[j]));
    n[2] += (unsigned) __popcll(__ballot(inr[j] && !keep[j]));
    n[3] += (unsigned) __popcll(__ballot(keep[j]));
  }
  if ((t & 63) == 0)
  {
#pragma unroll
    for (int q = 0; q < kFilterCounters; q++)
      s_cnt[(t >> 6) * kFilterCounters + q] = n[q];
  }
  __syncthreads();
  if (t < kFilterCounters)
    atomicAdd(&cnt[t], (unsigned long long) (s_cnt[t] + s_cnt[kFilterCounters + t] + s_cnt[2 * kFilterCounters + t] + s_cnt[3 * kFilterCounters + t]));
}

__device__ __forceinline__ void deproject_filtered(const DepthView& im, uint32_t tile, const DepthFilterArgs& f, float* __restrict__ out,
  unsigned long long* __restrict__ cnt)
{
  __shared__ __attribute__((aligned(16))) float s_z[kTileRows * kTilePitch];
  __shared__ unsigned s_cnt[(kDeprojBlock / 64) * kFilterCounters];
  if (f.radius == 1)
    deproject_filtered_tile<1>(im, tile, f, out, cnt, s_z, s_cnt);
  else
    deproject_filtered_tile<2>(im, tile, f, out, cnt, s_z, s_cnt);
}

extern "C" __global__ __launch_bounds__(kDeprojBlock) void k_deproject_filtered(DepthArgs a, int n_images, DepthFilterArgs f,
  float* __restrict__ out, unsigned long long* __restrict__ counts)
{
  const int k = (n_images > 1 && blockIdx.x >= a.v[1].first_block) ? 1 : 0;
  const DepthView& im = a.v[k];
  deproject_filtered(im, blockIdx.x - im.first_block, f, out, counts + kFilterCounters * k);
}

// (the views as k_deproject_batch finds them; counts: kFilterCounters per view, in launch order)
extern "C" __global__ __launch_bounds__(kDeprojBlock) void k_deproject_filtered_batch(const DepthView* __restrict__ views, int n_views,
  DepthFilterArgs f, float* __restrict__ out, unsigned long long* __restrict__ counts)
{
  int lo = 0, hi = n_views - 1;
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (views[mid].first_block <= blockIdx.x)
      lo = mid;
    else
      hi = mid - 1;
  }
  const DepthView& im = views[lo];
  deproject_filtered(im, blockIdx.x - im.first_block, f, out, counts + kFilterCounters * lo);
}

inline int64_t elem_size(int32_t format) { return format == AGH_DEPTH_U16 ? 2 : 4; }
inline int64_t packed_bytes(const agh_depth_image& im) { return (int64_t) im.width * im.height * elem_size(im.format); }
// where image k's packed rows start in a depth buffer of the context: the images of a capture (or of a whole batch, in capture
// order) one after the other, each at a 256-byte boundary (the wide loads hold whenever the width does)
inline int64_t aligned_bytes(const agh_depth_image& im) { return (packed_bytes(im) + 255) / 256 * 256; }
inline int64_t depth_image_offset(const agh_depth_image* im, int k)
{
  int64_t off = 0;
  for (int j = 0; j < k; j++)
    off += aligned_bytes(im[j]);
  return off;
}
inline int64_t depth_buffer_bytes(const agh_depth_image* im, int n) { return depth_image_offset(im, n - 1) + packed_bytes(im[n - 1]); }

// host images into a depth buffer, rows packed (what was staged before stays ahead of these copies on its stream)
hipError_t upload_images(uint8_t* dst, const agh_depth_image* im, int n, hipStream_t st)
{
  int64_t off = 0;
  for (int k = 0; k < n; off += aligned_bytes(im[k]), k++)
  {
    const size_t row = (size_t) im[k].width * (size_t) elem_size(im[k].format);
    uint8_t* d = dst + off;
    const hipError_t e = (size_t) im[k].row_stride_bytes == row
      ? hipMemcpyAsync(d, im[k].data, row * (size_t) im[k].height, hipMemcpyHostToDevice, st)
      : hipMemcpy2DAsync(d, row, im[k].data, (size_t) im[k].row_stride_bytes, row, (size_t) im[k].height, hipMemcpyHostToDevice, st);
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

// image `im` as k_deproject reads it: rows at `data` with `stride` bytes, its first point at `base`, its blocks from first_block on
DepthView make_view(const agh_depth_image& im, const uint8_t* data, int64_t stride, int64_t base, uint32_t first_block)
{
  DepthView v;
  std::memset(&v, 0, sizeof(v));
  v.data = data;
  v.stride = stride;
  v.base = base;
  v.w = im.width;
  v.h = im.height;
  v.fmt = im.format;
  v.runs = (im.width + kRun - 1) / kRun;
  v.first_block = first_block;
  v.scale = im.depth_scale;
  v.kx = (float) (1.0 / im.fx);
  v.ky = (float) (1.0 / im.fy);
  v.cx = (float) im.cx;
  v.cy = (float) im.cy;
  for (int q = 0; q < 12; q++)
    v.p[q] = (float) im.pose[q];
  return v;
}
inline uint32_t view_blocks(const DepthView& v) { return (uint32_t) (((int64_t) v.runs * v.h + kDeprojBlock - 1) / kDeprojBlock); }
// ... and as the filtered kernels count them: first_block and the launch in tiles
inline uint32_t view_tiles(const DepthView& v) { return (uint32_t) ((v.w + kTileW - 1) / kTileW) * (uint32_t) ((v.h + kTileH - 1) / kTileH); }

// the filter held by the context as the kernels take it: the four doubles rounded once to float32
DepthFilterArgs filter_args(const Ctx* c)
{
  DepthFilterArgs f;
  f.radius = c->depth_filter.radius;
  f.min_support = c->depth_filter.min_support;
  f.ja = (float) c->depth_filter.max_jump_abs;
  f.jr = (float) c->depth_filter.max_jump_rel;
  f.zlo = (float) c->depth_filter.z_min;
  f.zhi = (float) c->depth_filter.z_max;
  return f;
}

// the per-view counters of the filtered launch that follows on `st`, zeroed in front of it
int filter_counts_for(Ctx* c, int views, hipStream_t st)
{
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are read back as int64_t");
  if (!c->d_filter_counts)
    if (int rc = dev_alloc(c, &c->d_filter_counts, (size_t) kMaxDepthViews * kFilterCounters))
      return rc;
  AGH_HIPCHK(c, hipMemsetAsync(c->d_filter_counts, 0, sizeof(int64_t) * kFilterCounters * (size_t) views, st));
  return AGH_OK;
}

// the raw buffer for `total` points, and `st` behind the last batch chain that read it (as stage_captures waits, localize.hip)
int raw_buffer_for(Ctx* c, int64_t total, hipStream_t st)
{
  if (3 * total > c->raw_cap || !c->d_raw_xyz)
  {
    if (int rc = dev_alloc(c, &c->d_raw_xyz, (size_t) (3 * total)))
      return rc;
    c->raw_cap = 3 * total;
    c->raw_read_set = false;
  }
  if (c->raw_read_set)
    AGH_HIPCHK(c, hipStreamWaitEvent(st, c->raw_read, 0));
  return AGH_OK;
}

// behind the last reader of the context's depth buffers: a later agh_localize_depth_stage overwrites one of them
int record_depth_read(Ctx* c, hipStream_t st)
{
  if (!c->depth_read)
    AGH_HIPCHK(c, hipEventCreateWithFlags(&c->depth_read, hipEventDisableTiming));
  AGH_HIPCHK(c, hipEventRecord(c->depth_read, st));
  return AGH_OK;
}

int ensure_depth_buffer(Ctx* c, uint8_t** buf, int64_t* cap, int64_t need)
{
  if (need <= *cap && *buf)
    return AGH_OK;
  if (int rc = dev_alloc(c, buf, (size_t) need))
  {
    *cap = 0;
    return rc;
  }
  *cap = need;
  return AGH_OK;
}

// depth_check's rules for ONE image: the text of the first rule broken, without a prefix, or an empty string (agh_fuse_depth's
// frames are checked with it too, under their own names)
std::string depth_image_fault(const agh_depth_image& im, bool on_device)
{
  if (!im.data)
    return "data is NULL";
  if (im.width < 1 || im.width > 8192)
    return "width must be 1..8192";
  if (im.height < 1 || im.height > 8192)
    return "height must be 1..8192";
  if (im.format != AGH_DEPTH_U16 && im.format != AGH_DEPTH_F32)
    return "format must be AGH_DEPTH_U16 or AGH_DEPTH_F32";
  const int64_t es = elem_size(im.format);
  // (a host image is repacked by its copy; a device image is read in place, an element at a time at the least)
  if (on_device && reinterpret_cast<uintptr_t>(im.data) % (uintptr_t) es != 0)
    return "data (a device pointer) must be aligned to the element size";
  if (im.row_stride_bytes < im.width * es || im.row_stride_bytes % es != 0)
    return "row_stride_bytes must be at least width x element size and a multiple of the element size";
  if (!std::isfinite(im.fx) || im.fx == 0.0)
    return "fx must be finite and not zero";
  if (!std::isfinite(im.fy) || im.fy == 0.0)
    return "fy must be finite and not zero";
  if (!std::isfinite(im.cx))
    return "cx must be finite";
  if (!std::isfinite(im.cy))
    return "cy must be finite";
  for (int q = 0; q < 12; q++)
    if (!std::isfinite(im.pose[q]))
      return "pose[" + std::to_string(q) + "] must be finite";
  if (im.format == AGH_DEPTH_U16 && !(std::isfinite(im.depth_scale) && im.depth_scale > 0.0f))
    return "depth_scale must be finite and positive";
  return std::string();
}

void swap_depth_buffers(Ctx* c)
{
  std::swap(c->d_depth, c->d_depth_stage);
  std::swap(c->depth_cap, c->depth_stage_cap);
}
}  // namespace

int depth_check(Ctx* c, const char* who, const agh_depth_image* images, int32_t n_images, bool on_device, int64_t* n_points, int capture)
{
  auto bad = [&](const std::string& what) {
    c->err = std::string(who) + ": " + what;
    return AGH_ERR_INVALID_ARGUMENT;
  };
  if (!images)
    return bad("images is NULL");
  const std::string cap = capture >= 0 ? "capture " + std::to_string(capture) : std::string();
  if (n_images != 1 && n_images != 2)
    return bad((capture >= 0 ? cap + ": " : cap) + "n_images must be 1 or 2");
  int64_t total = 0;
  for (int k = 0; k < n_images; k++)
  {
    const agh_depth_image& im = images[k];
    const std::string at = (capture >= 0 ? cap + ", " : cap) + "image " + std::to_string(k) + ": ";
    const std::string fault = depth_image_fault(im, on_device);
    if (!fault.empty())
      return bad(at + fault);
    total += (int64_t) im.width * im.height;
  }
  if (n_points)
    *n_points = total;
  return AGH_OK;
}

int depth_to_raw(agh_ctx* ctx, const char* who, const agh_depth_image* images, int n_images, bool on_device, bool use_staged,
  hipStream_t st)
{
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  int rc;
  if (!on_device)
  {
    if (use_staged && L.staged_depth_is(images, n_images) && c->d_depth_stage)
    {
      // the images are (or are about to be) in the second depth buffer: the two change places, the chain waits for the copy
      swap_depth_buffers(c);
      L.staged = false;
      AGH_HIPCHK(c, hipStreamWaitEvent(st, c->stage_done, 0));
    }
    else
    {
      if (use_staged)
      {
        // (a staged set of any kind that is not this capture is dropped; the chain waits for its copy, as agh_localize_begin does)
        if (L.staged)
          AGH_HIPCHK(c, hipStreamWaitEvent(st, c->stage_done, 0));
        L.staged = false;
      }
      if ((rc = ensure_depth_buffer(c, &c->d_depth, &c->depth_cap, depth_buffer_bytes(images, n_images))))
        return rc;
      AGH_HIPCHK(c, upload_images(c->d_depth, images, n_images, st));
    }
  }
  int64_t total = 0;
  for (int k = 0; k < n_images; k++)
    total += (int64_t) images[k].width * images[k].height;
  if ((rc = raw_buffer_for(c, total, st)))
    return rc;
  const bool filtered = c->depth_filter_set;
  c->filter_views = 0;  // (agh_get_depth_filter_counts: the views of the last deprojection, if it ran with a filter)
  DepthArgs a;
  std::memset(&a, 0, sizeof(a));
  int64_t base = 0;
  uint32_t blocks = 0;
  for (int k = 0; k < n_images; k++)
  {
    const agh_depth_image& im = images[k];
    a.v[k] = on_device ? make_view(im, static_cast<const uint8_t*>(im.data), im.row_stride_bytes, base, blocks)
                       : make_view(im, c->d_depth + depth_image_offset(images, k), (int64_t) im.width * elem_size(im.format), base, blocks);
    base += (int64_t) im.width * im.height;
    blocks += filtered ? view_tiles(a.v[k]) : view_blocks(a.v[k]);
  }
  {
    // (agh_set_hand_filter's observed-space criterion reads the same bytes behind the search: they stay until the chain ends)
    const uint8_t* data[2] = { a.v[0].data, a.v[1].data };
    const int64_t stride[2] = { a.v[0].stride, a.v[1].stride };
    const int32_t count = n_images;
    hand_filter_keep_views(c, images, &count, 1, data, stride);
  }
  if (filtered)
  {
    if ((rc = filter_counts_for(c, n_images, st)))
      return rc;
    hipLaunchKernelGGL(k_deproject_filtered, dim3(blocks), dim3(kDeprojBlock), 0, st, a, n_images, filter_args(c), c->d_raw_xyz,
      reinterpret_cast<unsigned long long*>(c->d_filter_counts));
    if (hipGetLastError() != hipSuccess)
    {
      c->err = std::string(who) + ": k_deproject_filtered launch failed";
      return AGH_ERR_HIP;
    }
    c->filter_views = n_images;
    c->filter_stream = st;
    if (!on_device)
      return record_depth_read(c, st);
    return AGH_OK;
  }
  hipLaunchKernelGGL(k_deproject, dim3(blocks), dim3(kDeprojBlock), 0, st, a, n_images, c->d_raw_xyz);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = std::string(who) + ": k_deproject launch failed";
    return AGH_ERR_HIP;
  }
  if (!on_device)
    return record_depth_read(c, st);
  return AGH_OK;
}

int depth_batch_check(Ctx* c, const char* who, const agh_depth_image* images, const int32_t* n_images, int32_t C, bool on_device,
  std::vector<int64_t>* first, std::vector<int64_t>* left0)
{
  auto bad = [&](const std::string& what) {
    c->err = std::string(who) + ": " + what;
    return AGH_ERR_INVALID_ARGUMENT;
  };
  if (C < 1 || C > kMaxClouds)
    return bad("n_captures must be 1..64");
  if (!images || !n_images)
    return bad("images or n_images is NULL");
  for (int k = 0; k < C; k++)
    if (n_images[k] != 1 && n_images[k] != 2)
      return bad("capture " + std::to_string(k) + ": n_images must be 1 or 2");
  first->assign((size_t) C + 1, 0);
  left0->assign((size_t) C, 0);
  const agh_depth_image* im = images;
  for (int k = 0; k < C; im += n_images[k], k++)
  {
    int64_t n = 0;
    if (int rc = depth_check(c, who, im, n_images[k], on_device, &n, k))
      return rc;
    (*first)[k + 1] = (*first)[k] + n;
    (*left0)[k] = (int64_t) im[0].width * im[0].height;
  }
  if ((*first)[C] >= (1ll << 30))
    return bad("need fewer than 2^30 points in all");
  return AGH_OK;
}

int depth_batch_to_raw(agh_ctx* ctx, const char* who, const agh_depth_image* images, const int32_t* n_images, int C, bool on_device,
  bool drop_staged, hipStream_t st)
{
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  static_assert(sizeof(DepthView) % 8 == 0, "the table's records are read with scalar loads");
  auto fail = [c, st](int code) {
    (void) hipStreamSynchronize(st);
    return code;
  };
  int rc;
  int views = 0;
  for (int k = 0; k < C; k++)
    views += n_images[k];
  if (!c->d_depth_views)
  {
    void* pin = nullptr;
    if ((rc = dev_alloc(c, &c->d_depth_views, sizeof(DepthView) * (size_t) kMaxDepthViews)))
      return rc;
    AGH_HIPCHK(c, hipHostMalloc(&pin, sizeof(DepthView) * (size_t) kMaxDepthViews, hipHostMallocDefault));
    c->h_depth_views = static_cast<uint8_t*>(pin);
  }
  if (!on_device)
  {
    if (drop_staged)
    {
      // (a staged set of any kind is dropped; the chain waits for its copy, as every begin that does not adopt it does)
      if (L.staged)
        AGH_HIPCHK(c, hipStreamWaitEvent(st, c->stage_done, 0));
      L.staged = false;
    }
    if ((rc = ensure_depth_buffer(c, &c->d_depth, &c->depth_cap, depth_buffer_bytes(images, views))))
      return rc;
    AGH_HIPCHK_OR(c, upload_images(c->d_depth, images, views, st), fail(AGH_ERR_HIP));
  }
  const bool filtered = c->depth_filter_set;
  c->filter_views = 0;
  DepthView* tab = reinterpret_cast<DepthView*>(c->h_depth_views);
  int64_t base = 0, off = 0;
  uint32_t blocks = 0;
  for (int j = 0; j < views; j++)
  {
    const agh_depth_image& im = images[j];
    tab[j] = on_device ? make_view(im, static_cast<const uint8_t*>(im.data), im.row_stride_bytes, base, blocks)
                       : make_view(im, c->d_depth + off, (int64_t) im.width * elem_size(im.format), base, blocks);
    base += (int64_t) im.width * im.height;
    off += aligned_bytes(im);
    blocks += filtered ? view_tiles(tab[j]) : view_blocks(tab[j]);
  }
  {
    // (agh_set_hand_filter's observed-space criterion reads the same bytes behind the search: they stay until the chain ends)
    std::vector<const uint8_t*> data((size_t) views);
    std::vector<int64_t> stride((size_t) views);
    for (int j = 0; j < views; j++)
    {
      data[(size_t) j] = tab[j].data;
      stride[(size_t) j] = tab[j].stride;
    }
    hand_filter_keep_views(c, images, n_images, C, data.data(), stride.data());
  }
  if ((rc = raw_buffer_for(c, base, st)))
    return fail(rc);
  AGH_HIPCHK_OR(c, hipMemcpyAsync(c->d_depth_views, tab, sizeof(DepthView) * (size_t) views, hipMemcpyHostToDevice, st), fail(AGH_ERR_HIP));
  if (filtered)
  {
    if ((rc = filter_counts_for(c, views, st)))
      return fail(rc);
    hipLaunchKernelGGL(k_deproject_filtered_batch, dim3(blocks), dim3(kDeprojBlock), 0, st,
      reinterpret_cast<const DepthView*>(c->d_depth_views), views, filter_args(c), c->d_raw_xyz,
      reinterpret_cast<unsigned long long*>(c->d_filter_counts));
    if (hipGetLastError() != hipSuccess)
    {
      c->err = std::string(who) + ": k_deproject_filtered_batch launch failed";
      return fail(AGH_ERR_HIP);
    }
    c->filter_views = views;
    c->filter_stream = st;
    if (!on_device && (rc = record_depth_read(c, st)))
      return fail(rc);
    return AGH_OK;
  }
  hipLaunchKernelGGL(k_deproject_batch, dim3(blocks), dim3(kDeprojBlock), 0, st, reinterpret_cast<const DepthView*>(c->d_depth_views),
    views, c->d_raw_xyz);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = std::string(who) + ": k_deproject_batch launch failed";
    return fail(AGH_ERR_HIP);
  }
  if (!on_device && (rc = record_depth_read(c, st)))
    return fail(rc);
  return AGH_OK;
}

extern "C" {

// ---- the depth filter's setting (include/agh.h): host-side, the parameters travel as kernel arguments ----
void agh_default_depth_filter_params(agh_depth_filter_params* p)
{
  if (!p)
    return;
  p->radius = 1;
  p->min_support = 3;
  p->max_jump_abs = 0.01;
  p->max_jump_rel = 0.01;
  p->z_min = 0.0;
  p->z_max = std::numeric_limits<double>::infinity();
}

int agh_set_depth_filter(agh_ctx* ctx, const agh_depth_filter_params* fp)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_set_depth_filter"))
    return AGH_ERR_STATE;
  if (!fp)
  {
    c->depth_filter_set = false;
    return AGH_OK;
  }
  auto bad = [c](const char* what) {
    c->err = std::string("agh_set_depth_filter: ") + what;
    return AGH_ERR_INVALID_ARGUMENT;
  };
  if (fp->radius != 1 && fp->radius != 2)
    return bad("radius must be 1 or 2");
  const int window = (2 * fp->radius + 1) * (2 * fp->radius + 1);
  if (fp->min_support < 1 || fp->min_support > window - 1)
    return bad("min_support must be 1 .. (2 radius + 1)^2 - 1");
  if (!(std::isfinite(fp->max_jump_abs) && fp->max_jump_abs >= 0.0))
    return bad("max_jump_abs must be finite and >= 0");
  if (!(std::isfinite(fp->max_jump_rel) && fp->max_jump_rel >= 0.0))
    return bad("max_jump_rel must be finite and >= 0");
  if (!(std::isfinite(fp->z_min) && fp->z_min >= 0.0))
    return bad("z_min must be finite and >= 0");
  if (!(fp->z_max > fp->z_min))  // (a NaN fails; +inf passes)
    return bad("z_max must be greater than z_min");
  c->depth_filter = *fp;
  c->depth_filter_set = true;
  return AGH_OK;
}

int agh_get_depth_filter(agh_ctx* ctx, agh_depth_filter_params* out)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;  // (host-side: allowed while a localize chain is in flight)
  if (!c->depth_filter_set)
    return 0;
  if (!out)
  {
    c->err = "agh_get_depth_filter: out is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  *out = c->depth_filter;
  return 1;
}

int agh_get_depth_filter_counts(agh_ctx* ctx, agh_depth_filter_counts* out, int32_t cap_views)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_depth_filter_counts"))
    return AGH_ERR_STATE;
  if (c->filter_views == 0)
    return 0;
  if (cap_views < c->filter_views || !out)
  {
    c->err = "agh_get_depth_filter_counts: room for " + std::to_string(c->filter_views) + " views is needed";
    return AGH_ERR_CAPACITY;
  }
  static_assert(sizeof(agh_depth_filter_counts) == sizeof(int64_t) * kFilterCounters, "a view's record is its four counters");
  AGH_HIPCHK(c, hipSetDevice(c->device));
  AGH_HIPCHK_OR(c, hipMemcpyAsync(out, c->d_filter_counts, sizeof(agh_depth_filter_counts) * (size_t) c->filter_views, hipMemcpyDeviceToHost,
    c->filter_stream), ((void) hipStreamSynchronize(c->filter_stream), AGH_ERR_HIP));
  AGH_HIPCHK(c, hipStreamSynchronize(c->filter_stream));
  return c->filter_views;
}

int agh_deproject(agh_ctx* ctx,const agh_depth_image* images, int32_t n_images, float* xyz_out, int64_t cap_points)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_deproject"))
    return AGH_ERR_STATE;
  if (c->batch_active)
  {
    c->err = "agh_deproject: an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  int64_t total = 0;
  if (int rc = depth_check(c, "agh_deproject", images, n_images, false, &total))
    return rc;
  if (cap_points < 0 || (cap_points > 0 && !xyz_out))
  {
    c->err = "agh_deproject: xyz_out is NULL or cap_points negative";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (total > cap_points)
  {
    c->err = "agh_deproject: xyz_out holds fewer than the images' " + std::to_string(total) + " points";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  // (a staged set is left alone: it lies in the other depth buffer, or in the points' second raw buffer)
  if (int rc = depth_to_raw(ctx, "agh_deproject", images, n_images, false, false, c->stream))
  {
    (void) hipStreamSynchronize(c->stream);
    return rc;
  }
  AGH_HIPCHK_OR(c, hipMemcpyAsync(xyz_out, c->d_raw_xyz, sizeof(float) * 3 * (size_t) total, hipMemcpyDeviceToHost, c->stream),
    ((void) hipStreamSynchronize(c->stream), AGH_ERR_HIP));
  AGH_HIPCHK(c, hipStreamSynchronize(c->stream));
  return (int) total;
}

// agh_deproject for a batch: the points k_deproject_batch makes of every capture's images, capture after capture.
int agh_deproject_batch(agh_ctx* ctx, const agh_depth_image* images, const int32_t* n_images, int32_t n_captures, float* xyz_out,
  int64_t cap_points)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_deproject_batch"))
    return AGH_ERR_STATE;
  if (c->batch_active)
  {
    c->err = "agh_deproject_batch: an agh_localize_batch is running on this context";
    return AGH_ERR_STATE;
  }
  std::vector<int64_t> first, left0;
  if (int rc = depth_batch_check(c, "agh_deproject_batch", images, n_images, n_captures, false, &first, &left0))
    return rc;
  const int64_t total = first[n_captures];
  if (cap_points < 0 || (cap_points > 0 && !xyz_out))
  {
    c->err = "agh_deproject_batch: xyz_out is NULL or cap_points negative";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (total > cap_points)
  {
    c->err = "agh_deproject_batch: xyz_out holds fewer than the images' " + std::to_string(total) + " points";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  // (a staged set is left alone, as by agh_deproject)
  if (int rc = depth_batch_to_raw(ctx, "agh_deproject_batch", images, n_images, n_captures, false, false, c->stream))
    return rc;
  AGH_HIPCHK_OR(c, hipMemcpyAsync(xyz_out, c->d_raw_xyz, sizeof(float) * 3 * (size_t) total, hipMemcpyDeviceToHost, c->stream),
    ((void) hipStreamSynchronize(c->stream), AGH_ERR_HIP));
  AGH_HIPCHK(c, hipStreamSynchronize(c->stream));
  return (int) total;
}

// The NEXT capture's images up, beside whatever runs on the context's stream: rows packed, into the second depth buffer, on the
// stage stream (stage_captures' rules, localize.hip: a pageable source has been read when the call returns).
int agh_localize_depth_stage(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  LocalizeState& L = c->loc;
  if (int rc = depth_check(c, "agh_localize_depth_stage", images, n_images, false, nullptr))
    return rc;
  AGH_HIPCHK(c, hipSetDevice(c->device));
  if (int rc = ensure_stage_stream(c, "agh_localize_depth_stage"))
    return rc;
  auto stage_fail = [c](int code) {
    (void) hipStreamSynchronize(c->stage_stream);
    c->loc.staged = false;
    return code;
  };
  // (the chain in flight reads d_depth; d_depth_stage's last reader, if any, is behind depth_read)
  if (int rc = ensure_depth_buffer(c, &c->d_depth_stage, &c->depth_stage_cap, depth_buffer_bytes(images, n_images)))
    return stage_fail(rc);
  if (c->depth_read)
    AGH_HIPCHK_OR(c, hipStreamWaitEvent(c->stage_stream, c->depth_read, 0), stage_fail(AGH_ERR_HIP));
  AGH_HIPCHK_OR(c, upload_images(c->d_depth_stage, images, n_images, c->stage_stream), stage_fail(AGH_ERR_HIP));
  AGH_HIPCHK_OR(c, hipEventRecord(c->stage_done, c->stage_stream), stage_fail(AGH_ERR_HIP));
  L.staged_images.assign(images, images + n_images);
  L.staged_depth = true;
  L.staged = true;
  return AGH_OK;
}

}  // extern "C"

// agh_fuse_depth and k_depth_fuse: part of this translation unit (the per-image rules and the packing of host images are shared)
#include "depth_fuse.hip"
