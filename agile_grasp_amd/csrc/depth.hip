// depth.hip -- the localize chain's third source kind (include/agh.h, agh_localize_depth*): a capture as the sensor's driver hands it
// over, one depth image per camera, back-projected on the device into the raw buffer an upload of points would have filled.
// k_deproject and its launch, the argument rules, the context's two depth buffers (this capture's images and the staged next
// ones), agh_deproject and agh_localize_depth_stage; the chain itself is localize.hip's.
#include "agh_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

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
    if (!im.data)
      return bad(at + "data is NULL");
    if (im.width < 1 || im.width > 8192)
      return bad(at + "width must be 1..8192");
    if (im.height < 1 || im.height > 8192)
      return bad(at + "height must be 1..8192");
    if (im.format != AGH_DEPTH_U16 && im.format != AGH_DEPTH_F32)
      return bad(at + "format must be AGH_DEPTH_U16 or AGH_DEPTH_F32");
    const int64_t es = elem_size(im.format);
    // (a host image is repacked by its copy; a device image is read in place, an element at a time at the least)
    if (on_device && reinterpret_cast<uintptr_t>(im.data) % (uintptr_t) es != 0)
      return bad(at + "data (a device pointer) must be aligned to the element size");
    if (im.row_stride_bytes < im.width * es || im.row_stride_bytes % es != 0)
      return bad(at + "row_stride_bytes must be at least width x element size and a multiple of the element size");
    if (!std::isfinite(im.fx) || im.fx == 0.0)
      return bad(at + "fx must be finite and not zero");
    if (!std::isfinite(im.fy) || im.fy == 0.0)
      return bad(at + "fy must be finite and not zero");
    if (!std::isfinite(im.cx))
      return bad(at + "cx must be finite");
    if (!std::isfinite(im.cy))
      return bad(at + "cy must be finite");
    for (int q = 0; q < 12; q++)
      if (!std::isfinite(im.pose[q]))
        return bad(at + "pose[" + std::to_string(q) + "] must be finite");
    if (im.format == AGH_DEPTH_U16 && !(std::isfinite(im.depth_scale) && im.depth_scale > 0.0f))
      return bad(at + "depth_scale must be finite and positive");
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
    blocks += view_blocks(a.v[k]);
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
    blocks += view_blocks(tab[j]);
  }
  if ((rc = raw_buffer_for(c, base, st)))
    return fail(rc);
  AGH_HIPCHK_OR(c, hipMemcpyAsync(c->d_depth_views, tab, sizeof(DepthView) * (size_t) views, hipMemcpyHostToDevice, st), fail(AGH_ERR_HIP));
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

int agh_deproject(agh_ctx* ctx, const agh_depth_image* images, int32_t n_images, float* xyz_out, int64_t cap_points)
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
