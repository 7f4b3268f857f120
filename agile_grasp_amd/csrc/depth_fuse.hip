// depth_fuse.hip -- agh_fuse_depth (include/agh.h, "DEPTH FUSION"; DESIGN.md, "Depth fusion"): a burst of up to 16 depth frames
// of one camera fused into one depth image in a slot buffer of the context, whose record every agh_*depth*_device call takes.
// k_depth_fuse and its launch, the argument rules, the slots, the staging buffer of the host form, the counters and the getters.
// The chain's kernels are not touched: the fused image is one more device image to them.
// Included at the end of depth.hip: the per-image rules (depth_image_fault), the packing of host images (upload_images,
// depth_image_offset, depth_buffer_bytes), elem_size and GlobalBytes are that file's.

namespace
{
constexpr int kFuseBlock = 256;
constexpr uint32_t kNoReading = 0xffffffffu;  // an invalid reading's key: it sorts behind every valid one

// the frames by value in the kernel's arguments (256 bytes): row v of frame t at data[t] + v * stride[t]
struct FuseFrames
{
  const uint8_t* data[kFuseMaxFrames];
  int64_t stride[kFuseMaxFrames];
};
struct FuseArgs
{
  int32_t w, h, fmt, n_frames, min_valid;
  float scale, sa, sr;
};

// A reading as its sort key.  U16: the raw integer, 1 .. 65535.  F32: the float's bits -- for 0 < z < +inf they order as the floats
// do.  Invalid readings are kNoReading, above both ranges.
__device__ __forceinline__ uint32_t fuse_key(const FuseFrames& f, const int t, const int fmt, const int u, const int v, const bool live)
{
  if (!live)
    return kNoReading;
  const GlobalBytes* row = (const GlobalBytes*) f.data[t] + (int64_t) v * f.stride[t];
  if (fmt == AGH_DEPTH_U16)
  {
    const uint32_t raw = ((const __attribute__((address_space(1))) uint16_t*) row)[u];
    return raw != 0 ? raw : kNoReading;
  }
  const float z = ((const __attribute__((address_space(1))) float*) row)[u];
  return (z > 0.0f && z < __builtin_huge_valf()) ? __float_as_uint(z) : kNoReading;
}

__device__ __forceinline__ float fuse_depth_of(const uint32_t key, const int fmt, const float scale)
{
  return fmt == AGH_DEPTH_U16 ? (float) key * scale : __uint_as_float(key);
}

#define AGH_FUSE_CE(i, j)                  \
  {                                        \
    const uint32_t lo_ = min(s[i], s[j]);  \
    s[j] = max(s[i], s[j]);                \
    s[i] = lo_;                            \
  }
// Batcher's odd-even merge sort of eight keys from s[b] on (19 compare-exchanges) ...
#define AGH_FUSE_SORT8(b)                                                                                                   \
  AGH_FUSE_CE(b + 0, b + 1) AGH_FUSE_CE(b + 2, b + 3) AGH_FUSE_CE(b + 4, b + 5) AGH_FUSE_CE(b + 6, b + 7)                   \
  AGH_FUSE_CE(b + 0, b + 2) AGH_FUSE_CE(b + 1, b + 3) AGH_FUSE_CE(b + 4, b + 6) AGH_FUSE_CE(b + 5, b + 7)                   \
  AGH_FUSE_CE(b + 1, b + 2) AGH_FUSE_CE(b + 5, b + 6)                                                                       \
  AGH_FUSE_CE(b + 0, b + 4) AGH_FUSE_CE(b + 1, b + 5) AGH_FUSE_CE(b + 2, b + 6) AGH_FUSE_CE(b + 3, b + 7)                   \
  AGH_FUSE_CE(b + 2, b + 4) AGH_FUSE_CE(b + 3, b + 5)                                                                       \
  AGH_FUSE_CE(b + 1, b + 2) AGH_FUSE_CE(b + 3, b + 4) AGH_FUSE_CE(b + 5, b + 6)
// ... and its merge of the two sorted halves of sixteen (25): together the 63 of the sixteen-key sort
#define AGH_FUSE_MERGE16                                                                                                    \
  AGH_FUSE_CE(0, 8) AGH_FUSE_CE(1, 9) AGH_FUSE_CE(2, 10) AGH_FUSE_CE(3, 11) AGH_FUSE_CE(4, 12) AGH_FUSE_CE(5, 13)           \
  AGH_FUSE_CE(6, 14) AGH_FUSE_CE(7, 15)                                                                                     \
  AGH_FUSE_CE(4, 8) AGH_FUSE_CE(5, 9) AGH_FUSE_CE(6, 10) AGH_FUSE_CE(7, 11)                                                 \
  AGH_FUSE_CE(2, 4) AGH_FUSE_CE(3, 5) AGH_FUSE_CE(6, 8) AGH_FUSE_CE(7, 9) AGH_FUSE_CE(10, 12) AGH_FUSE_CE(11, 13)           \
  AGH_FUSE_CE(1, 2) AGH_FUSE_CE(3, 4) AGH_FUSE_CE(5, 6) AGH_FUSE_CE(7, 8) AGH_FUSE_CE(9, 10) AGH_FUSE_CE(11, 12)            \
  AGH_FUSE_CE(13, 14)

// One lane = one pixel, pixels row-major; the frames in unrolled loops under the wave-uniform t < n_frames, the readings in
// registers (nothing here is indexed by a runtime value).  The contract's arithmetic (include/agh.h): float32, left to right, not
// contracted (-ffp-contract=off is the build's).  A streaming kernel without LDS: it reads n_frames x W x H elements once and
// writes W x H.  Counters: a ballot and a popcount per class, one atomic per wave and class that has any -- into one of kFuseRows
// rows of counters, 256 bytes apart, that the block index picks: with ONE row the few thousand atomics of an image queue up on
// five addresses of one cache line and take twenty times as long as the pixels (profiles/NOTES.md, "Depth fusion").
extern "C" __global__ __launch_bounds__(kFuseBlock) void k_depth_fuse(FuseFrames f, FuseArgs a, uint8_t* __restrict__ out,
  unsigned long long* __restrict__ counts)
{
  const uint32_t g = blockIdx.x * kFuseBlock + threadIdx.x;  // (W x H is at most 2^26)
  const bool live = g < (uint32_t) a.w * (uint32_t) a.h;
  const int v = live ? (int) (g / (uint32_t) a.w) : 0;
  const int u = live ? (int) (g - (uint32_t) v * (uint32_t) a.w) : 0;

  uint32_t r[kFuseMaxFrames], s[kFuseMaxFrames];
#pragma unroll
  for (int t = 0; t < kFuseMaxFrames; t++)
  {
    r[t] = kNoReading;
    if (t < a.n_frames)
      r[t] = fuse_key(f, t, a.fmt, u, v, live);
    s[t] = r[t];
  }
  int m = 0;
  bool last_ok = false;
#pragma unroll
  for (int t = 0; t < kFuseMaxFrames; t++)
    if (t < a.n_frames)
    {
      last_ok = r[t] != kNoReading;
      m += last_ok ? 1 : 0;
    }

  // (frames beyond n_frames are kNoReading and lie behind already: eight frames or fewer need the lower half only)
  AGH_FUSE_SORT8(0)
  if (a.n_frames > 8)
  {
    AGH_FUSE_SORT8(8)
    AGH_FUSE_MERGE16
  }
  const int pick = (m - 1) / 2;  // 0 .. 7
  uint32_t med = s[0];
#pragma unroll
  for (int j = 1; j < kFuseMaxFrames / 2; j++)
    med = pick == j ? s[j] : med;

  const float zm = fuse_depth_of(med, a.fmt, a.scale);
  const float tol = a.sa + (a.sr * zm);
  int k = 0;
  uint32_t sum = 0;
  float fs = 0.0f;
#pragma unroll
  for (int t = 0; t < kFuseMaxFrames; t++)
    if (t < a.n_frames)
    {
      const float z = fuse_depth_of(r[t], a.fmt, a.scale);
      const bool in = r[t] != kNoReading && fabsf(z - zm) <= tol;
      sum += in ? r[t] : 0u;
      fs = in ? (k == 0 ? z : fs + z) : fs;
      k += in ? 1 : 0;
    }

  const bool empty = live && m == 0;
  const bool unsupported = live && m > 0 && m < a.min_valid;
  const bool inconsistent = live && m >= a.min_valid && k < a.min_valid;
  const bool fused = live && m >= a.min_valid && k >= a.min_valid;
  if (live)
  {
    if (a.fmt == AGH_DEPTH_U16)
    {
      const uint32_t kk = (uint32_t) max(k, 1);
      reinterpret_cast<uint16_t*>(out)[g] = fused ? (uint16_t) ((sum + kk / 2u) / kk) : (uint16_t) 0;
    }
    else
      reinterpret_cast<float*>(out)[g] = fused ? __fdiv_rn(fs, (float) k) : __builtin_nanf("");
  }
  const bool cls[kFuseCounters] = { empty, unsupported, inconsistent, fused, fused && !last_ok };
  const bool first_lane = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int q = 0; q < kFuseCounters; q++)
  {
    const unsigned long long n = (unsigned long long) __popcll(__ballot(cls[q]));
    if (first_lane && n != 0)
      atomicAdd(counts + (blockIdx.x & (kFuseRows - 1)) * kFuseRowWords + q, n);
  }
}

#undef AGH_FUSE_CE
#undef AGH_FUSE_SORT8
#undef AGH_FUSE_MERGE16

inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// the context's fusion state, made by the first call that needs it
int ensure_fuse_state(Ctx* c)
{
  if (c->fuse)
    return AGH_OK;
  unsigned long long* d_counts = nullptr;
  if (int rc = dev_alloc(c, &d_counts, (size_t) kFuseSlots * kFuseSlotWords))
    return rc;
  void* pin = nullptr;
  AGH_HIPCHK_OR(c, hipHostMalloc(&pin, sizeof(int64_t) * (size_t) kFuseSlots * kFuseSlotWords, hipHostMallocDefault),
    ((void) hipFree(d_counts), AGH_ERR_HIP));
  c->fuse = new DepthFuseState();  // (only with both in hand: a failed first call leaves nothing half made)
  c->fuse->d_counts = d_counts;
  c->fuse->h_counts = static_cast<int64_t*>(pin);
  return AGH_OK;
}

int fuse_check(Ctx* c, const char* who, const agh_depth_image* frames, int32_t n_frames, const agh_depth_fusion_params* fp, int32_t slot,
  const agh_depth_image* fused_out, bool on_device)
{
  auto bad = [&](const std::string& what) {
    c->err = std::string(who) + ": " + what;
    return AGH_ERR_INVALID_ARGUMENT;
  };
  if (!frames)
    return bad("frames is NULL");
  if (!fp)
    return bad("params is NULL");
  if (!fused_out)
    return bad("fused_out is NULL");
  if (n_frames < 1 || n_frames > kFuseMaxFrames)
    return bad("n_frames must be 1..16");
  if (slot < 0 || slot >= kFuseSlots)
    return bad("slot must be 0..127");
  if (fp->min_valid < 1 || fp->min_valid > n_frames)
    return bad("min_valid must be 1..n_frames");
  if (!(std::isfinite(fp->max_spread_abs) && fp->max_spread_abs >= 0.0))
    return bad("max_spread_abs must be finite and >= 0");
  if (!(std::isfinite(fp->max_spread_rel) && fp->max_spread_rel >= 0.0))
    return bad("max_spread_rel must be finite and >= 0");
  if (fp->reserved != 0)
    return bad("reserved must be 0");
  const agh_depth_image& f0 = frames[0];
  for (int t = 0; t < n_frames; t++)
  {
    const agh_depth_image& im = frames[t];
    const std::string at = "frame " + std::to_string(t) + ": ";
    const std::string fault = depth_image_fault(im, on_device);
    if (!fault.empty())
      return bad(at + fault);
    if (t == 0)
      continue;
    auto differs = [&](const char* field) { return bad(at + field + " differs from frame 0"); };
    if (im.width != f0.width)
      return differs("width");
    if (im.height != f0.height)
      return differs("height");
    if (im.format != f0.format)
      return differs("format");
    if (std::memcmp(&im.depth_scale, &f0.depth_scale, sizeof(float)) != 0)
      return differs("depth_scale");
    if (!same_bits(im.fx, f0.fx))
      return differs("fx");
    if (!same_bits(im.fy, f0.fy))
      return differs("fy");
    if (!same_bits(im.cx, f0.cx))
      return differs("cx");
    if (!same_bits(im.cy, f0.cy))
      return differs("cy");
    for (int q = 0; q < 12; q++)
      if (!same_bits(im.pose[q], f0.pose[q]))
        return differs(("pose[" + std::to_string(q) + "]").c_str());
  }
  return AGH_OK;
}

int fuse(agh_ctx* ctx, const char* who, const agh_depth_image* frames, int32_t n_frames, const agh_depth_fusion_params* fp, int32_t slot,
  agh_depth_image* fused_out, bool on_device)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, who))
    return AGH_ERR_STATE;
  if (int rc = fuse_check(c, who, frames, n_frames, fp, slot, fused_out, on_device))
    return rc;
  AGH_HIPCHK(c, hipSetDevice(c->device));
  if (int rc = ensure_fuse_state(c))
    return rc;
  DepthFuseState& S = *c->fuse;
  DepthFuseSlot& L = S.slot[slot];
  hipStream_t st = c->stream;
  const agh_depth_image& f0 = frames[0];
  const int64_t es = elem_size(f0.format);
  const int64_t row = (int64_t) f0.width * es, bytes = row * f0.height;
  // (a regrown buffer frees the old one, which waits for whatever still reads it)
  if (bytes > L.cap || !L.d)
  {
    L.cap = 0;
    L.fused = false;
    if (int rc = dev_alloc(c, &L.d, (size_t) bytes))
      return rc;
    L.cap = bytes;
  }
  if (!L.done)
    AGH_HIPCHK(c, hipEventCreateWithFlags(&L.done, hipEventDisableTiming));

  FuseFrames f;
  std::memset(&f, 0, sizeof(f));
  if (on_device)
    for (int t = 0; t < n_frames; t++)
    {
      f.data[t] = static_cast<const uint8_t*>(frames[t].data);
      f.stride[t] = frames[t].row_stride_bytes;
    }
  else
  {
    const int64_t need = depth_buffer_bytes(frames, n_frames);
    if (need > S.stage_cap || !S.d_stage)
    {
      S.stage_cap = 0;
      if (int rc = dev_alloc(c, &S.d_stage, (size_t) need))
        return rc;
      S.stage_cap = need;
    }
    // (the copies queue behind the last kernel that read the staging buffer: one stream)
    AGH_HIPCHK(c, upload_images(S.d_stage, frames, n_frames, st));
    bool pinned = false;
    for (int t = 0; t < n_frames; t++)
    {
      f.data[t] = S.d_stage + depth_image_offset(frames, t);
      f.stride[t] = row;
      pinned = pinned || is_pinned_host(frames[t].data);
    }
    // "returns when the caller's frames have been READ": by itself for pageable frames, page-locked ones are waited for -- the
    // copies only, the kernel stays queued
    if (pinned)
    {
      if (!S.staged)
        AGH_HIPCHK(c, hipEventCreateWithFlags(&S.staged, hipEventDisableTiming));
      AGH_HIPCHK(c, hipEventRecord(S.staged, st));
      AGH_HIPCHK(c, hipEventSynchronize(S.staged));
    }
  }
  FuseArgs a;
  a.w = f0.width;
  a.h = f0.height;
  a.fmt = f0.format;
  a.n_frames = n_frames;
  a.min_valid = fp->min_valid;
  a.scale = f0.depth_scale;
  a.sa = (float) fp->max_spread_abs;
  a.sr = (float) fp->max_spread_rel;
  unsigned long long* d_counts = S.d_counts + (size_t) slot * kFuseSlotWords;
  int64_t* h_counts = S.h_counts + (size_t) slot * kFuseSlotWords;
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are read back as int64_t");
  AGH_HIPCHK(c, hipMemsetAsync(d_counts, 0, sizeof(int64_t) * kFuseSlotWords, st));
  const int64_t pixels = (int64_t) f0.width * f0.height;
  const unsigned blocks = (unsigned) ((pixels + kFuseBlock - 1) / kFuseBlock);
  hipLaunchKernelGGL(k_depth_fuse, dim3(blocks), dim3(kFuseBlock), 0, st, f, a, L.d, d_counts);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = std::string(who) + ": k_depth_fuse launch failed";
    L.fused = false;
    return AGH_ERR_HIP;
  }
  AGH_HIPCHK(c, hipMemcpyAsync(h_counts, d_counts, sizeof(int64_t) * kFuseSlotWords, hipMemcpyDeviceToHost, st));
  AGH_HIPCHK(c, hipEventRecord(L.done, st));
  L.rec = f0;
  L.rec.data = L.d;
  L.rec.row_stride_bytes = row;
  L.fused = true;
  *fused_out = L.rec;
  return AGH_OK;
}

// a slot's state for a getter, behind its kernel: nullptr with *rc set (0: never fused)
DepthFuseSlot* fused_slot(agh_ctx* ctx, const char* who, int32_t slot, int* rc)
{
  *rc = AGH_ERR_INVALID_ARGUMENT;
  if (!ctx)
    return nullptr;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, who))
  {
    *rc = AGH_ERR_STATE;
    return nullptr;
  }
  if (slot < 0 || slot >= kFuseSlots)
  {
    c->err = std::string(who) + ": slot must be 0..127";
    return nullptr;
  }
  *rc = 0;
  if (!c->fuse || !c->fuse->slot[slot].fused)
    return nullptr;
  DepthFuseSlot* L = &c->fuse->slot[slot];
  if (hipSetDevice(c->device) != hipSuccess || hipEventSynchronize(L->done) != hipSuccess)
  {
    c->err = std::string(who) + ": " + hipGetErrorString(hipGetLastError());
    *rc = AGH_ERR_HIP;
    return nullptr;
  }
  return L;
}
}  // namespace

namespace agh
{
void depth_fuse_release(Ctx* c)
{
  DepthFuseState* S = c->fuse;
  if (!S)
    return;
  for (DepthFuseSlot& L : S->slot)
  {
    if (L.d)
      (void) hipFree(L.d);
    if (L.done)
      (void) hipEventDestroy(L.done);
  }
  if (S->d_stage)
    (void) hipFree(S->d_stage);
  if (S->d_counts)
    (void) hipFree(S->d_counts);
  if (S->h_counts)
    (void) hipHostFree(S->h_counts);
  if (S->staged)
    (void) hipEventDestroy(S->staged);
  delete S;
  c->fuse = nullptr;
}
}  // namespace agh

extern "C" {

void agh_default_depth_fusion_params(agh_depth_fusion_params* p)
{
  if (!p)
    return;
  p->min_valid = 2;
  p->reserved = 0;
  p->max_spread_abs = 0.005;
  p->max_spread_rel = 0.005;
}

int agh_fuse_depth(agh_ctx* ctx, const agh_depth_image* frames, int32_t n_frames, const agh_depth_fusion_params* fp, int32_t slot,
  agh_depth_image* fused_out)
{
  return fuse(ctx, "agh_fuse_depth", frames, n_frames, fp, slot, fused_out, false);
}

int agh_fuse_depth_device(agh_ctx* ctx, const agh_depth_image* frames, int32_t n_frames, const agh_depth_fusion_params* fp, int32_t slot,
  agh_depth_image* fused_out)
{
  return fuse(ctx, "agh_fuse_depth_device", frames, n_frames, fp, slot, fused_out, true);
}

int agh_get_depth_fusion_counts(agh_ctx* ctx, int32_t slot, agh_depth_fusion_counts* out)
{
  int rc;
  const DepthFuseSlot* L = fused_slot(ctx, "agh_get_depth_fusion_counts", slot, &rc);
  if (!L)
    return rc;
  Ctx* c = &ctx->c;
  if (!out)
  {
    c->err = "agh_get_depth_fusion_counts: out is NULL";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  int64_t n[kFuseCounters] = {};
  for (int row = 0; row < kFuseRows; row++)
    for (int q = 0; q < kFuseCounters; q++)
      n[q] += c->fuse->h_counts[(size_t) slot * kFuseSlotWords + (size_t) row * kFuseRowWords + q];
  out->n_pixels = (int64_t) L->rec.width * L->rec.height;
  out->n_empty = n[kFuseEmpty];
  out->n_unsupported = n[kFuseUnsupported];
  out->n_inconsistent = n[kFuseInconsistent];
  out->n_fused = n[kFuseFused];
  out->n_filled = n[kFuseFilled];
  return 1;
}

int agh_get_fused_depth(agh_ctx* ctx, int32_t slot, void* pixels_out, int64_t cap_bytes, agh_depth_image* record_out)
{
  int rc;
  const DepthFuseSlot* L = fused_slot(ctx, "agh_get_fused_depth", slot, &rc);
  if (!L)
    return rc;
  Ctx* c = &ctx->c;
  if (record_out)  // (also in front of AGH_ERR_CAPACITY: the record says how many bytes the image has)
    *record_out = L->rec;
  const int64_t bytes = L->rec.row_stride_bytes * L->rec.height;
  if (!pixels_out || cap_bytes < bytes)
  {
    c->err = "agh_get_fused_depth: pixels_out must hold the image's " + std::to_string(bytes) + " bytes";
    return AGH_ERR_CAPACITY;
  }
  AGH_HIPCHK(c, hipMemcpy(pixels_out, L->d, (size_t) bytes, hipMemcpyDeviceToHost));
  return (int) bytes;
}

}  // extern "C"
