// plane.hip -- the table-plane removal of Localization::localizeHands(..., uses_clustering = true) (localization.cpp:51-98):
// pcl::SACSegmentation (SACMODEL_PLANE, SAC_RANSAC, 100 iterations, threshold 0.01, refit on) followed by
// pcl::ExtractIndices::setNegative(true).  The algorithm as restated from PCL 1.7 is in DESIGN.md ("Table-plane removal");
// tests/cpp/plane_ref.cpp is its host transcription, and the GPU agrees with it bit for bit.
//
// RANSAC's draws depend only on the cloud and the seed, not on the inlier counts, so the loop is unrolled:
//   k_plane_candidates  one lane: boost::mt19937, the persistent partial Fisher-Yates of drawIndexSample, isSampleGood and
//                       computeModelCoefficients -- the max_iterations + 1 candidate planes RANSAC may score, in order
//   k_plane_score       every work-group reads its points once and counts the inliers of ALL candidates (ballot +
//                       popcount, integer atomics: exact in any order)
//   host                one read-back; RandomSampleConsensus::computeModel's termination replayed over the counts (glibc
//                       log / pow, as the restatement)
//   k_plane_count / k_plane_scan / k_plane_terms / k_plane_moments
//                       the nine float sums of computeMeanAndCovarianceMatrix over the inliers IN INLIER ORDER: the
//                       products are written compacted (stable), then nine lanes run the nine dependent chains while the
//                       other waves stage the next chunk into LDS
//   host                pcl::eigen33 (atan2f / cosf / sinf of the host's libm, as the restatement)
//   k_plane_count / k_plane_scan / k_plane_split
//                       reselection with the refined plane: inlier indices and the kept points, compacted stably; the kept
//                       points become the context's cloud through agh_set_cloud_device
// The distance test is PCL's  fabsf(dot) < threshold  with a DOUBLE threshold; a float |dot| passes it exactly when it is
// <= the largest float below the threshold, which is what the kernels compare against.
#include "agh_internal.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace agh
{

constexpr int kPlaneMaxCand = 1024;       // max_iterations + 1 candidates at most (agh_plane_params::max_iterations < 1024)
constexpr int kPlaneSampleChecks = 1000;  // SampleConsensusModel::max_sample_checks_
constexpr int kPlaneScorePts = 8;         // points per thread of k_plane_score
constexpr int kPlaneChunk = 512;          // inliers per LDS chunk of k_plane_moments

struct PlaneCand
{
  float c[4];      // a, b, c, d
  int32_t s[3];    // the sample's point indices
  int32_t pad;
};
struct PlaneHdr
{
  int32_t n_cand;   // candidates drawn
  int32_t skipped;  // computeModelCoefficients refusals (never after isSampleGood: the same test)
  int32_t n_in;     // inliers of the last k_plane_scan
  int32_t pad;
};

struct PlaneState
{
  int32_t* d_shuf = nullptr;  // shuffled_indices_ beyond its first three entries (those live in registers)
  int64_t shuf_cap = 0;
  PlaneCand* d_cand = nullptr;
  unsigned* d_counts = nullptr;
  PlaneHdr* d_hdr = nullptr;
  float* d_accu = nullptr;
  int* d_blk = nullptr;       // inliers per tile of 256 points ...
  int* d_blk_off = nullptr;   // ... and their exclusive prefix sums
  int64_t blk_cap = 0;
  float* d_terms = nullptr;   // 9 x (inliers): xx xy xz yy yz zz x y z of the inliers, in inlier order, term-major
  int64_t terms_floats = 0;
  int32_t* d_idx = nullptr;   // the inliers of the last call (agh_get_plane_inliers)
  int64_t idx_cap = 0;
  float* d_xyz[2] = { nullptr, nullptr };  // the kept cloud: two sets, so that a second call never writes the cloud it reads
  int32_t* d_cam[2] = { nullptr, nullptr };
  int64_t out_cap[2] = { 0, 0 };
  // last call
  bool has_result = false;
  int64_t n_inliers = 0;
  std::vector<PlaneCand> cand;
  std::vector<int64_t> counts;
};

void plane_release(Ctx* c)
{
  PlaneState* P = c->plane;
  if (!P)
    return;
  void* ptrs[] = { P->d_shuf, P->d_cand, P->d_counts, P->d_hdr, P->d_accu, P->d_blk, P->d_blk_off, P->d_terms, P->d_idx,
    P->d_xyz[0], P->d_xyz[1], P->d_cam[0], P->d_cam[1] };
  for (void* p : ptrs)
    if (p)
      (void) hipFree(p);
  delete P;
  c->plane = nullptr;
}

namespace
{

template <typename T>
int plane_grow(Ctx* c, T** p, int64_t* cap, int64_t need)
{
  if (need <= *cap && *p)
    return AGH_OK;
  const int rc = dev_alloc(c, p, (size_t) std::max<int64_t>(need, 1));
  if (rc == AGH_OK)
    *cap = std::max<int64_t>(need, 1);
  return rc;
}

// ---- device side ----

// SampleConsensusModelPlane's point-to-plane value  model_coefficients.dot(Vector4f(x, y, z, 1))  in the association order
// of a 4-float SSE packet reduction, ((a x + c z) + (b y + d 1)) -- DESIGN.md states the order (Eigen's is not pinned)
__device__ __forceinline__ float plane_dot(float4 p, float x, float y, float z)
{
  return (p.x * x + p.z * z) + (p.y * y + p.w * 1.0f);
}

__device__ __forceinline__ void plane_point(const float* __restrict__ xyz, int64_t sf, int64_t i, float& x, float& y, float& z)
{
  const float* q = xyz + i * sf;
  x = q[0];
  y = q[1];
  z = q[2];
}

__device__ __forceinline__ bool plane_in(const float* __restrict__ xyz, int64_t sf, int64_t i, float4 p, float thr)
{
  float x, y, z;
  plane_point(xyz, sf, i, x, y, z);
  return fabsf(plane_dot(p, x, y, z)) <= thr;  // (NaN: false, as PCL's  <  is)
}

__device__ __forceinline__ uint32_t mt_next(uint32_t* mt, int& mti)
{
  if (mti >= 624)
  {
    for (int k = 0; k < 624; k++)
    {
      const uint32_t y = (mt[k] & 0x80000000u) | (mt[k + 1 < 624 ? k + 1 : 0] & 0x7fffffffu);
      mt[k] = mt[k + 397 < 624 ? k + 397 : k + 397 - 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    mti = 0;
  }
  uint32_t y = mt[mti++];
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__global__ __launch_bounds__(256) void k_plane_iota(int32_t* __restrict__ shuf, int n)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n)
    shuf[i] = i;
}

// One lane draws; the other lanes of the group clear the counts k_plane_score adds into.
__global__ __launch_bounds__(64) void k_plane_candidates(const float* __restrict__ xyz, int64_t sf, int n, int32_t* __restrict__ shuf,
  PlaneCand* __restrict__ cand, unsigned* __restrict__ counts, PlaneHdr* __restrict__ hdr, int max_cand, int max_skip, uint32_t seed)
{
  __shared__ uint32_t mt[624];
  for (int k = threadIdx.x; k < max_cand; k += 64)
    counts[k] = 0u;
  if (threadIdx.x != 0)
    return;
  mt[0] = seed;
  for (int k = 1; k < 624; k++)
    mt[k] = 1812433253u * (mt[k - 1] ^ (mt[k - 1] >> 30)) + (uint32_t) k;
  int mti = 624;
  int s0 = 0, s1 = 1, s2 = 2;  // shuffled_indices_[0 .. 2]
  int n_cand = 0, skipped = 0;
  while (n >= 3 && n_cand < max_cand && skipped < max_skip)
  {
    // getSamples: at most max_sample_checks_ draws until isSampleGood
    bool good = false;
    float x0 = 0.f, y0 = 0.f, z0 = 0.f, dx1 = 0.f, dy1 = 0.f, dz1 = 0.f, dx2 = 0.f, dy2 = 0.f, dz2 = 0.f;
    for (int t = 0; t < kPlaneSampleChecks && !good; t++)
    {
      // drawIndexSample: swap(shuffled_indices_[i], shuffled_indices_[i + rnd() % (N - i)]), rnd() = mt19937() >> 1
#pragma unroll
      for (int i = 0; i < 3; i++)
      {
        const uint32_t r = mt_next(mt, mti) >> 1;
        const int j = i + (int) (r % (uint32_t) (n - i));
        const int vi = i == 0 ? s0 : (i == 1 ? s1 : s2);
        const int vj = j == 0 ? s0 : (j == 1 ? s1 : (j == 2 ? s2 : shuf[j]));
        if (i == 0)
          s0 = vj;
        else if (i == 1)
          s1 = vj;
        else
          s2 = vj;
        if (j == 0)
          s0 = vi;
        else if (j == 1)
          s1 = vi;
        else if (j == 2)
          s2 = vi;
        else
          shuf[j] = vi;
      }
      float x1, y1, z1, x2, y2, z2;
      plane_point(xyz, sf, s0, x0, y0, z0);
      plane_point(xyz, sf, s1, x1, y1, z1);
      plane_point(xyz, sf, s2, x2, y2, z2);
      dx1 = x1 - x0, dy1 = y1 - y0, dz1 = z1 - z0;
      dx2 = x2 - x0, dy2 = y2 - y0, dz2 = z2 - z0;
      const float r0 = dx1 / dx2, r1 = dy1 / dy2, r2 = dz1 / dz2;
      good = (r0 != r1) || (r2 != r1);  // isSampleGood
    }
    if (!good)
      break;  // an empty selection ends RANSAC's loop
    {
      // computeModelCoefficients: its collinearity test is isSampleGood's negation
      const float r0 = dx1 / dx2, r1 = dy1 / dy2, r2 = dz1 / dz2;
      if (r0 == r1 && r2 == r1)
      {
        skipped++;
        continue;
      }
    }
    float a = dy1 * dz2 - dz1 * dy2;
    float b = dz1 * dx2 - dx1 * dz2;
    float cc = dx1 * dy2 - dy1 * dx2;
    float w = 0.0f;
    const float norm = sqrtf((a * a + cc * cc) + (b * b + w * w));
    a = a / norm, b = b / norm, cc = cc / norm, w = w / norm;
    const float d = -((a * x0 + cc * z0) + (b * y0 + w * 1.0f));
    PlaneCand pc;
    pc.c[0] = a, pc.c[1] = b, pc.c[2] = cc, pc.c[3] = d;
    pc.s[0] = s0, pc.s[1] = s1, pc.s[2] = s2;
    pc.pad = 0;
    cand[n_cand++] = pc;
  }
  PlaneHdr h;
  h.n_cand = n_cand, h.skipped = skipped, h.n_in = 0, h.pad = 0;
  *hdr = h;
}

__global__ __launch_bounds__(256) void k_plane_score(const float* __restrict__ xyz, int64_t sf, int n,
  const PlaneCand* __restrict__ cand, const PlaneHdr* __restrict__ hdr, float thr, unsigned* __restrict__ counts)
{
  __shared__ float4 sp[kPlaneMaxCand];
  __shared__ unsigned sc[kPlaneMaxCand];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nc = hdr->n_cand;
  for (int k = tid; k < nc; k += 256)
  {
    sp[k] = make_float4(cand[k].c[0], cand[k].c[1], cand[k].c[2], cand[k].c[3]);
    sc[k] = 0u;
  }
  __syncthreads();
  float px[kPlaneScorePts], py[kPlaneScorePts], pz[kPlaneScorePts];
  bool v[kPlaneScorePts];
  const int64_t base = (int64_t) blockIdx.x * 256 * kPlaneScorePts + tid;
#pragma unroll
  for (int u = 0; u < kPlaneScorePts; u++)
  {
    const int64_t i = base + u * 256;
    v[u] = i < n;
    px[u] = py[u] = pz[u] = 0.f;
    if (v[u])
      plane_point(xyz, sf, i, px[u], py[u], pz[u]);
  }
  for (int k = 0; k < nc; k++)
  {
    const float4 p = sp[k];
    unsigned cnt = 0;
#pragma unroll
    for (int u = 0; u < kPlaneScorePts; u++)
      cnt += (unsigned) __popcll(__ballot(v[u] && fabsf(plane_dot(p, px[u], py[u], pz[u])) <= thr));
    if (lane == 0 && cnt)
      atomicAdd(&sc[k], cnt);
  }
  __syncthreads();
  for (int k = tid; k < nc; k += 256)
    if (sc[k])
      atomicAdd(&counts[k], sc[k]);
}

// position of this lane's point among the points of its 256-point tile that pass `pred` (exclusive); wc: 4 ints of LDS
__device__ __forceinline__ int tile_rank(bool pred, int* wc)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long m = __ballot(pred);
  if (lane == 0)
    wc[wave] = __popcll(m);
  __syncthreads();
  int r = __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; w++)
    r += wc[w];
  return r;
}

__global__ __launch_bounds__(256) void k_plane_count(const float* __restrict__ xyz, int64_t sf, int n, float4 p, float thr,
  int* __restrict__ blk)
{
  __shared__ int wc[4];
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  const unsigned long long m = __ballot(i < n && plane_in(xyz, sf, i, p, thr));
  if ((threadIdx.x & 63) == 0)
    wc[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0)
    blk[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// exclusive prefix sums of the tile counts (one work-group); hdr->n_in = the total
__global__ __launch_bounds__(1024) void k_plane_scan(const int* __restrict__ blk, int nblk, int* __restrict__ off, PlaneHdr* __restrict__ hdr)
{
  __shared__ int ws[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (nblk + 1023) / 1024;
  const int lo = std::min(tid * per, nblk), hi = std::min(lo + per, nblk);
  int s = 0;
  for (int k = lo; k < hi; k++)
    s += blk[k];
  int incl = s;
  for (int d = 1; d < 64; d <<= 1)
  {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d)
      incl += t;
  }
  if (lane == 63)
    ws[wave] = incl;
  __syncthreads();
  int run = incl - s;
  for (int w = 0; w < wave; w++)
    run += ws[w];
  for (int k = lo; k < hi; k++)
  {
    off[k] = run;
    run += blk[k];
  }
  if (tid == 1023)
    hdr->n_in = run;
}

// the nine products of every inlier, at its position in the inlier list (terms: 9 x cap, term-major)
__global__ __launch_bounds__(256) void k_plane_terms(const float* __restrict__ xyz, int64_t sf, int n, float4 p, float thr,
  const int* __restrict__ off, float* __restrict__ terms, int64_t cap)
{
  __shared__ int wc[4];
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < n)
    plane_point(xyz, sf, i, x, y, z);
  const bool in = i < n && fabsf(plane_dot(p, x, y, z)) <= thr;
  const int r = off[blockIdx.x] + tile_rank(in, wc);
  if (in && r < cap)  // (cap: the chosen candidate's score, which this pass reproduces)
  {
    terms[0 * cap + r] = x * x;
    terms[1 * cap + r] = x * y;
    terms[2 * cap + r] = x * z;
    terms[3 * cap + r] = y * y;
    terms[4 * cap + r] = y * z;
    terms[5 * cap + r] = z * z;
    terms[6 * cap + r] = x;
    terms[7 * cap + r] = y;
    terms[8 * cap + r] = z;
  }
}

// one chunk of the nine term arrays into LDS by the 192 lanes of waves 1 .. 3: every lane issues its 24 loads before it stores
// any of them (one memory latency per chunk, not 24); entries past the inliers are left as zeros nobody reads
__device__ __forceinline__ void plane_stage(const float* __restrict__ terms, int64_t cap, int m, int k0, float* dst, int t)
{
  constexpr int kPer = 9 * kPlaneChunk / 192;
  float v[kPer];
#pragma unroll
  for (int q = 0; q < kPer; q++)
  {
    const int e = t + 192 * q, j = e / kPlaneChunk, k = e - j * kPlaneChunk;
    v[q] = k0 + k < m ? terms[j * cap + k0 + k] : 0.0f;
  }
#pragma unroll
  for (int q = 0; q < kPer; q++)
    dst[t + 192 * q] = v[q];
}

// computeMeanAndCovarianceMatrix's accumulation: accu[j] += term j of inlier k for k = 0, 1, ... -- nine dependent float
// chains, one per lane of wave 0, fed from LDS (16-byte reads, the adds one by one in order); waves 1 .. 3 stage the next
// chunk meanwhile.
__global__ __launch_bounds__(256) void k_plane_moments(const float* __restrict__ terms, int64_t cap, const PlaneHdr* __restrict__ hdr,
  float* __restrict__ accu)
{
  static_assert((9 * kPlaneChunk) % 192 == 0 && kPlaneChunk % 4 == 0, "chunk layout");
  __shared__ __align__(16) float buf[2][9 * kPlaneChunk];
  const int tid = threadIdx.x;
  const int m = (int) std::min<int64_t>(hdr->n_in, cap);
  const int nch = (m + kPlaneChunk - 1) / kPlaneChunk;
  float acc = 0.0f;
  if (tid >= 64 && nch > 0)
    plane_stage(terms, cap, m, 0, buf[0], tid - 64);
  __syncthreads();
  for (int ch = 0; ch < nch; ch++)
  {
    if (tid >= 64 && ch + 1 < nch)
      plane_stage(terms, cap, m, (ch + 1) * kPlaneChunk, buf[(ch + 1) & 1], tid - 64);
    if (tid < 9)
    {
      const float* b = buf[ch & 1] + tid * kPlaneChunk;
      const int len = std::min(kPlaneChunk, m - ch * kPlaneChunk);
      const float4* b4 = reinterpret_cast<const float4*>(b);
      int k = 0;
#pragma unroll 4
      for (; k + 4 <= len; k += 4)
      {
        const float4 q = b4[k >> 2];
        acc += q.x;
        acc += q.y;
        acc += q.z;
        acc += q.w;
      }
      for (; k < len; k++)
        acc += b[k];
    }
    __syncthreads();
  }
  if (tid < 9)
    accu[tid] = acc;
}

// reselection: the inliers' indices at their positions, the other points (and camera ids) packed in their order
__global__ __launch_bounds__(256) void k_plane_split(const float* __restrict__ xyz, int64_t sf, int n, const int32_t* __restrict__ cam,
  float4 p, float thr, const int* __restrict__ off, int32_t* __restrict__ idx, float* __restrict__ xyz_out, int32_t* __restrict__ cam_out,
  int cam_by_position)
{
  __shared__ int wc[4];
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < n)
    plane_point(xyz, sf, i, x, y, z);
  const bool in = i < n && fabsf(plane_dot(p, x, y, z)) <= thr;
  const int r = off[blockIdx.x] + tile_rank(in, wc);  // inliers before point i
  if (i >= n)
    return;
  if (in)
    idx[r] = (int32_t) i;
  else
  {
    const int64_t o = i - r;
    xyz_out[3 * o] = x;
    xyz_out[3 * o + 1] = y;
    xyz_out[3 * o + 2] = z;
    cam_out[o] = cam ? cam[cam_by_position ? o : i] : 0;
  }
}

// ---- host side (the restatement's arithmetic: IEEE float / double, no contraction, the host's libm) ----

// computeRoots2 (pcl/common/eigen.hpp): the roots of x^2 - b x + c with a zero root
void compute_roots2(float b, float c, float roots[3])
{
  roots[0] = 0.0f;
  float d = (float) (b * b - 4.0 * c);
  if (d < 0.0)
    d = 0.0f;
  const float sd = std::sqrt(d);
  roots[2] = 0.5f * (b + sd);
  roots[1] = 0.5f * (b - sd);
}

// computeRoots: the eigenvalues of a symmetric 3 x 3 matrix, ascending
void compute_roots(const float m[3][3], float roots[3])
{
  const float c0 = m[0][0] * m[1][1] * m[2][2] + 2.0f * m[0][1] * m[0][2] * m[1][2] - m[0][0] * m[1][2] * m[1][2] -
    m[1][1] * m[0][2] * m[0][2] - m[2][2] * m[0][1] * m[0][1];
  const float c1 = m[0][0] * m[1][1] - m[0][1] * m[0][1] + m[0][0] * m[2][2] - m[0][2] * m[0][2] + m[1][1] * m[2][2] -
    m[1][2] * m[1][2];
  const float c2 = m[0][0] + m[1][1] + m[2][2];
  if (std::fabs(c0) < std::numeric_limits<float>::epsilon())
  {
    compute_roots2(c2, c1, roots);
    return;
  }
  const float s_inv3 = (float) (1.0 / 3.0);
  const float s_sqrt3 = std::sqrt(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0f)
    a_over_3 = 0.0f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0f)
    q = 0.0f;
  const float rho = std::sqrt(-a_over_3);
  const float theta = std::atan2(std::sqrt(-q), half_b) * s_inv3;
  const float cos_theta = std::cos(theta);
  const float sin_theta = std::sin(theta);
  roots[0] = c2_over_3 + 2.0f * rho * cos_theta;
  roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  if (roots[0] >= roots[1])
    std::swap(roots[0], roots[1]);
  if (roots[1] >= roots[2])
  {
    std::swap(roots[1], roots[2]);
    if (roots[0] >= roots[1])
      std::swap(roots[0], roots[1]);
  }
  if (roots[0] <= 0.0f)
    compute_roots2(c2, c1, roots);
}

// pcl::eigen33(mat, eigenvalue, eigenvector): the eigenvector of the smallest eigenvalue
void eigen33_smallest(const float mat[3][3], float v[3])
{
  float scale = 0.0f;
  for (int j = 0; j < 3; j++)  // (column-major, as Eigen visits a Matrix3f; the order only matters for NaN)
    for (int i = 0; i < 3; i++)
      scale = std::max(scale, std::fabs(mat[i][j]));
  if (scale <= std::numeric_limits<float>::min())
    scale = 1.0f;
  float s[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      s[i][j] = mat[i][j] / scale;
  float roots[3];
  compute_roots(s, roots);
  for (int i = 0; i < 3; i++)
    s[i][i] -= roots[0];
  auto cross = [](const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  float v1[3], v2[3], v3[3];
  cross(s[0], s[1], v1);
  cross(s[0], s[2], v2);
  cross(s[1], s[2], v3);
  // squaredNorm of a Vector3f: Eigen's unrolled reduction x^2 + (y^2 + z^2)
  const float len1 = v1[0] * v1[0] + (v1[1] * v1[1] + v1[2] * v1[2]);
  const float len2 = v2[0] * v2[0] + (v2[1] * v2[1] + v2[2] * v2[2]);
  const float len3 = v3[0] * v3[0] + (v3[1] * v3[1] + v3[2] * v3[2]);
  const float* src;
  float len;
  if (len1 >= len2 && len1 >= len3)
    src = v1, len = len1;
  else if (len2 >= len1 && len2 >= len3)
    src = v2, len = len2;
  else
    src = v3, len = len3;
  const float sq = std::sqrt(len);
  for (int k = 0; k < 3; k++)
    v[k] = src[k] / sq;
}

// optimizeModelCoefficients from the nine sums: centroid, covariance, eigen33, plane through the centroid
void plane_refit(const float accu_in[9], int64_t n_in, float out[4])
{
  float a[9];
  const float cnt = (float) n_in;
  for (int k = 0; k < 9; k++)
    a[k] = accu_in[k] / cnt;
  float m[3][3];
  m[0][0] = a[0] - a[6] * a[6];
  m[0][1] = a[1] - a[6] * a[7];
  m[0][2] = a[2] - a[6] * a[8];
  m[1][1] = a[3] - a[7] * a[7];
  m[1][2] = a[4] - a[7] * a[8];
  m[2][2] = a[5] - a[8] * a[8];
  m[1][0] = m[0][1];
  m[2][0] = m[0][2];
  m[2][1] = m[1][2];
  float v[3];
  eigen33_smallest(m, v);
  const float w = 0.0f;
  out[0] = v[0], out[1] = v[1], out[2] = v[2];
  out[3] = -1.0f * ((v[0] * a[6] + v[2] * a[8]) + (v[1] * a[7] + w * 1.0f));
}

// the largest float below the double threshold: fabsf(x) < thr (in double) <=> fabsf(x) <= this
float plane_threshold(double thr)
{
  float t = (float) thr;
  if ((double) t >= thr)
    t = std::nextafter(t, -std::numeric_limits<float>::infinity());
  return t;
}

}  // namespace
}  // namespace agh

using namespace agh;

void agh_default_plane_params(agh_plane_params* p)
{
  if (!p)
    return;
  p->max_iterations = 100;
  p->optimize = 1;
  p->distance_threshold = 0.01;
  p->probability = 0.99;
  p->seed = 12345u;
  p->cam_ids_by_position = 1;
}

void agh_plane_replay(const int64_t* counts, int64_t n, int64_t n_points, int32_t max_iterations, double probability,
  int32_t* best, int32_t* iterations)
{
  // RandomSampleConsensus::computeModel (sac/impl/ransac.hpp), candidate i being the i-th model it scores
  int32_t b = -1, it = 0;
  int64_t n_best = -INT_MAX;
  double k = 1.0;
  const double log_probability = std::log(1.0 - probability);
  const double one_over_indices = 1.0 / (double) n_points;
  for (int64_t i = 0; counts && i < n && it < k; i++)
  {
    if (counts[i] > n_best)
    {
      n_best = counts[i];
      b = (int32_t) i;
      const double w = (double) n_best * one_over_indices;
      double p_no_outliers = 1.0 - std::pow(w, 3.0);
      p_no_outliers = std::max(std::numeric_limits<double>::epsilon(), p_no_outliers);
      p_no_outliers = std::min(1.0 - std::numeric_limits<double>::epsilon(), p_no_outliers);
      k = log_probability / std::log(p_no_outliers);
    }
    ++it;
    if (it > max_iterations)
      break;
  }
  if (best)
    *best = b;
  if (iterations)
    *iterations = it;
}

int agh_remove_plane(agh_ctx* ctx, const agh_plane_params* pp, agh_plane_result* result)
{
  if (!ctx)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (result)
    std::memset(result, 0, sizeof(*result));
  if (!pp || !result || pp->max_iterations < 0 || pp->max_iterations >= kPlaneMaxCand || !(pp->probability > 0.0) ||
      !(pp->probability < 1.0) || !(pp->distance_threshold >= 0.0))
  {
    c->err = "agh_remove_plane: need params, a result, 0 <= max_iterations < 1024, 0 < probability < 1, threshold >= 0";
    return AGH_ERR_INVALID_ARGUMENT;
  }
  if (c->loc.active)
  {
    c->err = "agh_remove_plane: an agh_localize_begin chain is in flight (agh_localize_end first)";
    return AGH_ERR_STATE;
  }
  if (!c->has_cloud || c->n_clouds != 1)
  {
    c->err = "agh_remove_plane: needs one cloud (agh_set_cloud* or agh_preprocess*), not none and not a batch";
    return AGH_ERR_STATE;
  }
  AGH_HIPCHK(c, hipSetDevice(c->device));
  if (!c->plane)
    c->plane = new PlaneState;
  PlaneState& P = *c->plane;
  P.has_result = false;
  P.n_inliers = 0;
  P.cand.clear();
  P.counts.clear();
  const int n = (int) c->n;
  const float* xyz = c->d_xyz;
  const int64_t sf = c->stride_floats;
  const int32_t* cam = c->d_cam;
  hipStream_t st = c->stream;
  result->n_remaining = n;
  if (n < 3)  // getSamples refuses: no model, the cloud stays
  {
    P.has_result = true;
    return AGH_OK;
  }
  const int max_cand = pp->max_iterations + 1;
  const int64_t nblk = (n + 255) / 256;
  int rc;
  if ((rc = plane_grow(c, &P.d_shuf, &P.shuf_cap, n)) || (rc = plane_grow(c, &P.d_idx, &P.idx_cap, n)))
    return rc;
  if (nblk > P.blk_cap || !P.d_blk)
  {
    if ((rc = dev_alloc(c, &P.d_blk, (size_t) nblk)) || (rc = dev_alloc(c, &P.d_blk_off, (size_t) nblk)))
      return rc;
    P.blk_cap = nblk;
  }
  if (!P.d_cand && ((rc = dev_alloc(c, &P.d_cand, kPlaneMaxCand)) || (rc = dev_alloc(c, &P.d_counts, kPlaneMaxCand)) ||
                    (rc = dev_alloc(c, &P.d_hdr, 1)) || (rc = dev_alloc(c, &P.d_accu, 9))))
    return rc;
  const float thr = plane_threshold(pp->distance_threshold);

  // 1. candidates and their scores, one read-back
  hipLaunchKernelGGL(k_plane_iota, dim3((unsigned) nblk), dim3(256), 0, st, P.d_shuf, n);
  hipLaunchKernelGGL(k_plane_candidates, dim3(1), dim3(64), 0, st, xyz, sf, n, P.d_shuf, P.d_cand, P.d_counts, P.d_hdr, max_cand,
    10 * pp->max_iterations, pp->seed);
  const int64_t per_blk = 256 * kPlaneScorePts;
  hipLaunchKernelGGL(k_plane_score, dim3((unsigned) ((n + per_blk - 1) / per_blk)), dim3(256), 0, st, xyz, sf, n,
    (const PlaneCand*) P.d_cand, (const PlaneHdr*) P.d_hdr, thr, P.d_counts);
  AGH_HIPCHK(c, hipGetLastError());
  PlaneHdr hdr;
  std::vector<unsigned> cnt((size_t) max_cand);
  P.cand.resize((size_t) max_cand);
  AGH_HIPCHK(c, hipMemcpyAsync(&hdr, P.d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
  AGH_HIPCHK(c, hipMemcpyAsync(P.cand.data(), P.d_cand, sizeof(PlaneCand) * (size_t) max_cand, hipMemcpyDeviceToHost, st));
  AGH_HIPCHK(c, hipMemcpyAsync(cnt.data(), P.d_counts, sizeof(unsigned) * (size_t) max_cand, hipMemcpyDeviceToHost, st));
  AGH_HIPCHK(c, hipStreamSynchronize(st));
  P.cand.resize((size_t) hdr.n_cand);
  P.counts.assign(cnt.begin(), cnt.begin() + hdr.n_cand);

  // 2. the termination rule, replayed
  int32_t best = -1, iterations = 0;
  agh_plane_replay(P.counts.data(), hdr.n_cand, n, pp->max_iterations, pp->probability, &best, &iterations);
  result->iterations = iterations;
  if (best < 0)  // no sample passed: no model, the cloud stays
  {
    P.has_result = true;
    return AGH_OK;
  }
  const PlaneCand& bc = P.cand[(size_t) best];
  float plane[4] = { bc.c[0], bc.c[1], bc.c[2], bc.c[3] };

  // 3. the refit over the model's inliers (optimizeModelCoefficients: at least 4 of them)
  if (pp->optimize && P.counts[(size_t) best] >= 4)
  {
    const float4 p = make_float4(plane[0], plane[1], plane[2], plane[3]);
    const int64_t m_in = P.counts[(size_t) best];
    if ((rc = plane_grow(c, &P.d_terms, &P.terms_floats, 9 * m_in)))  // (term j of inlier r at j * m_in + r)
      return rc;
    hipLaunchKernelGGL(k_plane_count, dim3((unsigned) nblk), dim3(256), 0, st, xyz, sf, n, p, thr, P.d_blk);
    hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(1024), 0, st, (const int*) P.d_blk, (int) nblk, P.d_blk_off, P.d_hdr);
    hipLaunchKernelGGL(k_plane_terms, dim3((unsigned) nblk), dim3(256), 0, st, xyz, sf, n, p, thr, (const int*) P.d_blk_off,
      P.d_terms, m_in);
    hipLaunchKernelGGL(k_plane_moments, dim3(1), dim3(256), 0, st, (const float*) P.d_terms, m_in, (const PlaneHdr*) P.d_hdr,
      P.d_accu);
    AGH_HIPCHK(c, hipGetLastError());
    float accu[9];
    AGH_HIPCHK(c, hipMemcpyAsync(accu, P.d_accu, sizeof(accu), hipMemcpyDeviceToHost, st));
    AGH_HIPCHK(c, hipMemcpyAsync(&hdr, P.d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    AGH_HIPCHK(c, hipStreamSynchronize(st));
    if (hdr.n_in != m_in)
    {
      c->err = "agh_remove_plane: the inliers of the chosen plane do not match its score";
      return AGH_ERR_HIP;
    }
    plane_refit(accu, m_in, plane);
  }

  // 4. reselection with the final plane; the other points become the context's cloud
  const int slot = (P.d_xyz[0] && (const float*) P.d_xyz[0] == xyz) ? 1 : 0;
  if (P.out_cap[slot] < n)
  {
    if ((rc = dev_alloc(c, &P.d_xyz[slot], (size_t) n * 3)) || (rc = dev_alloc(c, &P.d_cam[slot], (size_t) n)))
      return rc;
    P.out_cap[slot] = n;
  }
  const float4 p = make_float4(plane[0], plane[1], plane[2], plane[3]);
  hipLaunchKernelGGL(k_plane_count, dim3((unsigned) nblk), dim3(256), 0, st, xyz, sf, n, p, thr, P.d_blk);
  hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(1024), 0, st, (const int*) P.d_blk, (int) nblk, P.d_blk_off, P.d_hdr);
  hipLaunchKernelGGL(k_plane_split, dim3((unsigned) nblk), dim3(256), 0, st, xyz, sf, n, cam, p, thr, (const int*) P.d_blk_off,
    P.d_idx, P.d_xyz[slot], P.d_cam[slot], pp->cam_ids_by_position ? 1 : 0);
  AGH_HIPCHK(c, hipGetLastError());
  AGH_HIPCHK(c, hipMemcpyAsync(&hdr, P.d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
  AGH_HIPCHK(c, hipStreamSynchronize(st));
  const int64_t n_in = hdr.n_in;
  const int64_t kept = n - n_in;
  rc = agh_set_cloud_device(ctx, P.d_xyz[slot], 12, P.d_cam[slot], kept, nullptr);
  if (rc != AGH_OK)
    return rc;
  c->cloud_async = true;  // (the grid build is queued on the context's stream, as after agh_set_cloud)
  P.has_result = true;
  P.n_inliers = n_in;
  std::memcpy(result->coefficients, plane, sizeof(plane));
  result->n_inliers = n_in;
  result->n_remaining = kept;
  result->found = 1;
  return AGH_OK;
}

int agh_get_plane_inliers(agh_ctx* ctx, int32_t* idx, int64_t cap)
{
  if (!ctx || cap < 0)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_plane_inliers"))
    return AGH_ERR_STATE;
  if (!c->plane || !c->plane->has_result)
  {
    c->err = "agh_get_plane_inliers: no agh_remove_plane result";
    return AGH_ERR_STATE;
  }
  const PlaneState& P = *c->plane;
  if (idx && P.n_inliers > cap)
  {
    c->err = "agh_get_plane_inliers: buffer too small";
    return AGH_ERR_CAPACITY;
  }
  if (idx && P.n_inliers > 0)
  {
    AGH_HIPCHK(c, hipSetDevice(c->device));
    AGH_HIPCHK(c, hipMemcpyAsync(idx, P.d_idx, sizeof(int32_t) * (size_t) P.n_inliers, hipMemcpyDeviceToHost, c->stream));
    AGH_HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return (int) P.n_inliers;
}

int agh_get_plane_candidates(agh_ctx* ctx, float* planes, int32_t* samples, int64_t* counts, int64_t cap)
{
  if (!ctx || cap < 0)
    return AGH_ERR_INVALID_ARGUMENT;
  Ctx* c = &ctx->c;
  if (refuse_mid_chain(c, "agh_get_plane_candidates"))
    return AGH_ERR_STATE;
  if (!c->plane || !c->plane->has_result)
  {
    c->err = "agh_get_plane_candidates: no agh_remove_plane result";
    return AGH_ERR_STATE;
  }
  const PlaneState& P = *c->plane;
  const int64_t k = std::min<int64_t>(cap, (int64_t) P.cand.size());
  for (int64_t i = 0; i < k; i++)
  {
    if (planes)
      std::memcpy(planes + 4 * i, P.cand[(size_t) i].c, sizeof(float) * 4);
    if (samples)
      std::memcpy(samples + 3 * i, P.cand[(size_t) i].s, sizeof(int32_t) * 3);
    if (counts)
      counts[i] = P.counts[(size_t) i];
  }
  return (int) P.cand.size();
}
