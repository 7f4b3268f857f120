// plane_fit.hip -- the support plane of a fitted clustered chain (include/agh.h, agh_localize_clustered_fit*; DESIGN.md, "A fitted
// plane for the clustered chain").
//
// agh_localize_clustered* takes the plane from the caller; here it comes from the voxelised cloud itself, by a finder made for the
// device (plane.hip restates PCL's serial RANSAC for agh_remove_plane, which is no stage of a chain):
//   k_fit_candidates    a thread per candidate: three voxels by splitmix64, their plane; the counts and sums zeroed
//   k_fit_score         every voxel read once, kFitPts per thread in registers; the <= 256 planes in LDS; hits by ballot + popcount
//                       per wave, kept in a lane's register, LDS integer atomics once per wave and candidate, then one global
//                       integer atomic per work-group and candidate
//   k_fit_moments       the arg-max of the counts again per work-group; the chosen candidate's inliers as 16.16 fixed-point
//                       differences against its p0: int64 wave reductions, LDS, ten 64-bit global atomics per work-group
//   k_fit_finish        one work-group: the arg-max, one lane the eigenvector (smallest_eigvec3), the orientation, the ClusterDev
//                       record in device memory that the cluster kernels read, and the result record in pinned memory
// Everything is queued on the chain's stream behind the preprocessing and in front of the cluster stage (sample_cluster.hip);
// launches are sized from the raw point count, the voxel count is read on the device (label_voxels); no launch count depends on
// C or N, nothing returns to the host.
//
// A fitted batch (agh_localize_batch_clustered_fit*; DESIGN.md, "A fitted plane in the batch chains") runs the same four bodies
// (fit_candidates, fit_score, fit_moments, fit_finish: __device__ functions, one copy of the arithmetic) with the capture on
// blockIdx.y: k_fit_*_batch read capture k's parameters and origin from a device table of PlaneFitDev, its voxel count from its
// own descriptor and its points at cloud_off[k] of the common voxel array, keep its candidates, counts and sums in block k of an
// array of PlaneFitBuffers, and write the plane into record k of the cluster stage's table.  One launch per step whatever
// n_captures and C_k are.
//
// Nothing depends on the order of an atomic operation: counts and sums are integers (no float atomic anywhere), the arg-max keys
// are distinct.
#include "agh_internal.h"
#include "taubin_eigen.h"

#include <cmath>

namespace agh
{

constexpr int kFitPts = 2;                    // voxels per thread of k_fit_score and k_fit_moments
constexpr int kFitTile = 256 * kFitPts;       // ... and per work-group
constexpr long long kFitMaxRefit = 1ll << 24; // contributors beyond which the refit is skipped (the sums' overflow bound)
static_assert(kPlaneFitMaxCandidates == 256, "a thread per candidate of a 256-thread work-group");

// ((a x + b y) + c z) + d in double on the float coordinates, left to right: cluster_foreground's evaluation order
__device__ __forceinline__ double fit_height(double a, double b, double c, double d, float x, float y, float z)
{
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a, (double) x), __dmul_rn(b, (double) y)), __dmul_rn(c, (double) z)), d);
}

// One work-group of 256.  counts and sums zeroed for the kernels behind this one; candidate tid < C drawn and its plane formed
// (rules 1 and 2): an invalid candidate's plane is zeros, and with N < 3 its indices are -1.
// xyz: the cloud's first voxel, N its voxels (a capture of a batch: its own, whatever lies beside them in the array).
__device__ __forceinline__ void fit_candidates(const float* __restrict__ xyz, int64_t stride, int64_t N, const PlaneFitDev& fp,
  PlaneFitBuffers* __restrict__ fb)
{
  const int c = threadIdx.x;
  fb->counts[c] = 0u;
  if (c < 16)
    fb->sums[c] = 0ull;
  if (c >= fp.C)
    return;
  double pl[4] = { 0.0, 0.0, 0.0, 0.0 };
  int32_t id[3] = { -1, -1, -1 };
  if (N >= 3)
  {
    double p[3][3];
#pragma unroll
    for (int s = 0; s < 3; s++)
    {
      const unsigned long long k = (unsigned long long) (3 * c + s);
      id[s] = (int32_t) (splitmix64(fp.seed ^ (k * 0x9E3779B97F4A7C15ull)) % (unsigned long long) N);  // (< N <= n: inside the cloud)
      const float* q = xyz + (int64_t) id[s] * stride;
      p[s][0] = (double) q[0];
      p[s][1] = (double) q[1];
      p[s][2] = (double) q[2];
    }
    const double ux = __dsub_rn(p[1][0], p[0][0]), uy = __dsub_rn(p[1][1], p[0][1]), uz = __dsub_rn(p[1][2], p[0][2]);
    const double vx = __dsub_rn(p[2][0], p[0][0]), vy = __dsub_rn(p[2][1], p[0][1]), vz = __dsub_rn(p[2][2], p[0][2]);
    const double nx = __dsub_rn(__dmul_rn(uy, vz), __dmul_rn(uz, vy));
    const double ny = __dsub_rn(__dmul_rn(uz, vx), __dmul_rn(ux, vz));
    const double nz = __dsub_rn(__dmul_rn(ux, vy), __dmul_rn(uy, vx));
    const double l2 = __dadd_rn(__dadd_rn(__dmul_rn(nx, nx), __dmul_rn(ny, ny)), __dmul_rn(nz, nz));
    if (isfinite(l2) && l2 > 0.0)
    {
      const double l = __dsqrt_rn(l2);
      pl[0] = __ddiv_rn(nx, l);
      pl[1] = __ddiv_rn(ny, l);
      pl[2] = __ddiv_rn(nz, l);
      pl[3] = -__dadd_rn(__dadd_rn(__dmul_rn(pl[0], p[0][0]), __dmul_rn(pl[1], p[0][1])), __dmul_rn(pl[2], p[0][2]));
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
    fb->planes[c][k] = pl[k];
#pragma unroll
  for (int s = 0; s < 3; s++)
    fb->idx[c][s] = id[s];
}

__global__ __launch_bounds__(256) void k_fit_candidates(const float* __restrict__ xyz, int64_t stride, const VoxDesc* __restrict__ d,
  int64_t n, PlaneFitDev fp, PlaneFitBuffers* __restrict__ fb)
{
  fit_candidates(xyz, stride, label_voxels(d, n), fp, fb);
}

// ... for capture blockIdx.y of a batch: its record of the device table (uniform per work-group: scalar loads, as the cluster
// kernels' ClusterDev), its voxels at cloud_off[k] (none for a capture whose descriptor carries an error: label_voxels), block k
__global__ __launch_bounds__(256) void k_fit_candidates_batch(VoxBatch vb, const float* __restrict__ xyz, int64_t stride,
  const int* __restrict__ cloud_off, const PlaneFitDev* __restrict__ fps, PlaneFitBuffers* __restrict__ fbs)
{
  const int k = blockIdx.y;
  const PlaneFitDev fp = fps[k];
  fit_candidates(xyz + (int64_t) cloud_off[k] * stride, stride, label_voxels(vb.desc + k, vb.cap[k].n), fp, fbs + k);
}

// The voxels of this thread: v = v0 + k * 256 + tid, k < kFitPts (a wave reads a run of 64 records per k); a position at or
// beyond N holds NaN, which is no plane's inlier.
__device__ __forceinline__ void fit_load_voxels(const float* __restrict__ xyz, int64_t stride, int64_t v0, int64_t N, float (&x)[kFitPts],
  float (&y)[kFitPts], float (&z)[kFitPts])
{
#pragma unroll
  for (int k = 0; k < kFitPts; k++)
  {
    const int64_t v = v0 + k * 256 + threadIdx.x;
    x[k] = y[k] = z[k] = __int_as_float(0x7fc00000);
    if (v < N)
    {
      const float* q = xyz + v * stride;
      x[k] = q[0];
      y[k] = q[1];
      z[k] = q[2];
    }
  }
}

// Rule 3.  (an invalid candidate, plane zeros, gets a NaN offset in LDS: no inlier)
__device__ __forceinline__ void fit_score(const float* __restrict__ xyz, int64_t stride, int64_t N, const PlaneFitDev& fp,
  PlaneFitBuffers* __restrict__ fb)
{
  __shared__ double pl[kPlaneFitMaxCandidates][4];
  __shared__ unsigned cnt[kPlaneFitMaxCandidates];
  const int64_t v0 = (int64_t) blockIdx.x * kFitTile;
  if (v0 >= N)  // (uniform: the launch is sized from the raw points -- in a batch from the largest capture's)
    return;
  const int tid = threadIdx.x;
  if (tid < fp.C)
  {
    const double a = fb->planes[tid][0], b = fb->planes[tid][1], c = fb->planes[tid][2];
    pl[tid][0] = a;
    pl[tid][1] = b;
    pl[tid][2] = c;
    pl[tid][3] = (a == 0.0 && b == 0.0 && c == 0.0) ? __longlong_as_double(0x7ff8000000000000ll) : fb->planes[tid][3];
  }
  cnt[tid] = 0u;
  float x[kFitPts], y[kFitPts], z[kFitPts];
  fit_load_voxels(xyz, stride, v0, N, x, y, z);
  __syncthreads();
  // (a wave's hits of candidate c are wave-uniform: lane c % 64 keeps them in a register, so the loop holds no memory operation
  // but the LDS reads of the plane; the four waves meet in LDS afterwards)
  unsigned mine[kPlaneFitMaxCandidates / 64] = { 0u, 0u, 0u, 0u };
  const int lane = tid & 63;
#pragma unroll
  for (int q = 0; q < kPlaneFitMaxCandidates / 64; q++)
    for (int c = 64 * q; c < min(fp.C, 64 * q + 64); c++)  // (uniform)
    {
      const double a = pl[c][0], b = pl[c][1], cc = pl[c][2], dd = pl[c][3];
      int hits = 0;
#pragma unroll
      for (int k = 0; k < kFitPts; k++)
        hits += __popcll(__ballot(fabs(fit_height(a, b, cc, dd, x[k], y[k], z[k])) <= fp.threshold));
      mine[q] += lane == (c & 63) ? (unsigned) hits : 0u;
    }
#pragma unroll
  for (int q = 0; q < kPlaneFitMaxCandidates / 64; q++)
    if (mine[q])
      atomicAdd(&cnt[64 * q + lane], mine[q]);
  __syncthreads();
  if (tid < fp.C && cnt[tid])
    atomicAdd(&fb->counts[tid], cnt[tid]);
}

__global__ __launch_bounds__(256) void k_fit_score(const float* __restrict__ xyz, int64_t stride, const VoxDesc* __restrict__ d,
  int64_t n, PlaneFitDev fp, PlaneFitBuffers* __restrict__ fb)
{
  fit_score(xyz, stride, label_voxels(d, n), fp, fb);
}

__global__ __launch_bounds__(256) void k_fit_score_batch(VoxBatch vb, const float* __restrict__ xyz, int64_t stride,
  const int* __restrict__ cloud_off, const PlaneFitDev* __restrict__ fps, PlaneFitBuffers* __restrict__ fbs)
{
  const int k = blockIdx.y;
  const PlaneFitDev fp = fps[k];
  fit_score(xyz + (int64_t) cloud_off[k] * stride, stride, label_voxels(vb.desc + k, vb.cap[k].n), fp, fbs + k);
}

// Rule 4, by the whole work-group of 256: the largest key (count << 32) | (0xFFFFFFFF - c) over c < C -- the keys are distinct,
// ties go to the smaller c.  part: four words of LDS.
__device__ __forceinline__ unsigned long long fit_best_key(const unsigned* counts, int C, unsigned long long* part)
{
  const int tid = threadIdx.x;
  unsigned long long key = 0ull;
  if (tid < C)
    key = ((unsigned long long) counts[tid] << 32) | (unsigned long long) (0xFFFFFFFFu - (unsigned) tid);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
  {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((tid & 63) == 0)
    part[tid >> 6] = key;
  __syncthreads();
  unsigned long long best = part[0];
#pragma unroll
  for (int w = 1; w < 4; w++)
    best = part[w] > best ? part[w] : best;
  return best;
}

// Rule 5's sums over the chosen candidate's inliers (the scoring has ended: the counts are final).
__device__ __forceinline__ void fit_moments(const float* __restrict__ xyz, int64_t stride, int64_t N, const PlaneFitDev& fp,
  PlaneFitBuffers* __restrict__ fb)
{
  __shared__ unsigned long long part[4];
  __shared__ unsigned long long acc[10];
  const int64_t v0 = (int64_t) blockIdx.x * kFitTile;
  if (v0 >= N || !fp.refine)  // (uniform)
    return;
  const int tid = threadIdx.x;
  if (tid < 10)
    acc[tid] = 0ull;
  const unsigned long long key = fit_best_key(fb->counts, fp.C, part);  // (its barrier covers acc)
  const long long count = (long long) (key >> 32);
  if (count < (long long) max(fp.min_inliers, 3))  // (not found: uniform)
    return;
  const int best = (int) (0xFFFFFFFFu - (unsigned) (key & 0xFFFFFFFFull));
  const double a = fb->planes[best][0], b = fb->planes[best][1], c = fb->planes[best][2], dd = fb->planes[best][3];
  const float* q0 = xyz + (int64_t) fb->idx[best][0] * stride;  // (found: the candidate is valid, its indices inside the cloud)
  const float x0 = q0[0], y0 = q0[1], z0 = q0[2];
  float x[kFitPts], y[kFitPts], z[kFitPts];
  fit_load_voxels(xyz, stride, v0, N, x, y, z);
  long long s[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
  for (int k = 0; k < kFitPts; k++)
  {
    const float dx = __fsub_rn(x[k], x0), dy = __fsub_rn(y[k], y0), dz = __fsub_rn(z[k], z0);
    if (fabs(fit_height(a, b, c, dd, x[k], y[k], z[k])) <= fp.threshold && fabsf(dx) < 8.f && fabsf(dy) < 8.f && fabsf(dz) < 8.f)
    {
      // (|q| < 2^19: no product beyond 2^38, no sum of 2^24 of them beyond 2^62)
      const long long qx = (long long) rint(__dmul_rn((double) dx, 65536.0)), qy = (long long) rint(__dmul_rn((double) dy, 65536.0)),
                      qz = (long long) rint(__dmul_rn((double) dz, 65536.0));
      s[0] += 1;
      s[1] += qx;
      s[2] += qy;
      s[3] += qz;
      s[4] += qx * qx;
      s[5] += qx * qy;
      s[6] += qx * qz;
      s[7] += qy * qy;
      s[8] += qy * qz;
      s[9] += qz * qz;
    }
  }
  if (__ballot(s[0] != 0))  // (wave-uniform)
  {
#pragma unroll
    for (int j = 0; j < 10; j++)
    {
      long long t = s[j];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1)
        t += __shfl_xor(t, o);
      if ((tid & 63) == 0)
        atomicAdd(&acc[j], (unsigned long long) t);  // (two's complement: the wrap of a negative partial sum cancels in the total)
    }
  }
  __syncthreads();
  if (tid < 10 && acc[tid])
    atomicAdd(&fb->sums[tid], acc[tid]);
}

__global__ __launch_bounds__(256) void k_fit_moments(const float* __restrict__ xyz, int64_t stride, const VoxDesc* __restrict__ d,
  int64_t n, PlaneFitDev fp, PlaneFitBuffers* __restrict__ fb)
{
  fit_moments(xyz, stride, label_voxels(d, n), fp, fb);
}

__global__ __launch_bounds__(256) void k_fit_moments_batch(VoxBatch vb, const float* __restrict__ xyz, int64_t stride,
  const int* __restrict__ cloud_off, const PlaneFitDev* __restrict__ fps, PlaneFitBuffers* __restrict__ fbs)
{
  const int k = blockIdx.y;
  const PlaneFitDev fp = fps[k];
  fit_moments(xyz + (int64_t) cloud_off[k] * stride, stride, label_voxels(vb.desc + k, vb.cap[k].n), fp, fbs + k);
}

// One work-group of 256 for the arg-max; lane 0 does rules 4 to 6 and returns true with the plane the cluster kernels are to read
// (NaN without one: every voxel background) and the result record.
__device__ __forceinline__ bool fit_finish(const float* __restrict__ xyz, int64_t stride, int64_t N, const PlaneFitDev& fp,
  const PlaneFitBuffers* fb, double (&pl)[4], agh_plane_fit_result& r)
{
  __shared__ unsigned long long part[4];
  const unsigned long long key = fit_best_key(fb->counts, fp.C, part);
  if (threadIdx.x != 0)
    return false;
  const long long count = (long long) (key >> 32);
  const int best = (int) (0xFFFFFFFFu - (unsigned) (key & 0xFFFFFFFFull));
  const bool found = count >= (long long) max(fp.min_inliers, 3);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  pl[0] = pl[1] = pl[2] = pl[3] = nan;
  long long n_refit = 0;
  int refined = 0;
  if (found)
  {
#pragma unroll
    for (int k = 0; k < 4; k++)
      pl[k] = fb->planes[best][k];
    if (fp.refine)
    {
      n_refit = (long long) fb->sums[0];
      if (n_refit >= 3 && n_refit <= kFitMaxRefit)
      {
        const double Nn = (double) n_refit, w1 = 0x1p-16, w2 = 0x1p-32;
        double S[10];
#pragma unroll
        for (int j = 1; j < 10; j++)
          S[j] = (double) (long long) fb->sums[j];
        const double mx = __dmul_rn(__ddiv_rn(S[1], Nn), w1), my = __dmul_rn(__ddiv_rn(S[2], Nn), w1), mz = __dmul_rn(__ddiv_rn(S[3], Nn), w1);
        const double M[6] = { __dsub_rn(__dmul_rn(__ddiv_rn(S[4], Nn), w2), __dmul_rn(mx, mx)),
                              __dsub_rn(__dmul_rn(__ddiv_rn(S[5], Nn), w2), __dmul_rn(mx, my)),
                              __dsub_rn(__dmul_rn(__ddiv_rn(S[6], Nn), w2), __dmul_rn(mx, mz)),
                              __dsub_rn(__dmul_rn(__ddiv_rn(S[7], Nn), w2), __dmul_rn(my, my)),
                              __dsub_rn(__dmul_rn(__ddiv_rn(S[8], Nn), w2), __dmul_rn(my, mz)),
                              __dsub_rn(__dmul_rn(__ddiv_rn(S[9], Nn), w2), __dmul_rn(mz, mz)) };
        double axis[3];
        smallest_eigvec3(M, axis);
        if (isfinite(axis[0]) && isfinite(axis[1]) && isfinite(axis[2]))
        {
          const float* q0 = xyz + (int64_t) fb->idx[best][0] * stride;
          const double cx = __dadd_rn((double) q0[0], mx), cy = __dadd_rn((double) q0[1], my), cz = __dadd_rn((double) q0[2], mz);
          pl[0] = axis[0];
          pl[1] = axis[1];
          pl[2] = axis[2];
          pl[3] = -__dadd_rn(__dadd_rn(__dmul_rn(axis[0], cx), __dmul_rn(axis[1], cy)), __dmul_rn(axis[2], cz));
          refined = 1;
        }
      }
    }
    const double s = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(pl[0], fp.origin[0]), __dmul_rn(pl[1], fp.origin[1])),
                                 __dmul_rn(pl[2], fp.origin[2])), pl[3]);
    if (s < 0.0)
    {
#pragma unroll
      for (int k = 0; k < 4; k++)
        pl[k] = -pl[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
    r.plane[k] = found ? pl[k] : 0.0;
  r.n_voxels = N;
  r.n_inliers = count;
  r.n_refit = n_refit;
  r.best_candidate = count > 0 ? best : -1;
  r.found = found ? 1 : 0;
  r.refined = refined;
  r.reserved = 0;
  return true;
}

// ... lane 0 writes the record the cluster kernels read (cp with the plane in place) and the pinned result.
__global__ __launch_bounds__(256) void k_fit_finish(const float* __restrict__ xyz, int64_t stride, const VoxDesc* __restrict__ d,
  int64_t n, PlaneFitDev fp, ClusterDev cp, PlaneFitBuffers* __restrict__ fb, agh_plane_fit_result* __restrict__ h_result)
{
  double pl[4];
  agh_plane_fit_result r;
  if (!fit_finish(xyz, stride, label_voxels(d, n), fp, fb, pl, r))
    return;
#pragma unroll
  for (int k = 0; k < 4; k++)
    cp.plane[k] = pl[k];
  fb->record = cp;
  *h_result = r;
}

// ... a work-group per capture: lane 0 writes the plane into capture k's record of the cluster stage's table -- the plane only:
// bounds, tol2 and min_voxels are the uploaded record's -- and the pinned result[k].
__global__ __launch_bounds__(256) void k_fit_finish_batch(VoxBatch vb, const float* __restrict__ xyz, int64_t stride,
  const int* __restrict__ cloud_off, const PlaneFitDev* __restrict__ fps, const PlaneFitBuffers* __restrict__ fbs,
  ClusterDev* __restrict__ cps, agh_plane_fit_result* __restrict__ h_results)
{
  const int k = blockIdx.x;
  const PlaneFitDev fp = fps[k];
  double pl[4];
  agh_plane_fit_result r;
  if (!fit_finish(xyz + (int64_t) cloud_off[k] * stride, stride, label_voxels(vb.desc + k, vb.cap[k].n), fp, fbs + k, pl, r))
    return;
#pragma unroll
  for (int q = 0; q < 4; q++)
    cps[k].plane[q] = pl[q];
  h_results[k] = r;
}

std::string plane_fit_params_fault(const agh_plane_fit_params& fp)
{
  if (fp.n_candidates < 1 || fp.n_candidates > kPlaneFitMaxCandidates)
    return "n_candidates must be 1 .. 256";
  if (fp.refine != 0 && fp.refine != 1)
    return "refine must be 0 or 1";
  if (fp.min_inliers < 3)
    return "min_inliers must be >= 3";
  if (fp.reserved != 0)
    return "reserved must be 0";
  if (!std::isfinite(fp.distance_threshold) || !(fp.distance_threshold > 0.0) || fp.distance_threshold > 0.05)
    return "distance_threshold must be finite and in (0, 0.05]";
  return std::string();
}

int plane_fit_stage(Ctx* c, int64_t n, const agh_plane_fit_params& fp, const ClusterDev& cp, hipStream_t st, const ClusterDev** d_cp_out)
{
  if (!c->d_fit)
  {
    PlaneFitBuffers* fb = nullptr;
    if (int rc = dev_alloc(c, &fb, 1))
      return rc;
    c->d_fit = fb;
  }
  if (!c->h_fit_result && hipHostMalloc((void**) &c->h_fit_result, sizeof(agh_plane_fit_result), hipHostMallocDefault) != hipSuccess)
  {
    c->h_fit_result = nullptr;
    c->err = "hipHostMalloc failed (plane fit result)";
    return AGH_ERR_HIP;
  }
  PlaneFitBuffers* fb = static_cast<PlaneFitBuffers*>(c->d_fit);
  // (camera 0's origin in force: the table's only row, or the context's own; the setter refuses mid-chain)
  const double* o = c->cam_tab_rows == 1 ? c->h_cam_tab : c->p.cam_origin[0];
  const PlaneFitDev dev{ fp.n_candidates, fp.refine, fp.min_inliers, 0, fp.distance_threshold, (unsigned long long) fp.seed,
    { o[0], o[1], o[2] } };
  const VoxDesc* desc = (const VoxDesc*) c->d_vox_desc;
  // (the voxelised cloud is the context's bound cloud: the preprocessing queued in front of this stage bound it)
  const float* xyz = c->d_xyz;
  const int64_t stride = c->stride_floats;
  hipLaunchKernelGGL(k_fit_candidates, dim3(1), dim3(256), 0, st, xyz, stride, desc, n, dev, fb);
  if (n > 0)
  {
    const unsigned blocks = (unsigned) ((n + kFitTile - 1) / kFitTile);
    hipLaunchKernelGGL(k_fit_score, dim3(blocks), dim3(256), 0, st, xyz, stride, desc, n, dev, fb);
    hipLaunchKernelGGL(k_fit_moments, dim3(blocks), dim3(256), 0, st, xyz, stride, desc, n, dev, fb);
  }
  hipLaunchKernelGGL(k_fit_finish, dim3(1), dim3(256), 0, st, xyz, stride, desc, n, dev, cp, fb, c->h_fit_result);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "plane fit launch failed";
    return AGH_ERR_HIP;
  }
  *d_cp_out = &fb->record;
  return AGH_OK;
}

// The stage over a batch (BatchFitStage, agh_internal.h): four launches whatever C and the C_k are, sized from n_max; work-groups
// whose tile starts at or beyond their capture's N_k leave at once.  The ClusterDev table must be uploaded in front (on st).
int plane_fit_stage_batch(Ctx* c, const BatchFitStage& m, hipStream_t st)
{
  const unsigned Cy = (unsigned) m.C;
  // (the voxelised batch is the context's bound batch: the preprocessing queued in front of this stage bound it)
  const float* xyz = c->d_xyz;
  const int64_t stride = c->stride_floats;
  hipLaunchKernelGGL(k_fit_candidates_batch, dim3(1, Cy), dim3(256), 0, st, m.vb, xyz, stride, m.cloud_off, m.fps, m.fbs);
  if (m.n_max > 0)
  {
    const unsigned blocks = (unsigned) ((m.n_max + kFitTile - 1) / kFitTile);
    hipLaunchKernelGGL(k_fit_score_batch, dim3(blocks, Cy), dim3(256), 0, st, m.vb, xyz, stride, m.cloud_off, m.fps, m.fbs);
    hipLaunchKernelGGL(k_fit_moments_batch, dim3(blocks, Cy), dim3(256), 0, st, m.vb, xyz, stride, m.cloud_off, m.fps, m.fbs);
  }
  hipLaunchKernelGGL(k_fit_finish_batch, dim3(Cy), dim3(256), 0, st, m.vb, xyz, stride, m.cloud_off, m.fps,
    (const PlaneFitBuffers*) m.fbs, m.cps, m.h_results);
  if (hipGetLastError() != hipSuccess)
  {
    c->err = "plane fit launch failed";
    return AGH_ERR_HIP;
  }
  return AGH_OK;
}

}  // namespace agh
