// plane_ref.cpp -- the contract of agh_remove_plane: PCL 1.7's plane segmentation as localization.cpp:51-98 configures it
// (SACMODEL_PLANE, SAC_RANSAC, setMaxIterations(100), setDistanceThreshold(0.01), setOptimizeCoefficients(true); PCL's
// defaults: fixed seed 12345, probability 0.99, max_sample_checks_ 1000), restated as plain sequential host code and
// followed by ExtractIndices::setNegative(true).  It is written from the PCL 1.7 sources as DESIGN.md ("Table-plane
// removal") restates them, and is NOT pinned against a PCL build.  Where Eigen's association order is not known the order
// written here is the contract (DESIGN.md lists each one).
//
// Build: g++ -O2 -std=c++11 -ffp-contract=off -fPIC -shared (IEEE arithmetic, no contraction, the host's libm for
// atan2f / cosf / sinf / sqrtf / log / pow -- the same functions libagile_grasp_hip.so's host side calls).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace
{

// boost::mt19937 (MT19937, Matsumoto & Nishimura 1998)
struct Mt19937
{
  uint32_t mt[624];
  int mti;
  explicit Mt19937(uint32_t seed)
  {
    mt[0] = seed;
    for (int i = 1; i < 624; i++)
      mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t) i;
    mti = 624;
  }
  uint32_t next()
  {
    if (mti >= 624)
    {
      int kk;
      for (kk = 0; kk < 624 - 397; kk++)
      {
        const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
        mt[kk] = mt[kk + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      for (; kk < 623; kk++)
      {
        const uint32_t y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
        mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      const uint32_t y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
      mt[623] = mt[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      mti = 0;
    }
    uint32_t y = mt[mti++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
  // boost::variate_generator<mt19937&, uniform_int<>(0, INT_MAX)>: 2^32 outcomes onto 2^31 values, bucket size 2
  int rnd() { return (int) (next() >> 1); }
};

struct Pt4
{
  float v[4];  // getArray4fMap: x, y, z, 1
};

struct Model
{
  const float* xyz;  // packed
  int64_t n;
  std::vector<int> shuffled;  // shuffled_indices_: iota(N), persistent across draws
  Mt19937 rng;
  Model(const float* p, int64_t count, uint32_t seed) : xyz(p), n(count), shuffled((size_t) count), rng(seed)
  {
    for (int64_t i = 0; i < n; i++)
      shuffled[(size_t) i] = (int) i;
  }
  Pt4 pt(int i) const
  {
    Pt4 p;
    p.v[0] = xyz[3 * (size_t) i], p.v[1] = xyz[3 * (size_t) i + 1], p.v[2] = xyz[3 * (size_t) i + 2], p.v[3] = 1.0f;
    return p;
  }
  void drawIndexSample(int s[3])
  {
    const size_t index_size = shuffled.size();
    for (unsigned i = 0; i < 3; i++)
      std::swap(shuffled[i], shuffled[i + ((size_t) rng.rnd() % (index_size - i))]);
    std::copy(shuffled.begin(), shuffled.begin() + 3, s);
  }
  // (p1 - p0) / (p2 - p0) on 4-float arrays
  void ratios(const int s[3], float d[4]) const
  {
    const Pt4 p0 = pt(s[0]), p1 = pt(s[1]), p2 = pt(s[2]);
    for (int k = 0; k < 4; k++)
      d[k] = (p1.v[k] - p0.v[k]) / (p2.v[k] - p0.v[k]);
  }
  bool isSampleGood(const int s[3]) const
  {
    float d[4];
    ratios(s, d);
    return (d[0] != d[1]) || (d[2] != d[1]);
  }
  // getSamples: false = the selection is empty
  bool getSamples(int s[3])
  {
    if (n < 3)
      return false;
    for (int iter = 0; iter < 1000; iter++)
    {
      drawIndexSample(s);
      if (isSampleGood(s))
        return true;
    }
    return false;
  }
  bool computeModelCoefficients(const int s[3], float c[4]) const
  {
    float d[4];
    ratios(s, d);
    if ((d[0] == d[1]) && (d[2] == d[1]))
      return false;
    const Pt4 p0 = pt(s[0]), p1 = pt(s[1]), p2 = pt(s[2]);
    float p1p0[4], p2p0[4];
    for (int k = 0; k < 4; k++)
      p1p0[k] = p1.v[k] - p0.v[k], p2p0[k] = p2.v[k] - p0.v[k];
    c[0] = p1p0[1] * p2p0[2] - p1p0[2] * p2p0[1];
    c[1] = p1p0[2] * p2p0[0] - p1p0[0] * p2p0[2];
    c[2] = p1p0[0] * p2p0[1] - p1p0[1] * p2p0[0];
    c[3] = 0.0f;
    // normalize(): divide by sqrt of the squared norm, summed as a 4-float packet reduction ((0 + 2) + (1 + 3))
    const float norm = std::sqrt((c[0] * c[0] + c[2] * c[2]) + (c[1] * c[1] + c[3] * c[3]));
    for (int k = 0; k < 4; k++)
      c[k] = c[k] / norm;
    c[3] = -1.0f * dot4(c, p0.v);
    return true;
  }
  // Vector4f dot in the same packet order
  static float dot4(const float a[4], const float b[4]) { return (a[0] * b[0] + a[2] * b[2]) + (a[1] * b[1] + a[3] * b[3]); }
  // float distance against the double threshold
  bool within(const float c[4], int i, double threshold) const
  {
    const Pt4 p = pt(i);
    return std::fabs(dot4(c, p.v)) < threshold;
  }
  int64_t countWithinDistance(const float c[4], double threshold) const
  {
    int64_t k = 0;
    for (int64_t i = 0; i < n; i++)
      k += within(c, (int) i, threshold) ? 1 : 0;
    return k;
  }
  void selectWithinDistance(const float c[4], double threshold, std::vector<int>& out) const
  {
    out.clear();
    for (int64_t i = 0; i < n; i++)
      if (within(c, (int) i, threshold))
        out.push_back((int) i);
  }
};

void computeRoots2(float b, float c, float roots[3])
{
  roots[0] = 0.0f;
  float d = (float) (b * b - 4.0 * c);
  if (d < 0.0)
    d = 0.0f;
  const float sd = std::sqrt(d);
  roots[2] = 0.5f * (b + sd);
  roots[1] = 0.5f * (b - sd);
}

void computeRoots(const float m[3][3], float roots[3])
{
  const float c0 = m[0][0] * m[1][1] * m[2][2] + 2.0f * m[0][1] * m[0][2] * m[1][2] - m[0][0] * m[1][2] * m[1][2] -
    m[1][1] * m[0][2] * m[0][2] - m[2][2] * m[0][1] * m[0][1];
  const float c1 = m[0][0] * m[1][1] - m[0][1] * m[0][1] + m[0][0] * m[2][2] - m[0][2] * m[0][2] + m[1][1] * m[2][2] -
    m[1][2] * m[1][2];
  const float c2 = m[0][0] + m[1][1] + m[2][2];
  if (std::fabs(c0) < std::numeric_limits<float>::epsilon())
  {
    computeRoots2(c2, c1, roots);
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
    computeRoots2(c2, c1, roots);
}

void eigen33(const float mat[3][3], float vec[3])
{
  float scale = 0.0f;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      scale = std::max(scale, std::fabs(mat[i][j]));
  if (scale <= std::numeric_limits<float>::min())
    scale = 1.0f;
  float s[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      s[i][j] = mat[i][j] / scale;
  float ev[3];
  computeRoots(s, ev);
  for (int i = 0; i < 3; i++)
    s[i][i] -= ev[0];
  float v[3][3];  // row0 x row1, row0 x row2, row1 x row2
  const int pairs[3][2] = { { 0, 1 }, { 0, 2 }, { 1, 2 } };
  float len[3];
  for (int k = 0; k < 3; k++)
  {
    const float* a = s[pairs[k][0]];
    const float* b = s[pairs[k][1]];
    v[k][0] = a[1] * b[2] - a[2] * b[1];
    v[k][1] = a[2] * b[0] - a[0] * b[2];
    v[k][2] = a[0] * b[1] - a[1] * b[0];
    len[k] = v[k][0] * v[k][0] + (v[k][1] * v[k][1] + v[k][2] * v[k][2]);  // Vector3f squaredNorm: x + (y + z)
  }
  int pick = 2;
  if (len[0] >= len[1] && len[0] >= len[2])
    pick = 0;
  else if (len[1] >= len[0] && len[1] >= len[2])
    pick = 1;
  const float r = std::sqrt(len[pick]);
  for (int k = 0; k < 3; k++)
    vec[k] = v[pick][k] / r;
}

// optimizeModelCoefficients
void optimize(const Model& m, const std::vector<int>& inliers, const float in[4], float out[4])
{
  if (inliers.size() < 4)
  {
    std::memcpy(out, in, sizeof(float) * 4);
    return;
  }
  float accu[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };  // computeMeanAndCovarianceMatrix: one float pass in inlier order
  for (size_t k = 0; k < inliers.size(); k++)
  {
    const Pt4 p = m.pt(inliers[k]);
    const float x = p.v[0], y = p.v[1], z = p.v[2];
    accu[0] += x * x;
    accu[1] += x * y;
    accu[2] += x * z;
    accu[3] += y * y;
    accu[4] += y * z;
    accu[5] += z * z;
    accu[6] += x;
    accu[7] += y;
    accu[8] += z;
  }
  const float count = (float) inliers.size();
  for (int k = 0; k < 9; k++)
    accu[k] = accu[k] / count;
  float cov[3][3];
  cov[0][0] = accu[0] - accu[6] * accu[6];
  cov[0][1] = accu[1] - accu[6] * accu[7];
  cov[0][2] = accu[2] - accu[6] * accu[8];
  cov[1][1] = accu[3] - accu[7] * accu[7];
  cov[1][2] = accu[4] - accu[7] * accu[8];
  cov[2][2] = accu[5] - accu[8] * accu[8];
  cov[1][0] = cov[0][1];
  cov[2][0] = cov[0][2];
  cov[2][1] = cov[1][2];
  float v[3];
  eigen33(cov, v);
  out[0] = v[0], out[1] = v[1], out[2] = v[2], out[3] = 0.0f;
  const float centroid[4] = { accu[6], accu[7], accu[8], 1.0f };
  out[3] = -1.0f * Model::dot4(out, centroid);
}

}  // namespace

extern "C" {

// the generator as RANSAC draws from it: rnd() = mt19937() >> 1
void pr_rnd(uint32_t seed, int64_t n, uint32_t* out)
{
  Mt19937 g(seed);
  for (int64_t i = 0; i < n; i++)
    out[i] = (uint32_t) g.rnd();
}

// SACSegmentation::segment + ExtractIndices(negative).  Candidates: every model RANSAC scored, in order (cap of them
// recorded); best: the one chosen (-1: none).  Returns 1 if a model was found.  inlier_mask[i] = 1 for PCL's
// inliers->indices; the kept cloud is the others in order.
int pr_segment(const float* xyz, int64_t n, int32_t max_iterations, double threshold, double probability, uint32_t seed,
  int32_t optimize_coefficients, float* cand_planes, int32_t* cand_samples, int64_t* cand_counts, int32_t cap,
  int32_t* n_cand, int32_t* best, int32_t* iterations, float* coefficients, uint8_t* inlier_mask)
{
  Model m(xyz, n, seed);
  // RandomSampleConsensus::computeModel
  int it = 0;
  int64_t n_best = -INT_MAX;
  double k = 1.0;
  const double log_probability = std::log(1.0 - probability);
  const double one_over_indices = 1.0 / (double) n;
  unsigned skipped = 0;
  const unsigned max_skip = (unsigned) max_iterations * 10;
  int chosen = -1, scored = 0;
  float model[4] = { 0, 0, 0, 0 };
  while (it < k && skipped < max_skip)
  {
    int s[3];
    if (!m.getSamples(s))
      break;
    float c[4];
    if (!m.computeModelCoefficients(s, c))
    {
      ++skipped;
      continue;
    }
    const int64_t count = m.countWithinDistance(c, threshold);
    if (scored < cap)
    {
      std::memcpy(cand_planes + 4 * scored, c, sizeof(c));
      std::memcpy(cand_samples + 3 * scored, s, sizeof(s));
      cand_counts[scored] = count;
    }
    if (count > n_best)
    {
      n_best = count;
      chosen = scored;
      std::memcpy(model, c, sizeof(c));
      const double w = (double) n_best * one_over_indices;
      double p_no_outliers = 1.0 - std::pow(w, 3.0);
      p_no_outliers = std::max(std::numeric_limits<double>::epsilon(), p_no_outliers);
      p_no_outliers = std::min(1.0 - std::numeric_limits<double>::epsilon(), p_no_outliers);
      k = log_probability / std::log(p_no_outliers);
    }
    scored++;
    ++it;
    if (it > max_iterations)
      break;
  }
  *n_cand = scored;
  *best = chosen;
  *iterations = it;
  std::memset(inlier_mask, 0, (size_t) n);
  if (chosen < 0)
    return 0;
  std::vector<int> inliers;
  m.selectWithinDistance(model, threshold, inliers);
  float final_c[4];
  std::memcpy(final_c, model, sizeof(model));
  if (optimize_coefficients)
  {
    optimize(m, inliers, model, final_c);
    m.selectWithinDistance(final_c, threshold, inliers);
  }
  std::memcpy(coefficients, final_c, sizeof(final_c));
  for (size_t q = 0; q < inliers.size(); q++)
    inlier_mask[inliers[q]] = 1;
  return 1;
}

}  // extern "C"
