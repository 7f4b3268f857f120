// cluster_fit_adapter_test.cpp -- runs the adapter's fitted clustered calls (include/agile_grasp_amd/localization.h):
//   cluster_fit_adapter_test gpu <capture.bin> <svm>   localizeHandlesClusteredFit against the C call (agh_localize_clustered_fit:
//                                                      the same plane, per object the same counts and handle records, the same
//                                                      sample list and object sizes), and a fitted call while a chain is pending
// capture.bin: int64 n, int64 size_left, n x 3 float32, double ws[6], double plane[4] (not read by the calls), double min_height,
// max_height, tolerance, int64 min_voxels, max_objects, n_samples, seed, double cam origins[2][3], int64 n_candidates, fit seed,
// double distance_threshold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_common.h"

int main(int argc, char** argv)
{
  if (argc < 4 || std::strcmp(argv[1], "gpu") != 0)
    return 2;
  FILE* f = std::fopen(argv[2], "rb");
  if (!f)
    return 2;
  long long n = 0, size_left = 0, iv[4];
  if (std::fread(&n, 8, 1, f) != 1 || std::fread(&size_left, 8, 1, f) != 1 || n < 1)
    return 2;
  std::vector<float> xyz((size_t) (3 * n));
  double ws[6], pl[7], org[6], threshold = 0.0;
  long long fv[2];
  if (std::fread(xyz.data(), 4, xyz.size(), f) != xyz.size() || std::fread(ws, 8, 6, f) != 6 || std::fread(pl, 8, 7, f) != 7 ||
      std::fread(iv, 8, 4, f) != 4 || std::fread(org, 8, 6, f) != 6 || std::fread(fv, 8, 2, f) != 2 || std::fread(&threshold, 8, 1, f) != 1)
    return 2;
  std::fclose(f);
  agh_cluster_params cp;
  agh_default_cluster_params(&cp);
  for (int k = 0; k < 4; k++)
    cp.plane[k] = pl[k];
  cp.min_height = pl[4];
  cp.max_height = pl[5];
  cp.tolerance = pl[6];
  cp.min_voxels = (std::int32_t) iv[0];
  cp.max_objects = (std::int32_t) iv[1];
  const long long n_samples = iv[2], seed = iv[3];
  const size_t K = (size_t) cp.max_objects;
  agh_plane_fit_params fp;
  agh_default_plane_fit_params(&fp);
  fp.n_candidates = (std::int32_t) fv[0];
  fp.seed = (std::uint64_t) fv[1];
  fp.distance_threshold = threshold;

  // the C call
  agh_params p;
  agh_default_params(&p);
  for (int k = 0; k < 2; k++)
    for (int r = 0; r < 3; r++)
      p.cam_origin[k][r] = org[3 * k + r];
  agh_ctx* ctx = nullptr;
  if (agh_create(&p, &ctx) != AGH_OK || agh_load_svm_file(ctx, argv[3]) != AGH_OK)
    return 3;
  agh_localize_params lp;
  std::memset(&lp, 0, sizeof(lp));
  lp.size_left = size_left;
  lp.dense = 1;
  lp.classify = 1;
  for (int i = 0; i < 6; i++)
    lp.workspace[i] = ws[i];
  lp.cell_size = 0.003;
  lp.n_samples = n_samples;
  lp.sample_seed = (std::uint64_t) seed;
  lp.min_inliers = 2;
  lp.min_length = 0.005;
  const std::int64_t cap = 8 * n_samples * (std::int64_t) K;
  std::vector<agh_handle> c_handles((size_t) cap);
  std::vector<std::int32_t> c_idx((size_t) cap), c_samples((size_t) n_samples * K);
  std::vector<agh_hypothesis> c_hands((size_t) cap);
  std::vector<agh_localize_batch_result> res(K);
  if (agh_localize_clustered_fit(ctx, xyz.data(), 12, n, &fp, &cp, &lp, c_handles.data(), cap, c_idx.data(), cap, c_hands.data(), cap,
        c_samples.data(), res.data()) != AGH_OK)
  {
    std::printf("agh_localize_clustered_fit: %s\n", agh_last_error(ctx));
    return 3;
  }
  agh_plane_fit_result fit;
  if (agh_get_plane_fit(ctx, &fit) != AGH_OK)
    return 3;
  agh_cluster_info info;
  std::vector<std::int64_t> m_c(K, -1);
  if (agh_get_cluster_info(ctx, &info, m_c.data(), nullptr, (std::int32_t) K) != AGH_OK)
    return 3;
  agh_destroy(ctx);
  long long c_kept = 0, c_n_handles = 0;
  for (size_t j = 0; j < K; j++)
  {
    c_kept += res[j].r.n_hands;
    c_n_handles += res[j].r.n_handles;
  }
  std::printf("C %lld %lld %lld %lld %d %d\n", c_kept, c_n_handles, (long long) info.n_objects, (long long) info.n_foreground, fit.found,
    fit.refined);

  PointCloud::Ptr cloud(new PointCloud);
  cloud->points.resize((size_t) n);
  cloud->is_dense = true;
  for (size_t i = 0; i < (size_t) n; i++)
  {
    cloud->points[i].x = xyz[3 * i];
    cloud->points[i].y = xyz[3 * i + 1];
    cloud->points[i].z = xyz[3 * i + 2];
  }
  Matrix4d tf[2];
  for (int k = 0; k < 2; k++)
    for (int r = 0; r < 3; r++)
      tf[k](r, 3) = org[3 * k + r];
  VectorXd w(6);
  for (int i = 0; i < 6; i++)
    w(i) = ws[i];
  Localization loc(1, false, 0);
  loc.setCameraTransforms(tf[0], tf[1]);
  loc.setWorkspace(w);
  loc.setDeterministicNormalEstimation(true);
  loc.setNumSamples((int) n_samples);
  loc.setSampleSeed((std::uint64_t) seed);
  loc.setClusterParams(cp.min_height, cp.max_height, cp.tolerance, cp.min_voxels, cp.max_objects);
  loc.setPlaneFitParams(fp.n_candidates, fp.distance_threshold, fp.min_inliers, fp.refine != 0, fp.seed);
  bool found_before = true;
  const VectorXd none = loc.fittedPlane(&found_before);  // (no chain yet: zeros)
  std::vector<std::vector<GraspHypothesis> > kept;
  PointCloud::Ptr cloud1(new PointCloud(*cloud));
  const std::vector<std::vector<Handle> > handles = loc.localizeHandlesClusteredFit(cloud1, (int) size_left, argv[3], 2, 0.005, &kept);
  bool found = false;
  const VectorXd plane = loc.fittedPlane(&found);
  bool same_plane = found && !found_before;
  for (int k = 0; k < 4; k++)
  {
    const double got = plane(k);
    same_plane = same_plane && std::memcmp(&fit.plane[k], &got, 8) == 0 && none(k) == 0.0;
  }
  const std::vector<int> list = loc.getLastSampleIndices();
  bool same_list = list.size() == c_samples.size();
  for (size_t i = 0; same_list && i < list.size(); i++)
    same_list = list[i] == c_samples[i];
  const std::vector<std::int64_t> m_a = loc.getClusterSizes();
  bool same_sizes = m_a.size() == K;
  for (size_t j = 0; same_sizes && j < K; j++)
    same_sizes = m_a[j] == m_c[j];
  bool same_handles = handles.size() == K && kept.size() == K;
  for (size_t j = 0; same_handles && j < K; j++)
  {
    same_handles = handles[j].size() == (size_t) res[j].r.n_handles && kept[j].size() == (size_t) res[j].r.n_hands;
    for (size_t i = 0; same_handles && i < handles[j].size(); i++)
    {
      const agh_handle& c = c_handles[(size_t) res[j].first_handle + i];
      for (int r = 0; same_handles && r < 3; r++)
        same_handles = handles[j][i].getAxis()(r) == c.axis[r] && handles[j][i].getCenter()(r) == c.center[r] &&
                       handles[j][i].getWidth() == c.width && (int) handles[j][i].getInliers().size() == c.n_inliers;
    }
  }
  std::printf("POINTS %d %d %d %d\n", same_list ? 1 : 0, same_sizes ? 1 : 0, same_handles ? 1 : 0, same_plane ? 1 : 0);

  // a fitted call while a chain is pending returns empty lists and leaves that chain collectable (no fitted plane then); 65
  // lists: none
  PointCloud::Ptr cloud2(new PointCloud(*cloud)), cloud3(new PointCloud(*cloud));
  if (!loc.localizeHandlesBegin(cloud2, (int) size_left, std::vector<int>(), argv[3], 2, 0.005))
    return 4;
  const std::vector<std::vector<Handle> > refused = loc.localizeHandlesClusteredFit(cloud3, (int) size_left, argv[3], 2, 0.005);
  bool found_pending = true;
  loc.fittedPlane(&found_pending);
  size_t refused_handles = 0;
  for (size_t j = 0; j < refused.size(); j++)
    refused_handles += refused[j].size();
  std::vector<GraspHypothesis> kept_p;
  loc.localizeHandlesEnd(&kept_p);
  loc.setClusterParams(cp.min_height, cp.max_height, cp.tolerance, cp.min_voxels, 65);
  PointCloud::Ptr cloud4(new PointCloud(*cloud));
  const size_t too_many = loc.localizeHandlesClusteredFit(cloud4, (int) size_left, argv[3], 2, 0.005).size();
  std::printf("PENDING %zu %zu %zu %zu %zu %d\n", refused.size(), refused_handles, kept_p.size(), too_many, loc.getClusterSizes().size(),
    found_pending ? 1 : 0);
  return 0;
}
