// batch_cluster_fit_adapter_test.cpp -- runs the adapter's fitted clustered batch calls (include/agile_grasp_amd/localization.h):
//   batch_cluster_fit_adapter_test gpu <capture.bin> <svm>   localizeHandlesBatchClusteredFit over the capture twice (capture k
//                                                            seeded with the sample seed + k) against the C call
//                                                            (agh_localize_batch_clustered_fit: the same planes, per capture
//                                                            and object the same counts and handle records, the same object
//                                                            sizes), its Begin / End halves, and a fitted batch while a
//                                                            chain is pending
// capture.bin: as tests/cpp/cluster_fit_adapter_test.cpp reads it.
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
  const size_t C = 2;
  agh_cluster_params cp1;
  agh_default_cluster_params(&cp1);
  for (int k = 0; k < 4; k++)
    cp1.plane[k] = pl[k];
  cp1.min_height = pl[4];
  cp1.max_height = pl[5];
  cp1.tolerance = pl[6];
  cp1.min_voxels = (std::int32_t) iv[0];
  cp1.max_objects = (std::int32_t) iv[1];
  const long long n_samples = iv[2], seed = iv[3];
  const size_t K = (size_t) cp1.max_objects, L = C * K;
  agh_plane_fit_params fp1;
  agh_default_plane_fit_params(&fp1);
  fp1.n_candidates = (std::int32_t) fv[0];
  fp1.seed = (std::uint64_t) fv[1];
  fp1.distance_threshold = threshold;
  const std::vector<agh_cluster_params> cp(C, cp1);
  const std::vector<agh_plane_fit_params> fp(C, fp1);

  // the C call
  agh_params p;
  agh_default_params(&p);
  for (int k = 0; k < 2; k++)
    for (int r = 0; r < 3; r++)
      p.cam_origin[k][r] = org[3 * k + r];
  agh_ctx* ctx = nullptr;
  if (agh_create(&p, &ctx) != AGH_OK || agh_load_svm_file(ctx, argv[3]) != AGH_OK)
    return 3;
  std::vector<agh_localize_params> lp(C);
  for (size_t k = 0; k < C; k++)
  {
    std::memset(&lp[k], 0, sizeof(lp[k]));
    lp[k].size_left = size_left;
    lp[k].dense = 1;
    lp[k].classify = 1;
    for (int i = 0; i < 6; i++)
      lp[k].workspace[i] = ws[i];
    lp[k].cell_size = 0.003;
    lp[k].n_samples = n_samples;
    lp[k].sample_seed = (std::uint64_t) seed + k;
    lp[k].min_inliers = 2;
    lp[k].min_length = 0.005;
  }
  const float* ptrs[C] = { xyz.data(), xyz.data() };
  const std::int64_t strides[C] = { 12, 12 }, ns[C] = { n, n };
  const std::int64_t cap = 8 * n_samples * (std::int64_t) L;
  std::vector<agh_handle> c_handles((size_t) cap);
  std::vector<std::int32_t> c_idx((size_t) cap);
  std::vector<agh_hypothesis> c_hands((size_t) cap);
  std::vector<agh_localize_batch_result> res(L);
  if (agh_localize_batch_clustered_fit(ctx, ptrs, strides, ns, fp.data(), cp.data(), lp.data(), (std::int32_t) C, c_handles.data(), cap,
        c_idx.data(), cap, c_hands.data(), cap, nullptr, res.data()) != AGH_OK)
  {
    std::printf("agh_localize_batch_clustered_fit: %s\n", agh_last_error(ctx));
    return 3;
  }
  agh_plane_fit_result fit[C];
  if (agh_get_batch_plane_fit(ctx, fit, (std::int32_t) C) != (int) C)
    return 3;
  std::vector<agh_cluster_info> info(C);
  std::vector<std::int64_t> m_c(L, -1);
  if (agh_get_batch_cluster_info(ctx, info.data(), m_c.data(), nullptr, (std::int32_t) C, (std::int32_t) L) != AGH_OK)
    return 3;
  agh_destroy(ctx);
  long long c_kept = 0, c_n_handles = 0;
  for (size_t l = 0; l < L; l++)
  {
    c_kept += res[l].r.n_hands;
    c_n_handles += res[l].r.n_handles;
  }
  std::printf("C %lld %lld %lld %lld %d %d\n", c_kept, c_n_handles, (long long) (info[0].n_objects + info[1].n_objects),
    (long long) (info[0].n_foreground + info[1].n_foreground), fit[0].found + fit[1].found, fit[0].refined + fit[1].refined);

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
  loc.setClusterParams(cp1.min_height, cp1.max_height, cp1.tolerance, cp1.min_voxels, cp1.max_objects);
  loc.setPlaneFitParams(fp1.n_candidates, fp1.distance_threshold, fp1.min_inliers, fp1.refine != 0, fp1.seed);
  std::vector<bool> found_before(1, true);
  const size_t planes_before = loc.fittedPlanes(&found_before).size();  // (no chain yet: none)
  std::vector<PointCloud::Ptr> clouds;
  for (size_t k = 0; k < C; k++)
    clouds.push_back(PointCloud::Ptr(new PointCloud(*cloud)));
  const std::vector<int> sizes_left(C, (int) size_left);
  std::vector<std::vector<std::vector<GraspHypothesis> > > kept;
  const std::vector<std::vector<std::vector<Handle> > > handles =
    loc.localizeHandlesBatchClusteredFit(clouds, sizes_left, argv[3], 2, 0.005, &kept);
  std::vector<bool> found;
  const std::vector<VectorXd> planes = loc.fittedPlanes(&found);
  bool same_planes = planes.size() == C && found.size() == C && planes_before == 0 && found_before.empty();
  for (size_t k = 0; same_planes && k < C; k++)
    for (int q = 0; q < 4; q++)
    {
      const double got = planes[k](q);
      same_planes = same_planes && found[k] == (fit[k].found != 0) && std::memcmp(&fit[k].plane[q], &got, 8) == 0;
    }
  const std::vector<std::int64_t> m_a = loc.getBatchClusterSizes();
  bool same_sizes = m_a.size() == L;
  for (size_t l = 0; same_sizes && l < L; l++)
    same_sizes = m_a[l] == m_c[l];
  bool same_handles = handles.size() == C && kept.size() == C;
  for (size_t k = 0; same_handles && k < C; k++)
  {
    same_handles = handles[k].size() == K && kept[k].size() == K;
    for (size_t j = 0; same_handles && j < K; j++)
    {
      const agh_localize_batch_result& r = res[k * K + j];
      same_handles = handles[k][j].size() == (size_t) r.r.n_handles && kept[k][j].size() == (size_t) r.r.n_hands;
      for (size_t i = 0; same_handles && i < handles[k][j].size(); i++)
      {
        const agh_handle& c = c_handles[(size_t) r.first_handle + i];
        for (int q = 0; same_handles && q < 3; q++)
          same_handles = handles[k][j][i].getAxis()(q) == c.axis[q] && handles[k][j][i].getCenter()(q) == c.center[q] &&
                         handles[k][j][i].getWidth() == c.width && (int) handles[k][j][i].getInliers().size() == c.n_inliers;
      }
    }
  }
  // the two halves give the blocking call's handles
  for (size_t k = 0; k < C; k++)
    clouds[k] = PointCloud::Ptr(new PointCloud(*cloud));
  bool same_halves = loc.localizeHandlesBatchClusteredFitBegin(clouds, sizes_left, argv[3], 2, 0.005);
  const std::vector<std::vector<std::vector<Handle> > > halves = loc.localizeHandlesBatchLabeledEnd();
  same_halves = same_halves && halves.size() == C;
  for (size_t k = 0; same_halves && k < C; k++)
  {
    same_halves = halves[k].size() == K;
    for (size_t j = 0; same_halves && j < K; j++)
      same_halves = halves[k][j].size() == handles[k][j].size();
  }
  std::printf("POINTS %d %d %d %d\n", same_planes ? 1 : 0, same_sizes ? 1 : 0, same_handles ? 1 : 0, same_halves ? 1 : 0);

  // a fitted batch while a chain is pending returns empty lists per capture and object and leaves that chain collectable (no
  // fitted planes then); cluster records for another number of captures: refused, no list
  PointCloud::Ptr cloud2(new PointCloud(*cloud));
  if (!loc.localizeHandlesBegin(cloud2, (int) size_left, std::vector<int>(), argv[3], 2, 0.005))
    return 4;
  for (size_t k = 0; k < C; k++)
    clouds[k] = PointCloud::Ptr(new PointCloud(*cloud));
  const std::vector<std::vector<std::vector<Handle> > > refused = loc.localizeHandlesBatchClusteredFit(clouds, sizes_left, argv[3], 2, 0.005);
  const size_t planes_pending = loc.fittedPlanes().size();
  size_t refused_lists = 0, refused_handles = 0;
  for (size_t k = 0; k < refused.size(); k++)
    for (size_t j = 0; j < refused[k].size(); j++)
    {
      refused_lists++;
      refused_handles += refused[k][j].size();
    }
  std::vector<GraspHypothesis> kept_p;
  loc.localizeHandlesEnd(&kept_p);
  const std::vector<agh_cluster_params> three(3, cp1);
  for (size_t k = 0; k < C; k++)
    clouds[k] = PointCloud::Ptr(new PointCloud(*cloud));
  const size_t mismatch = loc.localizeHandlesBatchClusteredFit(clouds, sizes_left, argv[3], 2, 0.005, nullptr, nullptr, &three).size();
  std::printf("PENDING %zu %zu %zu %zu %zu %zu\n", refused.size(), refused_lists, refused_handles, kept_p.size(), planes_pending, mismatch);
  return 0;
}
