// plane_adapter_test.cpp -- Localization::localizeHands(left.pcd, right.pcd, calculates_antipodal, uses_clustering = true),
// the call src/nodes/train.cpp:115 makes: preprocessing, table-plane removal, search over the remaining points.
//   plane_adapter_test <left.pcd> <right.pcd> <xmin xmax ymin ymax zmin zmax> <cam0 xyz> <cam1 xyz> <num_samples> <seed>
// prints the plane result, the searched cloud, the samples drawn over it and the hands.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "agile_grasp_amd/localization.h"

using namespace agile_grasp_amd;

int main(int argc, char** argv)
{
  if (argc != 17)
  {
    std::printf("usage: %s <left.pcd> <right.pcd> <workspace x6> <cam0 x3> <cam1 x3> <num_samples> <seed>\n", argv[0]);
    return 2;
  }
  VectorXd ws(6);
  for (int i = 0; i < 6; i++)
    ws((std::size_t) i) = std::atof(argv[3 + i]);
  Matrix4d tl, tr;
  for (int r = 0; r < 3; r++)
  {
    tl(r, 3) = std::atof(argv[9 + r]);
    tr(r, 3) = std::atof(argv[12 + r]);
  }
  Localization loc(1, false, 0);
  loc.setCameraTransforms(tl, tr);
  loc.setWorkspace(ws);
  loc.setNumSamples(std::atoi(argv[15]));
  loc.setDeterministicNormalEstimation(true);
  loc.getHandSearch().setSampleSeed((std::uint64_t) std::atoll(argv[16]));
  std::vector<GraspHypothesis> hands = loc.localizeHands(argv[1], argv[2], true, true);
  const PointCloud::Ptr& cloud = loc.getSearchedCloud();
  const VectorXi& cam = loc.getSearchedCamSource();
  std::printf("CLOUD %zu\n", cloud ? cloud->size() : (size_t) 0);
  for (size_t i = 0; cloud && i < cloud->size(); i++)
    std::printf("P %.9g %.9g %.9g %d\n", cloud->points[i].x, cloud->points[i].y, cloud->points[i].z, (int) cam((std::size_t) i));
  const std::vector<std::int32_t>& idx = loc.getHandSearch().getLastSampleIndices();
  for (size_t i = 0; i < idx.size(); i++)
    std::printf("S %d\n", (int) idx[i]);
  std::printf("RESULT %zu\n", hands.size());
  for (size_t i = 0; i < hands.size(); i++)
    std::printf("H %.17g %.17g %.17g %.17g %d %d\n", hands[i].getGraspSurface()(0), hands[i].getGraspSurface()(1),
      hands[i].getGraspSurface()(2), hands[i].getGraspWidth(), hands[i].getCamSource(), hands[i].isFullAntipodal() ? 1 : 0);
  return 0;
}
