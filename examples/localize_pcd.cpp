// localize_pcd.cpp -- what src/nodes/find_grasps.cpp + grasp_localizer.cpp do per cloud, without ROS: read one or two
// PCD files, localise hands, keep the ones the SVM calls antipodal, search handles, print the Grasp message fields.
//
//   g++ -std=c++11 -O2 -Iinclude examples/localize_pcd.cpp -o localize_pcd -Lagile_grasp_amd/lib -lagile_grasp_hip
//       -Wl,-rpath,$PWD/agile_grasp_amd/lib -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib
//   ./localize_pcd [--filters-boundaries] [--voxel-filter R,K] [--approach dx,dy,dz,cos] [--aperture lo,hi]
//                  [--clearance near,far,half_w,half_h[,max_points]] [--rank w_support,w_margin[,max_handles]]
//                  [--table a,b,c,d [--cluster-tolerance t]] <svm file> <left.pcd> [right.pcd] [num_samples] [min_inliers]
//
// Parameters are the node's defaults (find_grasps.cpp:10-21): finger width 0.01, outer diameter 0.09, hand depth 0.06,
// hand height 0.02, init bite 0.01, 2000 samples, workspace [0.65 0.9 -0.1 0.1 -0.2 1.0], min_inliers 3, camera poses
// of find_grasps.cpp:35-45.  --filters-boundaries builds the Localization as the nodes do (grasp_localizer.cpp:21,
// nodes/test.cpp:72): hands within 2 cm of a face of the workspace are dropped before the classifier.
// --table a,b,c,d names the support plane ((a, b, c) a unit vector pointing from the table towards the objects): the objects are
// the connected components of the points above it (Localization::localizeHandlesClustered), num_samples samples are drawn on
// EACH of them and the handles are printed per object; --cluster-tolerance t (metres, default 0.01) is the distance up to which
// two voxels belong to one object.
// --voxel-filter R,K prunes, on the device, the voxels with fewer than K occupied voxels of their own camera within R voxels
// (Localization::setVoxelFilter): stray returns in free space, which would veto placements beside them.
// --approach dx,dy,dz,cos keeps the hands whose approach vector (hand -> object) has a dot product of at least cos with the unit
// vector (dx, dy, dz) -- 0,0,-1,0.7 is a top-down cell -- and --aperture lo,hi those whose grasp width lies in [lo, hi] metres,
// the gripper's stroke (Localization::setHandFilter): the others are dropped on the device, ahead of the classifier.  (The filter's
// third criterion, fingers in observed space, needs depth images, which a PCD file does not hold.)
// --clearance near,far,half_w,half_h[,max_points] drops the hands whose approach corridor -- the box from near to far metres behind
// the palm, +- half_w along the closing direction, +- half_h along the hand's axis -- holds more than max_points (default 0) points
// of the cloud: 0,0.12,0.05,0.04 is a gripper body of 10 x 8 cm over 12 cm (Localization::setHandClearance).
// --rank w_support,w_margin[,max_handles] returns the handles best first: scored on the device by their number of hands (up to
// ten) and the classifier's mean margin under the two weights, at most max_handles of them (default 0: all), the score printed
// beside each (Localization::setHandleRanking).  The ranking is a stage of the one-call chain, so with --rank and no --table the
// cloud goes through localizeHandles, samples drawn on the device, where it otherwise takes the node's three calls.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "agile_grasp_amd/localization.h"

using namespace agile_grasp_amd;

int main(int argc, char** argv)
{
  const bool filters_boundaries = argc > 1 && std::strcmp(argv[1], "--filters-boundaries") == 0;
  if (filters_boundaries)
  {
    argv[1] = argv[0];
    argv++;
    argc--;
  }
  bool table = false, voxel_filter = false, approach = false, aperture = false;
  int vf_radius = 0, vf_neighbors = 0;
  agh_hand_filter_params hand_filter;
  agh_default_hand_filter_params(&hand_filter);
  bool clearance = false;
  agh_hand_clearance_params hand_clearance;
  agh_default_hand_clearance_params(&hand_clearance);
  bool rank = false;
  agh_handle_ranking_params ranking;
  agh_default_handle_ranking_params(&ranking);
  double plane[4] = { 0.0, 0.0, 1.0, 0.0 }, cluster_tolerance = 0.01;
  while (argc > 2 && (std::strcmp(argv[1], "--table") == 0 || std::strcmp(argv[1], "--cluster-tolerance") == 0 ||
                      std::strcmp(argv[1], "--voxel-filter") == 0 || std::strcmp(argv[1], "--approach") == 0 ||
                      std::strcmp(argv[1], "--aperture") == 0 || std::strcmp(argv[1], "--clearance") == 0 ||
                      std::strcmp(argv[1], "--rank") == 0))
  {
    if (std::strcmp(argv[1], "--table") == 0)
      table = std::sscanf(argv[2], "%lf,%lf,%lf,%lf", &plane[0], &plane[1], &plane[2], &plane[3]) == 4;
    else if (std::strcmp(argv[1], "--voxel-filter") == 0)
      voxel_filter = std::sscanf(argv[2], "%d,%d", &vf_radius, &vf_neighbors) == 2;
    else if (std::strcmp(argv[1], "--approach") == 0)
      approach = std::sscanf(argv[2], "%lf,%lf,%lf,%lf", &hand_filter.approach_dir[0], &hand_filter.approach_dir[1],
                   &hand_filter.approach_dir[2], &hand_filter.min_approach_cos) == 4;
    else if (std::strcmp(argv[1], "--aperture") == 0)
      aperture = std::sscanf(argv[2], "%lf,%lf", &hand_filter.min_width, &hand_filter.max_width) == 2;
    else if (std::strcmp(argv[1], "--clearance") == 0)
      clearance = std::sscanf(argv[2], "%lf,%lf,%lf,%lf,%d", &hand_clearance.near_offset, &hand_clearance.far_offset,
                    &hand_clearance.half_width, &hand_clearance.half_height, &hand_clearance.max_points) >= 4;
    else if (std::strcmp(argv[1], "--rank") == 0)
      rank = std::sscanf(argv[2], "%lf,%lf,%d", &ranking.w_support, &ranking.w_margin, &ranking.max_handles) >= 2;
    else
      cluster_tolerance = std::atof(argv[2]);
    argv[2] = argv[0];
    argv += 2;
    argc -= 2;
  }
  if (argc < 3)
  {
    std::printf("usage: %s [--filters-boundaries] [--voxel-filter R,K] [--approach dx,dy,dz,cos] [--aperture lo,hi] "
                "[--clearance near,far,half_w,half_h[,max_points]] [--rank w_support,w_margin[,max_handles]] "
                "[--table a,b,c,d [--cluster-tolerance t]] "
                "<svm file> <left.pcd> [right.pcd] [num_samples] [min_inliers]\n", argv[0]);
    return 2;
  }
  const std::string svm = argv[1], left = argv[2], right = argc > 3 ? argv[3] : "";
  const int num_samples = argc > 4 ? std::atoi(argv[4]) : 2000;
  const int min_inliers = argc > 5 ? std::atoi(argv[5]) : 3;
  // camera poses: base_tf * sqrt_tf^-1 and base_tf * sqrt_tf; only the translations enter the search
  Matrix4d cam_left, cam_right;
  const double tl[3] = { 0.2535951756826822, 0.2724534249381174, 0.19915903314998992 };
  const double tr[3] = { 0.2671843128, -0.3013, 0.2105167716 };
  for (int r = 0; r < 3; r++)
  {
    cam_left(r, 3) = tl[r];
    cam_right(r, 3) = tr[r];
  }
  Localization loc(4, filters_boundaries, 0);  // num_threads (unused on the GPU), filters_boundaries, plotting mode
  loc.setCameraTransforms(cam_left, cam_right);
  VectorXd ws(6);
  const double w[6] = { 0.65, 0.9, -0.1, 0.1, -0.2, 1.0 };
  for (int i = 0; i < 6; i++)
    ws(i) = w[i];
  loc.setWorkspace(ws);
  loc.setNumSamples(num_samples);
  loc.setFingerWidth(0.01);
  loc.setHandOuterDiameter(0.09);
  loc.setHandDepth(0.06);
  loc.setInitBite(0.01);
  loc.setHandHeight(0.02);
  if (voxel_filter)
  {
    agh_voxel_filter_params fp;
    fp.radius = vf_radius;
    fp.min_neighbors = vf_neighbors;
    if (!loc.setVoxelFilter(fp))  // (the library's message says which field it refused)
      return 1;
  }
  if (approach || aperture)
  {
    hand_filter.approach_on = approach ? 1 : 0;
    hand_filter.width_on = aperture ? 1 : 0;
    if (!loc.setHandFilter(hand_filter))  // (likewise)
      return 1;
  }
  if (clearance && !loc.setHandClearance(hand_clearance))  // (likewise)
    return 1;
  if (rank && !loc.setHandleRanking(ranking))  // (likewise)
    return 1;

  if (table)
  {
    // handles per object on the table: the clouds are read as localizeHands(left, right) reads them
    PointCloud::Ptr cloud(new PointCloud), cloud_right(new PointCloud);
    if (loadPCDFile(left, *cloud) == -1 || (right.length() > 0 && loadPCDFile(right, *cloud_right) == -1))
    {
      std::printf("could not read the PCD files\n");
      return 1;
    }
    const int size_left = (int) cloud->size();
    cloud->points.insert(cloud->points.end(), cloud_right->points.begin(), cloud_right->points.end());
    cloud->is_dense = cloud->is_dense && cloud_right->is_dense;
    VectorXd pl(4);
    for (int i = 0; i < 4; i++)
      pl(i) = plane[i];
    loc.setClusterParams(0.01, 0.5, cluster_tolerance, 50, 16);
    const std::vector<std::vector<Handle> > per_object = loc.localizeHandlesClustered(cloud, size_left, pl, svm, min_inliers, 0.005);
    const std::vector<std::int64_t> sizes = loc.getClusterSizes();
    const std::vector<agh_handle_score> scores = loc.handleScores();  // (all objects' handles, object after object; empty unranked)
    std::size_t first = 0;
    for (std::size_t j = 0; j < per_object.size(); first += per_object[j].size(), j++)
    {
      if (j >= sizes.size() || sizes[j] <= 0)
        continue;
      const Grasps msg = createGraspsMsg(per_object[j]);
      std::printf("object %zu: %lld voxels, %zu handles\n", j, (long long) sizes[j], per_object[j].size());
      for (std::size_t i = 0; i < msg.grasps.size(); i++)
      {
        std::printf("  grasp %zu: center %.4f %.4f %.4f  axis %.4f %.4f %.4f  width %.4f", i, msg.grasps[i].center(0),
          msg.grasps[i].center(1), msg.grasps[i].center(2), msg.grasps[i].axis(0), msg.grasps[i].axis(1), msg.grasps[i].axis(2),
          (double) msg.grasps[i].width);
        if (first + i < scores.size())
          std::printf("  score %.6f (found as handle %d)", scores[first + i].score, (int) scores[first + i].index);
        std::printf("\n");
      }
    }
    return 0;
  }
  if (rank)
  {
    // the one-call chain, which ranks: the clouds read as localizeHands(left, right) reads them, the samples drawn on the device
    PointCloud::Ptr cloud(new PointCloud), cloud_right(new PointCloud);
    if (loadPCDFile(left, *cloud) == -1 || (right.length() > 0 && loadPCDFile(right, *cloud_right) == -1))
    {
      std::printf("could not read the PCD files\n");
      return 1;
    }
    const int size_left = (int) cloud->size();
    cloud->points.insert(cloud->points.end(), cloud_right->points.begin(), cloud_right->points.end());
    cloud->is_dense = cloud->is_dense && cloud_right->is_dense;
    std::vector<GraspHypothesis> antipodal;
    const std::vector<Handle> handles = loc.localizeHandles(cloud, size_left, std::vector<int>(), svm, min_inliers, 0.005, &antipodal);
    const std::vector<agh_handle_score> scores = loc.handleScores();
    const Grasps msg = createGraspsMsg(handles);
    std::printf("%zu antipodal, %zu handles\n", antipodal.size(), handles.size());
    for (std::size_t i = 0; i < msg.grasps.size(); i++)
    {
      const Grasp& g = msg.grasps[i];
      std::printf("grasp %zu: center %.4f %.4f %.4f  axis %.4f %.4f %.4f  approach %.4f %.4f %.4f  width %.4f", i,
        g.center(0), g.center(1), g.center(2), g.axis(0), g.axis(1), g.axis(2), g.approach(0), g.approach(1), g.approach(2),
        (double) g.width);
      if (i < scores.size())
        std::printf("  score %.6f (found as handle %d)", scores[i].score, (int) scores[i].index);
      std::printf("\n");
    }
    return 0;
  }
  std::vector<GraspHypothesis> hands = loc.localizeHands(left, right, false, false);      // grasp_localizer.cpp:95
  std::vector<GraspHypothesis> antipodal = loc.predictAntipodalHands(hands, svm);          // :102
  std::vector<Handle> handles = loc.findHandles(antipodal, min_inliers, 0.005);            // :103
  const Grasps msg = createGraspsMsg(handles);                                             // :106
  std::printf("%zu hands, %zu antipodal, %zu handles\n", hands.size(), antipodal.size(), handles.size());
  for (std::size_t i = 0; i < msg.grasps.size(); i++)
  {
    const Grasp& g = msg.grasps[i];
    std::printf("grasp %zu: center %.4f %.4f %.4f  axis %.4f %.4f %.4f  approach %.4f %.4f %.4f  width %.4f\n", i,
      g.center(0), g.center(1), g.center(2), g.axis(0), g.axis(1), g.axis(2), g.approach(0), g.approach(1), g.approach(2),
      (double) g.width);
  }
  return 0;
}
