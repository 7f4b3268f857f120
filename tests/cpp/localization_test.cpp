// localization_test.cpp -- drives the Localization facade (include/agile_grasp_amd/localization.h) on a RAW cloud
// (NaNs, points outside the workspace, no voxelisation), like src/tests/test_local_axes.cpp drives the reference's.
//   localization_test <raw.bin> <svm file> <mode: voxels|hands|antipodal|chain|stream|rebegin>
//   (antipodal: src/tests/antipodal_test.cpp)
// raw.bin as chain_common.h reads it.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_common.h"

int main(int argc, char** argv)
{
  if (argc < 4)
    return 2;
  Capture c;
  if (!read_capture(argv[1], c))
    return 2;
  const PointCloud::Ptr cloud = c.cloud;
  const int size_left = c.size_left;
  const std::vector<int>& idx = c.idx;
  Localization loc(1, false, 0);
  setup(loc, c);
  if (std::strcmp(argv[3], "voxels") == 0)
  {
    // preprocessing as localizeHands runs it (on the GPU): print the cloud the search worked on
    std::vector<GraspHypothesis> hands = loc.localizeHands(cloud, size_left, idx, false, false);
    const PointCloud::Ptr& vox = loc.getSearchedCloud();
    if (!vox)
    {
      std::printf("NO_CLOUD\n");
      return 0;
    }
    std::printf("VOXELS %zu\n", vox->points.size());
    for (size_t i = 0; i < vox->points.size(); i++)
      std::printf("V %.9g %.9g %.9g %d\n", vox->points[i].x, vox->points[i].y, vox->points[i].z,
        (int) loc.getSearchedCamSource()((int) i));
    return 0;
  }
  if (std::strcmp(argv[3], "chain") == 0)
  {
    // grasp_localizer.cpp:95-103 twice: the three calls of the reference's caller, then the one-call form; the two must print
    // the same kept hands and the same handles
    std::vector<GraspHypothesis> hands3 = loc.localizeHands(cloud, size_left, idx, false, false);
    std::vector<GraspHypothesis> kept3 = loc.predictAntipodalHands(hands3, argv[2]);
    std::vector<Handle> handles3 = loc.findHandles(kept3, 2, 0.005);
    std::vector<GraspHypothesis> kept1;
    std::vector<Handle> handles1 = loc.localizeHandles(cloud, size_left, idx, argv[2], 2, 0.005, &kept1);
    for (int pass = 0; pass < 2; pass++)
    {
      const std::vector<GraspHypothesis>& kept = pass == 0 ? kept3 : kept1;
      const std::vector<Handle>& handles = pass == 0 ? handles3 : handles1;
      std::printf("CHAIN%d %zu %zu\n", pass == 0 ? 3 : 1, kept.size(), handles.size());
      for (size_t i = 0; i < kept.size(); i++)
        std::printf("K%d %.17g %.17g %.17g %.17g %d\n", pass == 0 ? 3 : 1, kept[i].getGraspSurface()(0), kept[i].getGraspBottom()(1),
          kept[i].getApproach()(2), kept[i].getGraspWidth(), kept[i].isFullAntipodal() ? 1 : 0);
      for (size_t i = 0; i < handles.size(); i++)
      {
        std::printf("G%d %zu %.17g %.17g %.17g %.17g %zu", pass == 0 ? 3 : 1, handles[i].getInliers().size(), handles[i].getAxis()(0),
          handles[i].getCenter()(1), handles[i].getBinormal()(2), handles[i].getWidth(), handles[i].getHandList().size());
        for (size_t k = 0; k < handles[i].getInliers().size(); k++)
          std::printf(" %d", handles[i].getInliers()[k]);
        std::printf("\n");
      }
    }
    return 0;
  }
  if (std::strcmp(argv[3], "stream") == 0)
  {
    // a node that holds the next capture while this one is searched: localizeHandlesBegin / stageNextCloud / localizeHandlesEnd
    // over three captures (copies of the cloud: distinct objects) against localizeHandles on the first
    PointCloud::Ptr clouds[3];
    for (int k = 0; k < 3; k++)
      clouds[k] = PointCloud::Ptr(new PointCloud(*cloud));
    std::vector<GraspHypothesis> kept1;
    PointCloud::Ptr ref_cloud(new PointCloud(*cloud));
    std::vector<Handle> handles1 = loc.localizeHandles(ref_cloud, size_left, idx, argv[2], 2, 0.005, &kept1);
    std::printf("CHAIN1 %zu %zu\n", kept1.size(), handles1.size());
    if (!loc.localizeHandlesBegin(clouds[0], size_left, idx, argv[2], 2, 0.005))
      return 3;
    for (int k = 0; k < 3; k++)
    {
      if (k + 1 < 3 && !loc.stageNextCloud(clouds[k + 1]))
        return 4;
      std::vector<GraspHypothesis> kept;
      std::vector<Handle> handles = loc.localizeHandlesEnd(&kept);
      if (k + 1 < 3 && !loc.localizeHandlesBegin(clouds[k + 1], size_left, idx, argv[2], 2, 0.005))
        return 5;
      std::printf("STREAM %d %zu %zu %d\n", k, kept.size(), handles.size(), same_chain(kept, handles, kept1, handles1) ? 1 : 0);
    }
    return 0;
  }
  if (std::strcmp(argv[3], "rebegin") == 0)
  {
    // localizeHandlesBegin while a chain is pending: refused, and the chain in flight stays pending.  Capture A is the cloud,
    // capture B the same points in reverse order (another cloud with as many voxels, so the indices stay valid).
    PointCloud::Ptr a(new PointCloud(*cloud)), a_again(new PointCloud(*cloud)), a_ref(new PointCloud(*cloud));
    PointCloud::Ptr b(new PointCloud(*cloud));
    std::reverse(b->points.begin(), b->points.end());
    std::vector<GraspHypothesis> kept_a, kept_b_ref;
    std::vector<Handle> handles_a = loc.localizeHandles(a_ref, size_left, idx, argv[2], 2, 0.005, &kept_a);
    Localization loc_b(1, false, 0);  // (B's results on an object of its own)
    setup(loc_b, c);
    PointCloud::Ptr b_ref(new PointCloud(*b));
    std::vector<Handle> handles_b_ref = loc_b.localizeHandles(b_ref, size_left, idx, argv[2], 2, 0.005, &kept_b_ref);
    std::printf("CHAIN1 %zu %zu\n", kept_a.size(), handles_a.size());
    if (!loc.localizeHandlesBegin(a, size_left, idx, argv[2], 2, 0.005))
      return 3;
    const bool b_refused = !loc.localizeHandlesBegin(b, size_left, idx, argv[2], 2, 0.005);
    const bool no_svm_refused = !loc.localizeHandlesBegin(a_again, size_left, idx, "no_such_svm_file", 2, 0.005);
    std::vector<GraspHypothesis> kept;
    std::vector<Handle> handles = loc.localizeHandlesEnd(&kept);
    std::printf("REBEGIN %d %d %zu %zu %d\n", b_refused ? 1 : 0, no_svm_refused ? 1 : 0, kept.size(), handles.size(),
      same_chain(kept, handles, kept_a, handles_a) ? 1 : 0);
    // the object is usable afterwards: B in one call, then a fresh Begin / End of A
    std::vector<GraspHypothesis> kept_b;
    std::vector<Handle> handles_b = loc.localizeHandles(b, size_left, idx, argv[2], 2, 0.005, &kept_b);
    PointCloud::Ptr a_fresh(new PointCloud(*cloud));
    const bool begun = loc.localizeHandlesBegin(a_fresh, size_left, idx, argv[2], 2, 0.005);
    std::vector<GraspHypothesis> kept2;
    std::vector<Handle> handles2 = loc.localizeHandlesEnd(&kept2);
    std::printf("AFTER %zu %zu %d %d %d\n", kept_b.size(), handles_b.size(), same_chain(kept_b, handles_b, kept_b_ref, handles_b_ref) ? 1 : 0,
      begun ? 1 : 0, same_chain(kept2, handles2, kept_a, handles_a) ? 1 : 0);
    return 0;
  }
  const bool antipodal = std::strcmp(argv[3], "antipodal") == 0;  // calculates_antipodal (antipodal_test.cpp:61)
  std::vector<GraspHypothesis> hands = loc.localizeHands(cloud, size_left, idx, antipodal, false);
  if (antipodal)
  {
    for (size_t i = 0; i < hands.size(); i++)
      std::printf("A %d %d\n", hands[i].isHalfAntipodal() ? 1 : 0, hands[i].isFullAntipodal() ? 1 : 0);
    return 0;
  }
  std::vector<GraspHypothesis> kept = loc.predictAntipodalHands(hands, argv[2]);
  std::printf("RESULT %zu %zu %zu\n", loc.getSearchedCloud() ? loc.getSearchedCloud()->size() : (size_t) 0, hands.size(),
    kept.size());
  for (size_t i = 0; i < hands.size(); i++)
    std::printf("H %.17g %.17g %.17g %.17g\n", hands[i].getGraspSurface()(0), hands[i].getGraspBottom()(1),
      hands[i].getApproach()(2), hands[i].getGraspWidth());
  // grasp_localizer.cpp:103 runs the handle search on the SVM-positive hands; all hands give the test more material
  std::vector<Handle> handles = loc.findHandles(hands, 3, 0.005);
  for (size_t i = 0; i < handles.size(); i++)
    std::printf("HANDLE %zu %d %.17g %.17g %.17g %.17g\n", handles[i].getInliers().size(), handles[i].getInliers()[0],
      handles[i].getAxis()(0), handles[i].getCenter()(1), handles[i].getBinormal()(2), handles[i].getWidth());
  return 0;
}
