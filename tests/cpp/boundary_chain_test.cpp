// boundary_chain_test.cpp -- Localization(4, true, 0), the nodes' configuration (grasp_localizer.cpp:21, nodes/test.cpp:72),
// through the fused chain: localizeHandles / localizeHandlesBegin / stageNextCloud / localizeHandlesEnd run filterHands on
// the device, between the search and the classifier.
//   boundary_chain_test chain <svm file> <raw.bin>
//       the three calls (localizeHands filters on the host) against localizeHandles on the same object
//   boundary_chain_test stream <svm file> <raw.bin> <raw.bin> <raw.bin>
//       three captures through Begin / stageNextCloud / End on a fresh object against localizeHandles per capture
// raw.bin as chain_common.h reads it (the workspace and camera origins of the first file hold for all).
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_common.h"

static void print_chain(const char* tag, const std::vector<GraspHypothesis>& kept, const std::vector<Handle>& handles)
{
  std::printf("CHAIN%s %zu %zu\n", tag, kept.size(), handles.size());
  for (size_t i = 0; i < kept.size(); i++)
    std::printf("K%s %.17g %.17g %.17g %.17g %d\n", tag, kept[i].getGraspSurface()(0), kept[i].getGraspSurface()(1),
      kept[i].getGraspSurface()(2), kept[i].getGraspWidth(), kept[i].isFullAntipodal() ? 1 : 0);
  for (size_t i = 0; i < handles.size(); i++)
  {
    std::printf("G%s %zu %.17g %.17g %.17g %.17g", tag, handles[i].getInliers().size(), handles[i].getAxis()(0),
      handles[i].getCenter()(1), handles[i].getBinormal()(2), handles[i].getWidth());
    for (size_t k = 0; k < handles[i].getInliers().size(); k++)
      std::printf(" %d", handles[i].getInliers()[k]);
    std::printf("\n");
  }
}

int main(int argc, char** argv)
{
  if (argc < 4)
    return 2;
  const char* svm = argv[2];
  if (std::strcmp(argv[1], "chain") == 0)
  {
    Capture c;
    if (!read_capture(argv[3], c))
      return 2;
    Localization loc(4, true, 0);
    setup(loc, c);
    // grasp_localizer.cpp:95-103 as the node runs it: localizeHands filters, then the classifier and the handle search
    PointCloud::Ptr c3(new PointCloud(*c.cloud)), c1(new PointCloud(*c.cloud));
    std::vector<GraspHypothesis> hands3 = loc.localizeHands(c3, c.size_left, c.idx, false, false);
    std::vector<GraspHypothesis> kept3 = loc.predictAntipodalHands(hands3, svm);
    std::vector<Handle> handles3 = loc.findHandles(kept3, 2, 0.005);
    std::printf("HANDS %zu\n", hands3.size());
    std::vector<GraspHypothesis> kept1;
    std::vector<Handle> handles1 = loc.localizeHandles(c1, c.size_left, c.idx, svm, 2, 0.005, &kept1);
    print_chain("3", kept3, handles3);
    print_chain("1", kept1, handles1);
    std::printf("SAME %d\n", same_chain(kept3, handles3, kept1, handles1) ? 1 : 0);
    // the next capture can be staged under a filtering chain
    // (fresh copies: localizeHandlesEnd filters the NaNs out of its capture in place)
    PointCloud::Ptr ca(new PointCloud(*c.cloud)), cn(new PointCloud(*c.cloud));
    if (!loc.localizeHandlesBegin(ca, c.size_left, c.idx, svm, 2, 0.005))
      return 3;
    const bool staged = loc.stageNextCloud(cn);
    std::vector<GraspHypothesis> kept_a, kept_b;
    std::vector<Handle> handles_a = loc.localizeHandlesEnd(&kept_a);
    if (!loc.localizeHandlesBegin(cn, c.size_left, c.idx, svm, 2, 0.005))
      return 4;
    std::vector<Handle> handles_b = loc.localizeHandlesEnd(&kept_b);
    std::printf("STAGE %d %d %d\n", staged ? 1 : 0, same_chain(kept_a, handles_a, kept1, handles1) ? 1 : 0,
      same_chain(kept_b, handles_b, kept1, handles1) ? 1 : 0);
    return 0;
  }
  if (std::strcmp(argv[1], "stream") == 0 && argc >= 6)
  {
    Capture c[3];
    for (int k = 0; k < 3; k++)
      if (!read_capture(argv[3 + k], c[k]))
        return 2;
    Localization ref(4, true, 0), loc(4, true, 0);
    setup(ref, c[0]);
    setup(loc, c[0]);
    std::vector<GraspHypothesis> kept_ref[3];
    std::vector<Handle> handles_ref[3];
    for (int k = 0; k < 3; k++)
    {
      PointCloud::Ptr copy(new PointCloud(*c[k].cloud));
      handles_ref[k] = ref.localizeHandles(copy, c[k].size_left, c[k].idx, svm, 2, 0.005, &kept_ref[k]);
    }
    if (!loc.localizeHandlesBegin(c[0].cloud, c[0].size_left, c[0].idx, svm, 2, 0.005))
      return 3;
    for (int k = 0; k < 3; k++)
    {
      const bool staged = k + 1 < 3 ? loc.stageNextCloud(c[k + 1].cloud) : true;
      std::vector<GraspHypothesis> kept;
      std::vector<Handle> handles = loc.localizeHandlesEnd(&kept);
      if (k + 1 < 3 && !loc.localizeHandlesBegin(c[k + 1].cloud, c[k + 1].size_left, c[k + 1].idx, svm, 2, 0.005))
        return 5;
      std::printf("STREAM %d %d %zu %zu %d\n", k, staged ? 1 : 0, kept.size(), handles.size(),
        same_chain(kept, handles, kept_ref[k], handles_ref[k]) ? 1 : 0);
    }
    return 0;
  }
  return 2;
}
