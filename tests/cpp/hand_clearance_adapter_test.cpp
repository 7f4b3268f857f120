// hand_clearance_adapter_test.cpp -- the adapter's hand-clearance methods (include/agile_grasp_amd/hand_search.h, localization.h):
// setHandClearance, clearHandClearance, handClearance and handClearanceCounts on Localization and on HandSearch, used the way a
// caller would; compiled in both type branches and run by tests/test_hand_clearance_adapter.py.
//   hand_clearance_adapter_test <svm file> <raw.bin> <near> <far> <half width> <half height> <max points>
//       localizeHandles on the capture without a clearance, with it (twice: the setting is sticky, and survives a setter that
//       re-creates the search), refused mid-chain, and cleared.  raw.bin as chain_common.h reads it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chain_common.h"

int main(int argc, char** argv)
{
  if (argc < 8)
    return 2;
  const char* svm = argv[1];
  Capture c;
  if (!read_capture(argv[2], c))
    return 2;
  agh_hand_clearance_params cp;
  agh_default_hand_clearance_params(&cp);
  const bool defaults = cp.near_offset == 0.0 && cp.far_offset == 0.12 && cp.half_width == 0.05 && cp.half_height == 0.04 &&
                        cp.max_points == 0 && cp.reserved == 0;
  cp.near_offset = std::atof(argv[3]);
  cp.far_offset = std::atof(argv[4]);
  cp.half_width = std::atof(argv[5]);
  cp.half_height = std::atof(argv[6]);
  cp.max_points = std::atoi(argv[7]);

  Localization loc(4, false, 0);
  setup(loc, c);
  agh_hand_clearance_params held;
  const bool none_before = !loc.handClearance(held) && loc.handClearanceCounts().empty();
  std::vector<GraspHypothesis> kept_plain, kept_a, kept_b, kept_c, kept_d;
  PointCloud::Ptr c0(new PointCloud(*c.cloud)), c1(new PointCloud(*c.cloud)), c2(new PointCloud(*c.cloud)),
    c3(new PointCloud(*c.cloud)), c4(new PointCloud(*c.cloud));
  std::vector<Handle> h_plain = loc.localizeHandles(c0, c.size_left, c.idx, svm, 2, 0.005, &kept_plain);
  const bool unset_counts = loc.handClearanceCounts().empty();

  const bool set = loc.setHandClearance(cp);
  const bool has = loc.handClearance(held) && held.far_offset == cp.far_offset && held.max_points == cp.max_points;
  agh_hand_clearance_params bad = cp;
  bad.far_offset = 0.6;  // refused: the setting held before stays in force
  const bool refused = !loc.setHandClearance(bad);
  const bool kept = loc.handClearance(held) && held.far_offset == cp.far_offset;
  std::vector<Handle> h_a = loc.localizeHandles(c1, c.size_left, c.idx, svm, 2, 0.005, &kept_a);
  const std::vector<agh_hand_clearance_counts> counts = loc.handClearanceCounts();
  if (counts.size() == 1)
    std::printf("COUNTS %lld %lld %lld\n", (long long) counts[0].n_tested, (long long) counts[0].n_dropped, (long long) counts[0].n_kept);
  const bool no_filter_counts = loc.handFilterCounts().empty();  // (only a clearance is set)

  // a setter that re-creates the search: the clearance follows
  loc.setHandHeight(0.021);
  loc.setHandHeight(0.02);
  std::vector<Handle> h_b = loc.localizeHandles(c2, c.size_left, c.idx, svm, 2, 0.005, &kept_b);
  const bool sticky = same_chain(kept_a, h_a, kept_b, h_b) && loc.handClearanceCounts().size() == 1;

  // refused while a chain is pending, the chain untouched
  bool mid_refused = false, mid_same = false;
  if (loc.localizeHandlesBegin(c3, c.size_left, c.idx, svm, 2, 0.005))
  {
    mid_refused = !loc.setHandClearance(cp) && !loc.clearHandClearance() && loc.handClearanceCounts().empty();
    std::vector<Handle> h_c = loc.localizeHandlesEnd(&kept_c);
    mid_same = same_chain(kept_a, h_a, kept_c, h_c);
  }

  const bool cleared = loc.clearHandClearance() && !loc.handClearance(held);
  std::vector<Handle> h_d = loc.localizeHandles(c4, c.size_left, c.idx, svm, 2, 0.005, &kept_d);
  const bool plain_again = same_chain(kept_plain, h_plain, kept_d, h_d) && loc.handClearanceCounts().empty();

  HandSearch& search = loc.getHandSearch();
  const bool s_set = search.setHandClearance(cp);
  const bool s_has = search.handClearance(held) && held.half_width == cp.half_width;
  const std::size_t s_lists = search.handClearanceCounts().size();
  const bool s_cleared = search.clearHandClearance() && !search.handClearance(held);
  std::printf("PLAIN %zu %zu\nCLEAR %zu %zu\n", kept_plain.size(), h_plain.size(), kept_a.size(), h_a.size());
  for (size_t i = 0; i < kept_a.size(); i++)
    std::printf("K %.17g %.17g %.17g %.17g\n", kept_a[i].getGraspSurface()(0), kept_a[i].getGraspSurface()(1),
      kept_a[i].getGraspSurface()(2), kept_a[i].getGraspWidth());
  std::printf("LOCALIZATION %d %d %d %d %d %d %d %d %d %d %d %d %d\nSEARCH %d %d %zu %d\n", defaults ? 1 : 0, none_before ? 1 : 0,
    unset_counts ? 1 : 0, set ? 1 : 0, has ? 1 : 0, refused ? 1 : 0, kept ? 1 : 0, no_filter_counts ? 1 : 0, sticky ? 1 : 0,
    mid_refused ? 1 : 0, mid_same ? 1 : 0, cleared ? 1 : 0, plain_again ? 1 : 0, s_set ? 1 : 0, s_has ? 1 : 0, s_lists,
    s_cleared ? 1 : 0);
  return 0;
}
