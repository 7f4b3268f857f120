// hand_filter_adapter_test.cpp -- the adapter's hand-filter methods (include/agile_grasp_amd/hand_search.h, localization.h):
// setHandFilter, clearHandFilter, handFilter and handFilterCounts on Localization and on HandSearch, used the way a caller
// would; compiled in both type branches by tests/test_hand_filter_abi.py and run by tests/test_hand_filter_adapter.py.
//   hand_filter_adapter_test <svm file> <raw.bin> <dx> <dy> <dz> <min cos> <min width> <max width>
//       localizeHandles on the capture without a filter, with the approach cone and the aperture (twice: the setting is sticky,
//       and survives a setter that re-creates the search), refused mid-chain, refused with the observed-space criterion (the
//       capture is points), and cleared.  raw.bin as chain_common.h reads it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chain_common.h"

int main(int argc, char** argv)
{
  if (argc < 9)
    return 2;
  const char* svm = argv[1];
  Capture c;
  if (!read_capture(argv[2], c))
    return 2;
  agh_hand_filter_params fp;
  agh_default_hand_filter_params(&fp);
  const bool defaults = fp.approach_on == 0 && fp.width_on == 0 && fp.view_on == 0 && fp.probes_per_finger == 4 &&
                        fp.depth_margin == 0.01 && fp.max_unobserved == 0 && fp.min_approach_cos == -1.0;
  fp.approach_on = 1;
  for (int k = 0; k < 3; k++)
    fp.approach_dir[k] = std::atof(argv[3 + k]);
  fp.min_approach_cos = std::atof(argv[6]);
  fp.width_on = 1;
  fp.min_width = std::atof(argv[7]);
  fp.max_width = std::atof(argv[8]);

  Localization loc(4, false, 0);
  setup(loc, c);
  agh_hand_filter_params held;
  const bool none_before = !loc.handFilter(held) && loc.handFilterCounts().empty();
  std::vector<GraspHypothesis> kept_plain, kept_a, kept_b, kept_c, kept_d, kept_e;
  PointCloud::Ptr c0(new PointCloud(*c.cloud)), c1(new PointCloud(*c.cloud)), c2(new PointCloud(*c.cloud)),
    c3(new PointCloud(*c.cloud)), c4(new PointCloud(*c.cloud)), c5(new PointCloud(*c.cloud));
  std::vector<Handle> h_plain = loc.localizeHandles(c0, c.size_left, c.idx, svm, 2, 0.005, &kept_plain);
  const bool unfiltered_counts = loc.handFilterCounts().empty();

  const bool set = loc.setHandFilter(fp);
  const bool has = loc.handFilter(held) && held.approach_on == 1 && held.max_width == fp.max_width;
  agh_hand_filter_params bad = fp;
  bad.min_width = fp.max_width + 0.01;  // refused: the filter held before stays in force
  const bool refused = !loc.setHandFilter(bad);
  const bool kept = loc.handFilter(held) && held.min_width == fp.min_width;
  std::vector<Handle> h_a = loc.localizeHandles(c1, c.size_left, c.idx, svm, 2, 0.005, &kept_a);
  const std::vector<agh_hand_filter_counts> counts = loc.handFilterCounts();
  if (counts.size() == 1)
    std::printf("COUNTS %lld %lld %lld %lld %lld\n", (long long) counts[0].n_hypotheses, (long long) counts[0].n_dropped_approach,
      (long long) counts[0].n_dropped_width, (long long) counts[0].n_dropped_unobserved, (long long) counts[0].n_kept);

  // a setter that re-creates the search: the filter follows
  loc.setHandHeight(0.021);
  loc.setHandHeight(0.02);
  std::vector<Handle> h_b = loc.localizeHandles(c2, c.size_left, c.idx, svm, 2, 0.005, &kept_b);
  const bool sticky = same_chain(kept_a, h_a, kept_b, h_b) && loc.handFilterCounts().size() == 1;

  // refused while a chain is pending, the chain untouched
  bool mid_refused = false, mid_same = false;
  if (loc.localizeHandlesBegin(c3, c.size_left, c.idx, svm, 2, 0.005))
  {
    mid_refused = !loc.setHandFilter(fp) && !loc.clearHandFilter() && loc.handFilterCounts().empty();
    std::vector<Handle> h_c = loc.localizeHandlesEnd(&kept_c);
    mid_same = same_chain(kept_a, h_a, kept_c, h_c);
  }
  // the observed-space criterion needs depth images: a points call fails, it does not skip the test
  agh_hand_filter_params view = fp;
  view.view_on = 1;
  const bool view_set = loc.setHandFilter(view);
  std::vector<Handle> h_e = loc.localizeHandles(c5, c.size_left, c.idx, svm, 2, 0.005, &kept_e);
  const bool view_refused = view_set && h_e.empty() && kept_e.empty();

  const bool cleared = loc.clearHandFilter() && !loc.handFilter(held);
  std::vector<Handle> h_d = loc.localizeHandles(c4, c.size_left, c.idx, svm, 2, 0.005, &kept_d);
  const bool plain_again = same_chain(kept_plain, h_plain, kept_d, h_d) && loc.handFilterCounts().empty();

  HandSearch& search = loc.getHandSearch();
  const bool s_set = search.setHandFilter(fp);
  const bool s_has = search.handFilter(held) && held.min_approach_cos == fp.min_approach_cos;
  const std::size_t s_lists = search.handFilterCounts().size();
  const bool s_cleared = search.clearHandFilter() && !search.handFilter(held);
  std::printf("PLAIN %zu %zu\nFILTERED %zu %zu\n", kept_plain.size(), h_plain.size(), kept_a.size(), h_a.size());
  for (size_t i = 0; i < kept_a.size(); i++)
    std::printf("K %.17g %.17g %.17g %.17g\n", kept_a[i].getGraspSurface()(0), kept_a[i].getGraspSurface()(1),
      kept_a[i].getGraspSurface()(2), kept_a[i].getGraspWidth());
  std::printf("LOCALIZATION %d %d %d %d %d %d %d %d %d %d %d %d %d\nSEARCH %d %d %zu %d\n", defaults ? 1 : 0, none_before ? 1 : 0,
    unfiltered_counts ? 1 : 0, set ? 1 : 0, has ? 1 : 0, refused ? 1 : 0, kept ? 1 : 0, sticky ? 1 : 0, mid_refused ? 1 : 0,
    mid_same ? 1 : 0, view_refused ? 1 : 0, cleared ? 1 : 0, plain_again ? 1 : 0, s_set ? 1 : 0, s_has ? 1 : 0, s_lists,
    s_cleared ? 1 : 0);
  return 0;
}
