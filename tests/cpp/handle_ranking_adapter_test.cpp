// handle_ranking_adapter_test.cpp -- the adapter's handle-ranking methods (include/agile_grasp_amd/hand_search.h, localization.h):
// setHandleRanking, clearHandleRanking, handleRanking, handleScores, handleRankingCounts and handMargins on Localization and on
// HandSearch, used the way a caller would; compiled in both type branches and run by tests/test_handle_ranking_adapter.py.
//   handle_ranking_adapter_test <svm file> <raw.bin> <w_support> <w_margin> <w_length> <max handles>
//       localizeHandles on the capture without a ranking, with it (twice: the setting is sticky, and survives a setter that
//       re-creates the search), refused mid-chain, and cleared.  raw.bin as chain_common.h reads it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chain_common.h"

int main(int argc, char** argv)
{
  if (argc < 7)
    return 2;
  const char* svm = argv[1];
  Capture c;
  if (!read_capture(argv[2], c))
    return 2;
  agh_handle_ranking_params rp;
  agh_default_handle_ranking_params(&rp);
  const bool defaults = rp.w_support == 1.0 && rp.w_margin == 1.0 && rp.w_approach == 0.0 && rp.w_length == 0.0 &&
                        rp.approach_dir[2] == -1.0 && rp.position_dir[2] == 1.0 && rp.min_score < -1e300 && rp.support_cap == 10 &&
                        rp.max_handles == 0;
  rp.w_support = std::atof(argv[3]);
  rp.w_margin = std::atof(argv[4]);
  rp.w_length = std::atof(argv[5]);
  rp.max_handles = std::atoi(argv[6]);

  Localization loc(4, false, 0);
  setup(loc, c);
  agh_handle_ranking_params held = agh_handle_ranking_params();
  const bool none_before = !loc.handleRanking(held) && loc.handleScores().empty() && loc.handleRankingCounts().empty();
  std::vector<GraspHypothesis> kept_plain, kept_a, kept_b, kept_c, kept_d;
  PointCloud::Ptr c0(new PointCloud(*c.cloud)), c1(new PointCloud(*c.cloud)), c2(new PointCloud(*c.cloud)),
    c3(new PointCloud(*c.cloud)), c4(new PointCloud(*c.cloud));
  std::vector<Handle> h_plain = loc.localizeHandles(c0, c.size_left, c.idx, svm, 2, 0.005, &kept_plain);
  const bool unset_empty = loc.handleScores().empty() && loc.handMargins().empty();

  const bool set = loc.setHandleRanking(rp);
  const bool has = loc.handleRanking(held) && held.w_length == rp.w_length && held.max_handles == rp.max_handles;
  agh_handle_ranking_params bad = rp;
  bad.support_cap = 0;  // refused: the setting held before stays in force
  const bool refused = !loc.setHandleRanking(bad);
  const bool kept = loc.handleRanking(held) && held.support_cap == 10;
  std::vector<Handle> h_a = loc.localizeHandles(c1, c.size_left, c.idx, svm, 2, 0.005, &kept_a);
  const std::vector<agh_handle_score> scores = loc.handleScores();
  const std::vector<agh_handle_ranking_counts> counts = loc.handleRankingCounts();
  const std::vector<double> margins = loc.handMargins();
  if (counts.size() == 1)
    std::printf("COUNTS %lld %lld %lld\n", (long long) counts[0].n_found, (long long) counts[0].n_below, (long long) counts[0].n_returned);
  for (size_t i = 0; i < scores.size() && i < h_a.size(); i++)
    std::printf("S %.17g %d %d %.17g %.17g %.17g\n", scores[i].score, (int) scores[i].index, (int) scores[i].best_inlier,
      h_a[i].getCenter()(0), h_a[i].getCenter()(1), h_a[i].getCenter()(2));
  const bool sizes = scores.size() == h_a.size() && margins.size() == kept_a.size() && kept_a.size() == kept_plain.size();

  // a setter that re-creates the search: the ranking follows
  loc.setHandHeight(0.021);
  loc.setHandHeight(0.02);
  std::vector<Handle> h_b = loc.localizeHandles(c2, c.size_left, c.idx, svm, 2, 0.005, &kept_b);
  const bool sticky = same_chain(kept_a, h_a, kept_b, h_b) && loc.handleRankingCounts().size() == 1;

  // refused while a chain is pending, the chain untouched
  bool mid_refused = false, mid_same = false;
  if (loc.localizeHandlesBegin(c3, c.size_left, c.idx, svm, 2, 0.005))
  {
    mid_refused = !loc.setHandleRanking(rp) && !loc.clearHandleRanking() && loc.handleScores().empty() && loc.handMargins().empty();
    std::vector<Handle> h_c = loc.localizeHandlesEnd(&kept_c);
    mid_same = same_chain(kept_a, h_a, kept_c, h_c);
  }

  const bool cleared = loc.clearHandleRanking() && !loc.handleRanking(held);
  std::vector<Handle> h_d = loc.localizeHandles(c4, c.size_left, c.idx, svm, 2, 0.005, &kept_d);
  const bool plain_again = same_chain(kept_plain, h_plain, kept_d, h_d) && loc.handleScores().empty();

  HandSearch& search = loc.getHandSearch();
  const bool s_set = search.setHandleRanking(rp);
  const bool s_has = search.handleRanking(held) && held.w_margin == rp.w_margin;
  const std::size_t s_lists = search.handleRankingCounts().size();
  const bool s_cleared = search.clearHandleRanking() && !search.handleRanking(held);
  std::printf("PLAIN %zu %zu\nRANKED %zu %zu\n", kept_plain.size(), h_plain.size(), kept_a.size(), h_a.size());
  std::printf("LOCALIZATION %d %d %d %d %d %d %d %d %d %d %d %d %d\nSEARCH %d %d %zu %d\n", defaults ? 1 : 0, none_before ? 1 : 0,
    unset_empty ? 1 : 0, set ? 1 : 0, has ? 1 : 0, refused ? 1 : 0, kept ? 1 : 0, sizes ? 1 : 0, sticky ? 1 : 0,
    mid_refused ? 1 : 0, mid_same ? 1 : 0, cleared ? 1 : 0, plain_again ? 1 : 0, s_set ? 1 : 0, s_has ? 1 : 0, s_lists,
    s_cleared ? 1 : 0);
  return 0;
}
