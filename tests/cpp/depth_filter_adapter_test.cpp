// depth_filter_adapter_test.cpp -- the adapter's depth-filter methods (include/agile_grasp_amd/hand_search.h, localization.h):
// setDepthFilter, clearDepthFilter, depthFilter and depthFilterCounts on HandSearch and on Localization, used the way a caller
// would; compiled in both type branches by tests/test_depth_filter_abi.py.
//   depth_filter_adapter_test   prints what the calls return (they need a device only once a context exists)
#include <cstdio>
#include <vector>

#include "chain_common.h"

int main()
{
  agh_depth_filter_params fp;
  agh_default_depth_filter_params(&fp);
  fp.radius = 2;
  fp.min_support = 5;
  fp.z_max = 3.0;

  Localization loc(1, false, 0);
  agh_depth_filter_params held;
  const bool none_before = !loc.depthFilter(held) && loc.depthFilterCounts().empty();
  const bool set = loc.setDepthFilter(fp);
  const bool has = loc.depthFilter(held) && held.radius == 2 && held.min_support == 5 && held.z_max == 3.0;
  fp.radius = 3;  // refused: the filter held before stays in force
  const bool refused = !loc.setDepthFilter(fp);
  const bool kept = loc.depthFilter(held) && held.radius == 2;
  const std::vector<agh_depth_filter_counts> counts = loc.depthFilterCounts();
  long long n_kept = 0;
  for (std::size_t k = 0; k < counts.size(); k++)
    n_kept += counts[k].n_kept + 0 * (counts[k].n_valid + counts[k].n_out_of_range + counts[k].n_unsupported);
  const bool cleared = loc.clearDepthFilter() && !loc.depthFilter(held);

  HandSearch& search = loc.getHandSearch();
  fp.radius = 1;
  fp.min_support = 3;
  const bool s_set = search.setDepthFilter(fp);
  const bool s_has = search.depthFilter(held) && held.radius == 1;
  const std::size_t s_views = search.depthFilterCounts().size();
  const bool s_cleared = search.clearDepthFilter() && !search.depthFilter(held);
  std::printf("LOCALIZATION %d %d %d %d %d %lld %d\nSEARCH %d %d %zu %d\n", none_before ? 1 : 0, set ? 1 : 0, has ? 1 : 0, refused ? 1 : 0,
    kept ? 1 : 0, n_kept, cleared ? 1 : 0, s_set ? 1 : 0, s_has ? 1 : 0, s_views, s_cleared ? 1 : 0);
  return 0;
}
