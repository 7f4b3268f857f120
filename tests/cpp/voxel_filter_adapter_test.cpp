// voxel_filter_adapter_test.cpp -- the adapter's voxel-filter methods (include/agile_grasp_amd/hand_search.h, localization.h):
// setVoxelFilter, clearVoxelFilter, voxelFilter and voxelFilterCounts on Localization and on HandSearch, used the way a caller
// would; compiled in both type branches by tests/test_voxel_filter_abi.py and run by tests/test_voxel_filter_adapter.py.
//   voxel_filter_adapter_test <svm file> <raw.bin> <radius> <min_neighbors>
//       localizeHandles on the capture without a filter, with it (twice: the setting is sticky, and survives a setter that
//       re-creates the search), refused mid-chain, and cleared.  raw.bin as chain_common.h reads it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chain_common.h"

static long long sum2(const std::int64_t v[2])
{
  return (long long) (v[0] + v[1]);
}

int main(int argc, char** argv)
{
  if (argc < 5)
    return 2;
  const char* svm = argv[1];
  Capture c;
  if (!read_capture(argv[2], c))
    return 2;
  agh_voxel_filter_params fp;
  agh_default_voxel_filter_params(&fp);
  const bool defaults = fp.radius == 2 && fp.min_neighbors == 4;
  fp.radius = std::atoi(argv[3]);
  fp.min_neighbors = std::atoi(argv[4]);

  Localization loc(4, false, 0);
  setup(loc, c);
  agh_voxel_filter_params held;
  const bool none_before = !loc.voxelFilter(held) && loc.voxelFilterCounts().empty();
  std::vector<GraspHypothesis> kept_plain, kept_a, kept_b, kept_c, kept_d;
  PointCloud::Ptr c0(new PointCloud(*c.cloud)), c1(new PointCloud(*c.cloud)), c2(new PointCloud(*c.cloud)),
    c3(new PointCloud(*c.cloud)), c4(new PointCloud(*c.cloud));
  std::vector<Handle> h_plain = loc.localizeHandles(c0, c.size_left, c.idx, svm, 2, 0.005, &kept_plain);
  const bool unfiltered_counts = loc.voxelFilterCounts().empty();

  const bool set = loc.setVoxelFilter(fp);
  const bool has = loc.voxelFilter(held) && held.radius == fp.radius && held.min_neighbors == fp.min_neighbors;
  agh_voxel_filter_params bad = fp;
  bad.radius = 5;  // refused: the filter held before stays in force
  const bool refused = !loc.setVoxelFilter(bad);
  const bool kept = loc.voxelFilter(held) && held.radius == fp.radius;
  std::vector<Handle> h_a = loc.localizeHandles(c1, c.size_left, c.idx, svm, 2, 0.005, &kept_a);
  const std::vector<agh_voxel_filter_counts> counts = loc.voxelFilterCounts();
  if (counts.size() == 1)
    std::printf("COUNTS %lld %lld %lld %lld %lld %lld\n", (long long) counts[0].n_occupied[0], (long long) counts[0].n_occupied[1],
      (long long) counts[0].n_pruned[0], (long long) counts[0].n_pruned[1], (long long) counts[0].n_kept[0],
      (long long) counts[0].n_kept[1]);
  const bool adds_up = counts.size() == 1 && sum2(counts[0].n_occupied) == sum2(counts[0].n_pruned) + sum2(counts[0].n_kept);

  // a setter that re-creates the search: the filter follows
  loc.setHandHeight(0.021);
  loc.setHandHeight(0.02);
  std::vector<Handle> h_b = loc.localizeHandles(c2, c.size_left, c.idx, svm, 2, 0.005, &kept_b);
  const bool sticky = same_chain(kept_a, h_a, kept_b, h_b) && loc.voxelFilterCounts().size() == 1;

  // refused while a chain is pending, the chain untouched
  bool mid_refused = false, mid_same = false;
  if (loc.localizeHandlesBegin(c3, c.size_left, c.idx, svm, 2, 0.005))
  {
    mid_refused = !loc.setVoxelFilter(fp) && !loc.clearVoxelFilter() && loc.voxelFilterCounts().empty();
    std::vector<Handle> h_c = loc.localizeHandlesEnd(&kept_c);
    mid_same = same_chain(kept_a, h_a, kept_c, h_c);
  }
  const bool cleared = loc.clearVoxelFilter() && !loc.voxelFilter(held);
  std::vector<Handle> h_d = loc.localizeHandles(c4, c.size_left, c.idx, svm, 2, 0.005, &kept_d);
  const bool plain_again = same_chain(kept_plain, h_plain, kept_d, h_d) && loc.voxelFilterCounts().empty();

  HandSearch& search = loc.getHandSearch();
  const bool s_set = search.setVoxelFilter(fp);
  const bool s_has = search.voxelFilter(held) && held.min_neighbors == fp.min_neighbors;
  const std::size_t s_captures = search.voxelFilterCounts().size();
  const bool s_cleared = search.clearVoxelFilter() && !search.voxelFilter(held);
  std::printf("PLAIN %zu %zu\nFILTERED %zu %zu\n", kept_plain.size(), h_plain.size(), kept_a.size(), h_a.size());
  std::printf("LOCALIZATION %d %d %d %d %d %d %d %d %d %d %d %d %d\nSEARCH %d %d %zu %d\n", defaults ? 1 : 0, none_before ? 1 : 0,
    unfiltered_counts ? 1 : 0, set ? 1 : 0, has ? 1 : 0, refused ? 1 : 0, kept ? 1 : 0, adds_up ? 1 : 0, sticky ? 1 : 0,
    mid_refused ? 1 : 0, mid_same ? 1 : 0, cleared ? 1 : 0, plain_again ? 1 : 0, s_set ? 1 : 0, s_has ? 1 : 0, s_captures,
    s_cleared ? 1 : 0);
  return 0;
}
