// batch_cluster_adapter_test.cpp -- the adapter's clustered batch calls (include/agile_grasp_amd/localization.h,
// include/agile_grasp_amd/hand_search.h) have the documented types, in both type branches: compiled, not run.  A plane per
// capture; an optional vector of per-capture cluster records; collected by localizeHandlesBatchLabeledEnd.
#include <string>
#include <type_traits>
#include <vector>

#include "chain_common.h"

typedef std::vector<std::vector<std::vector<GraspHypothesis> > > KeptLists;
typedef std::vector<std::vector<std::vector<Handle> > > HandleLists;
typedef std::vector<PointCloud::Ptr> Clouds;
typedef std::vector<std::vector<DepthImage> > Captures;
typedef std::vector<VectorXd> Vectors;
typedef std::vector<agh_cluster_params> Records;

typedef HandleLists (Localization::*points_fn)(const Clouds&, const std::vector<int>&, const Vectors&, const std::string&, int, double,
  KeptLists*, const Vectors*, const Records*);
typedef bool (Localization::*points_begin_fn)(const Clouds&, const std::vector<int>&, const Vectors&, const std::string&, int, double,
  const Vectors*, const Records*);
typedef HandleLists (Localization::*depth_fn)(const Captures&, const Vectors&, const std::string&, int, double, KeptLists*,
  const Vectors*, const Records*);
typedef bool (Localization::*depth_begin_fn)(const Captures&, const Vectors&, const std::string&, int, double, const Vectors*,
  const Records*);
static_assert(std::is_same<decltype(&Localization::localizeHandlesBatchClustered), points_fn>::value, "localizeHandlesBatchClustered");
static_assert(std::is_same<decltype(&Localization::localizeHandlesBatchClusteredBegin), points_begin_fn>::value,
  "localizeHandlesBatchClusteredBegin");
static_assert(std::is_same<decltype(&Localization::localizeHandlesDepthBatchClustered), depth_fn>::value,
  "localizeHandlesDepthBatchClustered");
static_assert(std::is_same<decltype(&Localization::localizeHandlesDepthBatchClusteredBegin), depth_begin_fn>::value,
  "localizeHandlesDepthBatchClusteredBegin");

typedef bool (HandSearch::*search_points_fn)(const Clouds&, const std::vector<int>&, const Records&, const Vectors&, double,
  const std::string&, int, double, bool);
typedef bool (HandSearch::*search_depth_fn)(const Captures&, const Records&, const Vectors&, double, const std::string&, int, double,
  bool);
typedef bool (HandSearch::*info_fn)(std::vector<agh_cluster_info>&, std::vector<std::int64_t>&, std::vector<std::int32_t>&);
static_assert(std::is_same<decltype(&HandSearch::localizeBatchClusteredBegin), search_points_fn>::value, "localizeBatchClusteredBegin");
static_assert(std::is_same<decltype(&HandSearch::localizeDepthBatchClusteredBegin), search_depth_fn>::value,
  "localizeDepthBatchClusteredBegin");
static_assert(std::is_same<decltype(&HandSearch::batchClusterInfo), info_fn>::value, "batchClusterInfo");

// every call instantiated as a cell with two rigs would make it: setClusterParams' record for both, then a record per rig
HandleLists two_rigs(Localization& loc, const Clouds& clouds, const Captures& captures, const std::string& svm, KeptLists* kept)
{
  Vectors planes(2, VectorXd(4));
  for (int k = 0; k < 2; k++)
  {
    planes[k](0) = 0.0;
    planes[k](1) = 0.0;
    planes[k](2) = 1.0;
    planes[k](3) = 0.1 * k;
  }
  const std::vector<int> sizes_left(2, 1);
  loc.setClusterParams(0.01, 0.5, 0.01, 50, 8);
  HandleLists out = loc.localizeHandlesBatchClustered(clouds, sizes_left, planes, svm, 2, 0.005, kept);
  Records records(2);
  agh_default_cluster_params(&records[0]);
  agh_default_cluster_params(&records[1]);
  records[1].max_objects = 3;
  if (loc.localizeHandlesBatchClusteredBegin(clouds, sizes_left, planes, svm, 2, 0.005, nullptr, &records))
    out = loc.localizeHandlesBatchLabeledEnd(kept);
  out = loc.localizeHandlesDepthBatchClustered(captures, planes, svm, 2, 0.005, kept, nullptr, &records);
  if (loc.localizeHandlesDepthBatchClusteredBegin(captures, planes, svm, 2, 0.005))
    out = loc.localizeHandlesBatchLabeledEnd();
  const std::vector<std::int64_t> sizes = loc.getBatchClusterSizes();
  (void) sizes;
  return out;
}

int main() { return 0; }
