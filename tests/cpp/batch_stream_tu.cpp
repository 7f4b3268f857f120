// Compile-only translation unit (`g++ -fsyntax-only`, in both branches of include/agile_grasp_amd/types.h: with the stand-in
// types, and with -DAGILE_GRASP_AMD_HAVE_PCL_EIGEN against tests/cpp/stubs) for the streamed batch calls of the adapter:
// HandSearch::localizeBatchBegin / localizeBatchStage / localizeBatchEnd and Localization::localizeHandlesBatchBegin /
// stageNextBatch / localizeHandlesBatchEnd, called the way a walk over a directory of captures calls them.
#include <string>
#include <vector>

#include <agile_grasp_amd/hand_search.h>
#include <agile_grasp_amd/localization.h>

using namespace agile_grasp_amd;

// batch k + 1 goes up while batch k is searched
std::vector<std::vector<Handle> > site_directory_walk(Localization& loc, const std::vector<std::vector<PointCloud::Ptr> >& batches,
  const std::vector<std::vector<int> >& sizes_left, const std::string& svm_file_name, int min_inliers)
{
  std::vector<std::vector<Handle> > all;
  if (batches.empty())
    return all;
  std::vector<std::vector<GraspHypothesis> > antipodal_hands;
  std::vector<std::vector<int> > indices(batches[0].size());
  if (!loc.localizeHandlesBatchBegin(batches[0], sizes_left[0], indices, svm_file_name, min_inliers, 0.005))
    return all;
  for (std::size_t k = 0; k < batches.size(); k++)
  {
    if (k + 1 < batches.size())
      (void) loc.stageNextBatch(batches[k + 1]);
    const std::vector<std::vector<Handle> > handles = loc.localizeHandlesBatchEnd(&antipodal_hands);
    all.insert(all.end(), handles.begin(), handles.end());
    if (k + 1 < batches.size())
    {
      indices.assign(batches[k + 1].size(), std::vector<int>());
      if (!loc.localizeHandlesBatchBegin(batches[k + 1], sizes_left[k + 1], indices, svm_file_name, min_inliers, 0.005))
        break;
    }
  }
  return all;
}

// the same one level down, with a workspace per capture
bool site_hand_search_batch(HandSearch& search, const std::vector<PointCloud::Ptr>& now, const std::vector<PointCloud::Ptr>& next,
  const std::vector<int>& sizes_left, const std::vector<VectorXd>& workspaces, const std::string& svm_file_name)
{
  std::vector<std::vector<int> > indices(now.size());
  std::vector<std::vector<agh_hypothesis> > hands;
  std::vector<std::vector<agh_handle> > handles;
  std::vector<std::vector<std::int32_t> > inliers;
  if (!search.localizeBatchBegin(now, sizes_left, workspaces, 0.003, indices, svm_file_name, 3, 0.005, true))
    return false;
  const bool staged = search.localizeBatchStage(next);
  return search.localizeBatchEnd(hands, handles, inliers) && staged;
}
