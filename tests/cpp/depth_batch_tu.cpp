// Compile-only translation unit (`g++ -fsyntax-only`, in both branches of include/agile_grasp_amd/types.h) for the depth-batch
// calls of the adapter: HandSearch::localizeDepthBatch / localizeDepthBatchBegin and Localization::localizeHandlesDepthBatch
// (with and without per-capture camera transforms) / localizeHandlesDepthBatchBegin, collected by localizeHandlesBatchEnd --
// called the way a cell with several sensor pairs calls them.
#include <cstdint>
#include <string>
#include <vector>

#include <agile_grasp_amd/hand_search.h>
#include <agile_grasp_amd/localization.h>

using namespace agile_grasp_amd;

// every sensor pair of the cell in one call
std::vector<std::vector<Handle> > cell_depth_batch(Localization& loc, const std::vector<std::vector<DepthImage> >& pairs,
  const std::string& svm_file_name, int min_inliers)
{
  const std::vector<std::vector<int> > indices(pairs.size());
  std::vector<std::vector<GraspHypothesis> > antipodal_hands;
  return loc.localizeHandlesDepthBatch(pairs, indices, svm_file_name, min_inliers, 0.005, &antipodal_hands);
}

// the two halves, with a workspace per pair
std::vector<std::vector<Handle> > cell_depth_batch_halves(Localization& loc, const std::vector<std::vector<DepthImage> >& pairs,
  const std::vector<VectorXd>& workspaces, const std::string& svm_file_name)
{
  const std::vector<std::vector<int> > indices(pairs.size());
  if (!loc.localizeHandlesDepthBatchBegin(pairs, indices, svm_file_name, 3, 0.005, &workspaces))
    return std::vector<std::vector<Handle> >();
  return loc.localizeHandlesBatchEnd();
}

// pairs of several rigs: one left and one right transform per pair
std::vector<std::vector<Handle> > cell_depth_batch_rigs(Localization& loc, const std::vector<std::vector<DepthImage> >& pairs,
  const std::vector<Matrix4d>& cams_left, const std::vector<Matrix4d>& cams_right, const std::string& svm_file_name)
{
  const std::vector<std::vector<int> > indices(pairs.size());
  return loc.localizeHandlesDepthBatch(pairs, indices, svm_file_name, 3, 0.005, cams_left, cams_right);
}

// the same one level down
bool cell_hand_search_depth_batch(HandSearch& search, const std::vector<std::vector<DepthImage> >& pairs, const VectorXd& workspace,
  const std::string& svm_file_name)
{
  const std::vector<VectorXd> workspaces(pairs.size(), workspace);
  const std::vector<std::vector<int> > indices(pairs.size());
  std::vector<std::vector<agh_hypothesis> > hands;
  std::vector<std::vector<agh_handle> > handles;
  std::vector<std::vector<std::int32_t> > inliers;
  if (!search.localizeDepthBatchBegin(pairs, workspaces, 0.003, indices, svm_file_name, 3, 0.005, true))
    return false;
  return search.localizeBatchEnd(hands, handles, inliers) &&
         search.localizeDepthBatch(pairs, workspaces, 0.003, indices, svm_file_name, 3, 0.005, hands, handles, inliers);
}
