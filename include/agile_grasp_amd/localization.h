// localization.h -- the Localization facade (include/agile_grasp/localization.h:64-351) over the MI355X hand search.
//
// Kept: constructors, every setter, localizeHands(cloud, size_left, indices, calculates_antipodal, uses_clustering) and
// its two PCD-filename overloads (pcd_io.h reads PCD files when PCL is absent), predictAntipodalHands(hand_list,
// svm_filename), findHandles(hand_list, min_inliers, min_length), filterHands.  The preprocessing that precedes the hot
// path (NaN removal, workspace box, per-camera 3 mm voxelisation: localization.cpp:25-45, 216-355; its output ORDER
// defines the point indices the search works on) runs on the GPU as well (agh_preprocess).
// uses_clustering = true removes the table plane before the search as localization.cpp:51-98 does (pcl::SACSegmentation's
// RANSAC restated on the GPU: agh_remove_plane); explicit indices together with it are refused (see localizeHands).
// Not carried over: the Plot members.
#ifndef AGILE_GRASP_AMD_LOCALIZATION_H
#define AGILE_GRASP_AMD_LOCALIZATION_H

#include <cmath>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "hand_search.h"
#include "handle_search.h"
#include "learning.h"
#include "pcd_io.h"

namespace agile_grasp_amd
{

class Localization
{
public:
  Localization() : num_threads_(1), num_samples_(2000), filters_boundaries_(false), plotting_mode_(0) { init(); }
  Localization(int num_threads, bool filters_boundaries, int plotting_mode)
    : num_threads_(num_threads), num_samples_(2000), filters_boundaries_(filters_boundaries), plotting_mode_(plotting_mode)
  {
    init();
  }

  // ---- setters (localization.h:148-259) ----
  void setCameraTransforms(const Matrix4d& cam_tf_left, const Matrix4d& cam_tf_right)
  {
    cam_tf_left_ = cam_tf_left;
    cam_tf_right_ = cam_tf_right;
    search_.reset();
  }
  const Matrix4d& getCameraTransform(bool is_left) { return is_left ? cam_tf_left_ : cam_tf_right_; }
  void setWorkspace(const VectorXd& workspace) { workspace_ = workspace; }
  void setNumSamples(int num_samples)
  {
    num_samples_ = num_samples;
    search_.reset();
  }
  // stored but never forwarded, exactly like the reference (localization.h:189-201 vs localization.cpp:111-112)
  void setNeighborhoodRadiusHands(double r) { nn_radius_hands_ = r; }
  void setNeighborhoodRadiusTaubin(double r) { nn_radius_taubin_ = r; }
  void setFingerWidth(double v)
  {
    finger_width_ = v;
    search_.reset();
  }
  void setHandDepth(double v)
  {
    hand_depth_ = v;
    search_.reset();
  }
  void setHandOuterDiameter(double v)
  {
    hand_outer_diameter_ = v;
    search_.reset();
  }
  void setInitBite(double v)
  {
    init_bite_ = v;
    search_.reset();
  }
  void setHandHeight(double v)
  {
    hand_height_ = v;
    search_.reset();
  }
  // additions: the reference hard-wires these inside HandSearch
  void setDeterministicNormalEstimation(bool b)
  {
    deterministic_ = b;
    search_.reset();
  }
  void setDevice(int device)
  {
    device_ = device;
    search_.reset();
  }
  /** Training runs (src/nodes/train.cpp): localizeHands(..., calculates_antipodal = true, ...) then returns hypotheses
   *  that carry their three instance images, the input of Learning::train / trainBalanced. */
  void setKeepsTrainingImages(bool b)
  {
    keeps_training_images_ = b;
    if (search_)
      search_->setKeepsTrainingImages(b);
  }
  /** The search the hypotheses came from: what this adapter's Learning is constructed on (train.cpp:122). */
  HandSearch& getHandSearch()
  {
    ensureSearch();
    return *search_;
  }

  /** localization.cpp:3-140 */
  std::vector<GraspHypothesis> localizeHands(const PointCloud::Ptr& cloud_in, int size_left,
    const std::vector<int>& indices, bool calculates_antipodal, bool uses_clustering)
  {
    std::vector<GraspHypothesis> hand_list;
    if (size_left == 0 || !cloud_in || cloud_in->size() == 0)
    {
      std::cout << "Input cloud is empty!\n";
      std::cout << size_left << std::endl;
      return hand_list;
    }
    // localization.cpp:17-45 on the GPU (agh_preprocess): camera id = (position >= size_left), removal of non-finite
    // points WITHOUT re-indexing the camera ids (the reference's behaviour), workspace box, per-camera 3 mm voxels in
    // lexicographic order.
    if (uses_clustering && !indices.empty())
    {
      // Explicit indices would address the cloud left after the table-plane removal, which the caller never sees (the
      // reference reads out of range once an index passes its size), so the combination fails like the reference's
      // other errors do.
      std::cout << " Error: uses_clustering with explicit indices is not supported: they would index the cloud left after "
                   "the table-plane removal; pass empty indices (samples drawn over that cloud) or uses_clustering = false\n";
      return hand_list;
    }
    std::cout << "Generating camera sources for " << cloud_in->size() << " points ...\n";
    std::cout << "Filtering workspace ...\nVoxelizing point cloud\n";
    ensureSearch();
    PointCloud::Ptr voxels;
    VectorXi pts_cam_source;
    if (!search_->preprocess(cloud_in, size_left, workspace_, 0.003, voxels, pts_cam_source))
      return hand_list;
    std::cout << " Created " << voxels->points.size() << " voxels\n";
    remove_nan_in_place(*cloud_in);  // localization.cpp:27 filters the caller's cloud in place
    if (uses_clustering)
    {
      // localization.cpp:51-98: the largest plane (the table) goes, the search runs on the rest
      std::cout << "Finding point cloud clusters ... \n";
      agh_plane_result plane;
      PointCloud::Ptr cluster;
      VectorXi cluster_cam;
      if (!search_->removePlane(plane, cluster, cluster_cam))
        return hand_list;
      if (!plane.found || plane.n_inliers == 0)
      {
        std::cout << " Could not estimate a planar model for the given dataset." << std::endl;
        return hand_list;
      }
      std::cout << " PointCloud representing the planar component: " << plane.n_inliers << " data points." << std::endl;
      std::cout << " PointCloud representing the non-planar component: " << plane.n_remaining << " data points." << std::endl;
      last_cloud_ = cluster;  // (cloud_plot, localization.cpp:95)
      last_cam_ = cluster_cam;
      if (plane.n_remaining == 0)
      {
        // the reference would go on searching an empty cloud
        std::cout << " No points left after removing the plane\n";
        return hand_list;
      }
      voxels = cluster;
      pts_cam_source = cluster_cam;
    }
    hand_list = search_->findHandsInSearchedCloud(indices, calculates_antipodal);
    if (filters_boundaries_)
    {
      std::cout << "Filtering out hands close to workspace boundaries ...\n";
      hand_list = filterHands(hand_list);
      std::cout << " # hands left: " << hand_list.size() << "\n";
    }
    last_cloud_ = voxels;
    last_cam_ = pts_cam_source;
    return hand_list;
  }

  /** localization.cpp:168-173 */
  std::vector<GraspHypothesis> localizeHands(const std::string& pcd_filename_left, const std::string& pcd_filename_right,
    bool calculates_antipodal = false, bool uses_clustering = false)
  {
    return localizeHands(pcd_filename_left, pcd_filename_right, std::vector<int>(), calculates_antipodal, uses_clustering);
  }

  /** localization.cpp:175-212 */
  std::vector<GraspHypothesis> localizeHands(const std::string& pcd_filename_left, const std::string& pcd_filename_right,
    const std::vector<int>& indices, bool calculates_antipodal = false, bool uses_clustering = false)
  {
    PointCloud::Ptr cloud_left(new PointCloud);
    if (loadPCDFile(pcd_filename_left, *cloud_left) == -1)
    {
      std::cout << "Couldn't read pcd_filename_left file: " << pcd_filename_left << " \n";
      return std::vector<GraspHypothesis>();
    }
    if (pcd_filename_right.length() > 0)
      std::cout << "Loaded left point cloud with " << cloud_left->size() << " data points.\n";
    else
      std::cout << "Loaded point cloud with " << cloud_left->size() << " data points.\n";
    PointCloud::Ptr cloud_right(new PointCloud);
    if (pcd_filename_right.length() > 0)
    {
      if (loadPCDFile(pcd_filename_right, *cloud_right) == -1)
      {
        std::cout << "Couldn't read pcd_filename_left file: " << pcd_filename_right << " \n";
        return std::vector<GraspHypothesis>();
      }
      std::cout << "Loaded right point cloud with " << cloud_right->size() << " data points.\n";
    }
    std::cout << "Concatenating point clouds ...\n";
    PointCloud::Ptr cloud(new PointCloud);
    *cloud = *cloud_left;  // *cloud_left + *cloud_right (pcl::PointCloud::operator+ also ANDs is_dense)
    cloud->points.insert(cloud->points.end(), cloud_right->points.begin(), cloud_right->points.end());
    cloud->is_dense = cloud_left->is_dense && cloud_right->is_dense;
    return localizeHands(cloud, (int) cloud_left->size(), indices, calculates_antipodal, uses_clustering);
  }

  /** localization.cpp:142-167 */
  std::vector<GraspHypothesis> predictAntipodalHands(const std::vector<GraspHypothesis>& hand_list,
    const std::string& svm_filename)
  {
    Learning learn(num_threads_);  // localization.cpp:146
    Matrix3Xd cams_mat;  // the images were rasterised with both camera origins already (localization.cpp:147-150)
    std::vector<GraspHypothesis> antipodal_hands = learn.classify(hand_list, svm_filename, cams_mat);
    std::cout << antipodal_hands.size() << " antipodal hand configurations found\n";
    return antipodal_hands;
  }

  /** localization.cpp:390-409 (the plotting branches aside) */
  std::vector<Handle> findHandles(const std::vector<GraspHypothesis>& hand_list, int min_inliers, double min_length)
  {
    HandleSearch handle_search;  // localization.cpp:392
    return handle_search.findHandles(hand_list, min_inliers, min_length);
  }

  /** Additional: what GraspLocalizer::localizeGrasps runs per cloud (grasp_localizer.cpp:95-103) --
   *      hands = localizeHands(cloud, size_left, indices, false, false);
   *      antipodal_hands = predictAntipodalHands(hands, svm_file_name);
   *      handles = findHandles(antipodal_hands, min_inliers, 0.005);
   *  -- as ONE call into the device library with one synchronisation (agh_localize: no host round trip of the hypotheses
   *  between the stages).  Same handles as the three calls on the same sample indices; with `indices` empty the samples are
   *  drawn on the device (see HandSearch::localize).  The hands the classifier kept come back through `antipodal_hands`
   *  (Handle::getHandList of every handle is that list).  With filters_boundaries (the nodes' configuration,
   *  grasp_localizer.cpp:21) the chain runs filterHands between the search and the classifier on the device: the same results
   *  as localizeHands (which filters) -> predictAntipodalHands -> findHandles. */
  std::vector<Handle> localizeHandles(const PointCloud::Ptr& cloud_in, int size_left, const std::vector<int>& indices,
    const std::string& svm_filename, int min_inliers, double min_length, std::vector<GraspHypothesis>* antipodal_hands = nullptr)
  {
    if (antipodal_hands)
      antipodal_hands->clear();
    if (!localizeHandlesBegin(cloud_in, size_left, indices, svm_filename, min_inliers, min_length))
      return std::vector<Handle>();
    return localizeHandlesEnd(antipodal_hands);
  }

  /** Additional: the same chain for a node that already holds the NEXT capture while this one is searched
   *  (GraspLocalizer::cloud_callback queues clouds, grasp_localizer.cpp:55-75):
   *      loc.localizeHandlesBegin(cloud_k, size_left, indices, svm, min_inliers, 0.005);   // queued, not waited for
   *      loc.stageNextCloud(cloud_k1);                                                     // its upload runs under cloud k's kernels
   *      handles = loc.localizeHandlesEnd(&antipodal_hands);                               // the one synchronisation
   *      loc.localizeHandlesBegin(cloud_k1, ...);                                          // finds cloud k + 1 on the device
   *  Same results as localizeHandles.  A Begin while a chain is pending returns false and leaves that chain as it was.  The
   *  clouds must stay alive and unchanged until the localizeHandlesEnd of their chain
   *  has returned (which then filters NaNs out of the searched cloud in place, as localization.cpp:27 does). */
  bool localizeHandlesBegin(const PointCloud::Ptr& cloud_in, int size_left, const std::vector<int>& indices,
    const std::string& svm_filename, int min_inliers, double min_length)
  {
    if (chainPending("localizeHandlesBegin"))
      return false;
    if (size_left == 0 || !cloud_in || cloud_in->size() == 0)
    {
      std::cout << "Input cloud is empty!\n";
      std::cout << size_left << std::endl;
      return false;
    }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    if (!search_->localizeBegin(cloud_in, size_left, workspace_, 0.003, indices, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pending_cloud_ = cloud_in;
    return true;
  }

  /** agh_localize_stage through the adapter: the next capture up, beside the chain in flight */
  bool stageNextCloud(const PointCloud::Ptr& next)
  {
    if (!next || next->size() == 0)
      return false;
    ensureSearch();
    return search_->localizeStage(next);
  }

  std::vector<Handle> localizeHandlesEnd(std::vector<GraspHypothesis>* antipodal_hands = nullptr)
  {
    std::vector<Handle> handle_list;
    if (antipodal_hands)
      antipodal_hands->clear();
    if (!pending_cloud_ && !pending_depth_)
      return handle_list;
    PointCloud::Ptr cloud_in = pending_cloud_;  // (none for a chain begun from depth images)
    pending_cloud_ = PointCloud::Ptr();
    pending_depth_ = false;
    std::vector<agh_hypothesis> hands;
    std::vector<agh_handle> handles;
    std::vector<std::int32_t> idx;
    if (!search_->localizeEnd(hands, handles, idx))
      return handle_list;
    return toHandles(cloud_in, hands, handles, idx, antipodal_hands);
  }

  /** Additional: localizeHandles straight from the sensor's depth images (agh_localize_depth): one or two images, image k is
   *  camera k, an image without a pose takes the k-th transform of setCameraTransforms (whose translations are the camera
   *  origins of the search either way).  No cloud is built on the host; otherwise as localizeHandles. */
  std::vector<Handle> localizeHandlesDepth(const std::vector<DepthImage>& images, const std::vector<int>& indices,
    const std::string& svm_filename, int min_inliers, double min_length, std::vector<GraspHypothesis>* antipodal_hands = nullptr)
  {
    if (antipodal_hands)
      antipodal_hands->clear();
    if (!localizeHandlesDepthBegin(images, indices, svm_filename, min_inliers, min_length))
      return std::vector<Handle>();
    return localizeHandlesEnd(antipodal_hands);
  }

  /** ... and as two calls, for a node that holds the NEXT pair of images while this one is searched:
   *      loc.localizeHandlesDepthBegin(images_k, indices, svm, min_inliers, 0.005);   // queued, not waited for
   *      loc.stageNextDepth(images_k1);                                               // their upload runs under capture k's kernels
   *      handles = loc.localizeHandlesEnd(&antipodal_hands);                          // the one synchronisation
   *      loc.localizeHandlesDepthBegin(images_k1, ...);                               // finds capture k + 1 on the device
   *  The pixel buffers must stay alive and unchanged until the localizeHandlesEnd of their chain has returned. */
  bool localizeHandlesDepthBegin(const std::vector<DepthImage>& images, const std::vector<int>& indices,
    const std::string& svm_filename, int min_inliers, double min_length)
  {
    if (chainPending("localizeHandlesDepthBegin"))
      return false;
    if (images.empty())
    {
      std::cout << "Input cloud is empty!\n";
      return false;
    }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    if (!search_->localizeDepthBegin(images, workspace_, 0.003, indices, svm_filename, min_inliers, min_length, filters_boundaries_))
      return false;
    pending_depth_ = true;
    return true;
  }

  /** Additional: localizeHandles with the samples drawn UNDER A MASK ("find grasps on this object"): `mask` holds one byte per
   *  point of cloud_in, as a detector or segmenter labels the capture; num_samples samples are drawn among the voxels that hold a
   *  masked point, and the whole cloud stays in the search for the hand's collision tests.  Otherwise as localizeHandles. */
  std::vector<Handle> localizeHandlesMasked(const PointCloud::Ptr& cloud_in, int size_left, const std::vector<std::uint8_t>& mask,
    const std::string& svm_filename, int min_inliers, double min_length, std::vector<GraspHypothesis>* antipodal_hands = nullptr)
  {
    if (antipodal_hands)
      antipodal_hands->clear();
    if (!localizeHandlesMaskedBegin(cloud_in, size_left, mask, svm_filename, min_inliers, min_length))
      return std::vector<Handle>();
    return localizeHandlesEnd(antipodal_hands);
  }

  /** ... as Begin + localizeHandlesEnd.  A Begin while a chain is pending returns false and leaves that chain as it was. */
  bool localizeHandlesMaskedBegin(const PointCloud::Ptr& cloud_in, int size_left, const std::vector<std::uint8_t>& mask,
    const std::string& svm_filename, int min_inliers, double min_length)
  {
    if (chainPending("localizeHandlesMaskedBegin"))
      return false;
    if (size_left == 0 || !cloud_in || cloud_in->size() == 0)
    {
      std::cout << "Input cloud is empty!\n";
      std::cout << size_left << std::endl;
      return false;
    }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    if (!search_->localizeMaskedBegin(cloud_in, size_left, mask, workspace_, 0.003, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pending_cloud_ = cloud_in;
    return true;
  }

  /** ... and straight from depth images with one mask per image (agh_localize_depth_masked); a mask without data makes no
   *  pixel of its image eligible.  Otherwise as localizeHandlesDepth. */
  std::vector<Handle> localizeHandlesDepthMasked(const std::vector<DepthImage>& images, const std::vector<SampleMask>& masks,
    const std::string& svm_filename, int min_inliers, double min_length, std::vector<GraspHypothesis>* antipodal_hands = nullptr)
  {
    if (antipodal_hands)
      antipodal_hands->clear();
    if (!localizeHandlesDepthMaskedBegin(images, masks, svm_filename, min_inliers, min_length))
      return std::vector<Handle>();
    return localizeHandlesEnd(antipodal_hands);
  }

  bool localizeHandlesDepthMaskedBegin(const std::vector<DepthImage>& images, const std::vector<SampleMask>& masks,
    const std::string& svm_filename, int min_inliers, double min_length)
  {
    if (chainPending("localizeHandlesDepthMaskedBegin"))
      return false;
    if (images.empty())
    {
      std::cout << "Input cloud is empty!\n";
      return false;
    }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    if (!search_->localizeDepthMaskedBegin(images, masks, workspace_, 0.003, svm_filename, min_inliers, min_length, filters_boundaries_))
      return false;
    pending_depth_ = true;
    return true;
  }

  /** Additional: localizeHandles for EVERY OBJECT of a label array in one call ("grasps on each of these objects", bin picking):
   *  `labels` holds one byte per point of cloud_in, as an instance segmenter labels the capture (0 = no object, j + 1 = object j
   *  of n_objects, 1 .. 64); num_samples samples are drawn per object among the voxels that hold one of its points.  The capture
   *  is preprocessed and searched once, on the whole cloud; the handle search runs per object.  Returns the handles per object
   *  (and the kept hands per object): object j's are those of localizeHandlesMasked with the mask labels == j + 1.  An error
   *  returns n_objects empty lists. */
  std::vector<std::vector<Handle> > localizeHandlesLabeled(const PointCloud::Ptr& cloud_in, int size_left,
    const std::vector<std::uint8_t>& labels, int n_objects, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object = nullptr)
  {
    const std::size_t K = n_objects >= 1 && n_objects <= 64 ? (std::size_t) n_objects : 0;
    std::vector<std::vector<Handle> > out = noHandles(K, antipodal_hands_per_object);
    if (chainPending("localizeHandlesLabeled"))
      return out;
    if (size_left == 0 || !cloud_in || cloud_in->size() == 0)
    {
      std::cout << "Input cloud is empty!\n";
      std::cout << size_left << std::endl;
      return out;
    }
    if (!detail::svmFileExists(svm_filename))
      return out;
    ensureSearch();
    std::vector<std::vector<agh_hypothesis> > hands;
    std::vector<std::vector<agh_handle> > handles;
    std::vector<std::vector<std::int32_t> > idx;
    if (!search_->localizeLabeled(cloud_in, size_left, labels, n_objects, workspace_, 0.003, svm_filename, min_inliers, min_length,
          hands, handles, idx, filters_boundaries_))
      return out;
    return labeledHandles(cloud_in, hands, handles, idx, antipodal_hands_per_object);
  }

  /** ... and straight from depth images with one label image per depth image (agh_localize_depth_labeled); a label image
   *  without data puts no pixel of its image into an object. */
  std::vector<std::vector<Handle> > localizeHandlesDepthLabeled(const std::vector<DepthImage>& images,
    const std::vector<LabelImage>& labels, int n_objects, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object = nullptr)
  {
    const std::size_t K = n_objects >= 1 && n_objects <= 64 ? (std::size_t) n_objects : 0;
    std::vector<std::vector<Handle> > out = noHandles(K, antipodal_hands_per_object);
    if (chainPending("localizeHandlesDepthLabeled"))
      return out;
    if (images.empty())
    {
      std::cout << "Input cloud is empty!\n";
      return out;
    }
    if (!detail::svmFileExists(svm_filename))
      return out;
    ensureSearch();
    std::vector<std::vector<agh_hypothesis> > hands;
    std::vector<std::vector<agh_handle> > handles;
    std::vector<std::vector<std::int32_t> > idx;
    if (!search_->localizeDepthLabeled(images, labels, n_objects, workspace_, 0.003, svm_filename, min_inliers, min_length, hands,
          handles, idx, filters_boundaries_))
      return out;
    return labeledHandles(PointCloud::Ptr(), hands, handles, idx, antipodal_hands_per_object);
  }

  /** The eligible voxels of every object of the last labelled call (agh_get_label_counts); empty if the last chain collected was
   *  not labelled, if there was none, or while a chain is pending. */
  std::vector<std::int64_t> getLabelCounts()
  {
    return search_ ? search_->labelCounts() : std::vector<std::int64_t>();
  }

  /** Additional: localizeHandles for every object ON A TABLE, without a segmenter (agh_localize_clustered): `plane` = (a, b, c, d),
   *  four entries, is the support plane the cell knows from calibration, (a, b, c) a unit vector pointing from the table towards the objects.
   *  The objects are the connected components of the voxels that stand above it (setClusterParams: the height band, the
   *  tolerance, the smallest object and the number of lists), found on the device inside the one call; nothing is removed from
   *  the cloud, so the hand search still sees the table.  Returns the handles per object, largest object first (and the kept hands
   *  per object), shaped like localizeHandlesLabeled's: max_objects lists, empty ones behind the objects found.  An error returns
   *  max_objects empty lists. */
  std::vector<std::vector<Handle> > localizeHandlesClustered(const PointCloud::Ptr& cloud_in, int size_left, const VectorXd& plane,
    const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object = nullptr)
  {
    return clusteredHandles("localizeHandlesClustered", cloud_in, size_left, clusterParams(plane), nullptr, svm_filename, min_inliers,
      min_length, antipodal_hands_per_object);
  }

  /** ... WITHOUT A CALIBRATED PLANE (agh_localize_clustered_fit): the dominant plane of the voxelised cloud is found on the device
   *  inside the call (setPlaneFitParams), oriented towards camera 0, and used as the support plane; fittedPlane() reports it.  No
   *  plane found: max_objects empty lists, as for an empty table. */
  std::vector<std::vector<Handle> > localizeHandlesClusteredFit(const PointCloud::Ptr& cloud_in, int size_left,
    const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object = nullptr)
  {
    return clusteredHandles("localizeHandlesClusteredFit", cloud_in, size_left, cluster_, &plane_fit_, svm_filename, min_inliers,
      min_length, antipodal_hands_per_object);
  }

  // the body of the two: fp == nullptr takes cp's plane
  std::vector<std::vector<Handle> > clusteredHandles(const char* fn, const PointCloud::Ptr& cloud_in, int size_left,
    const agh_cluster_params& cp, const agh_plane_fit_params* fp, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object)
  {
    const std::size_t K = cp.max_objects >= 1 && cp.max_objects <= 64 ? (std::size_t) cp.max_objects : 0;
    std::vector<std::vector<Handle> > out = noHandles(K, antipodal_hands_per_object);
    if (chainPending(fn))
      return out;
    if (size_left == 0 || !cloud_in || cloud_in->size() == 0)
    {
      std::cout << "Input cloud is empty!\n";
      std::cout << size_left << std::endl;
      return out;
    }
    if (!detail::svmFileExists(svm_filename))
      return out;
    ensureSearch();
    std::vector<std::vector<agh_hypothesis> > hands;
    std::vector<std::vector<agh_handle> > handles;
    std::vector<std::vector<std::int32_t> > idx;
    if (!search_->localizeClustered(cloud_in, size_left, cp, workspace_, 0.003, svm_filename, min_inliers, min_length, hands, handles,
          idx, filters_boundaries_, fp))
      return out;
    return labeledHandles(cloud_in, hands, handles, idx, antipodal_hands_per_object);
  }

  /** ... and straight from depth images (agh_localize_depth_clustered) */
  std::vector<std::vector<Handle> > localizeHandlesDepthClustered(const std::vector<DepthImage>& images, const VectorXd& plane,
    const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object = nullptr)
  {
    return depthClusteredHandles("localizeHandlesDepthClustered", images, clusterParams(plane), nullptr, svm_filename, min_inliers,
      min_length, antipodal_hands_per_object);
  }

  /** ... and localizeHandlesClusteredFit straight from depth images (agh_localize_depth_clustered_fit) */
  std::vector<std::vector<Handle> > localizeHandlesDepthClusteredFit(const std::vector<DepthImage>& images,
    const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object = nullptr)
  {
    return depthClusteredHandles("localizeHandlesDepthClusteredFit", images, cluster_, &plane_fit_, svm_filename, min_inliers,
      min_length, antipodal_hands_per_object);
  }

  std::vector<std::vector<Handle> > depthClusteredHandles(const char* fn, const std::vector<DepthImage>& images,
    const agh_cluster_params& cp, const agh_plane_fit_params* fp, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object)
  {
    const std::size_t K = cp.max_objects >= 1 && cp.max_objects <= 64 ? (std::size_t) cp.max_objects : 0;
    std::vector<std::vector<Handle> > out = noHandles(K, antipodal_hands_per_object);
    if (chainPending(fn))
      return out;
    if (images.empty())
    {
      std::cout << "Input cloud is empty!\n";
      return out;
    }
    if (!detail::svmFileExists(svm_filename))
      return out;
    ensureSearch();
    std::vector<std::vector<agh_hypothesis> > hands;
    std::vector<std::vector<agh_handle> > handles;
    std::vector<std::vector<std::int32_t> > idx;
    if (!search_->localizeDepthClustered(images, cp, workspace_, 0.003, svm_filename, min_inliers, min_length, hands, handles, idx,
          filters_boundaries_, fp))
      return out;
    return labeledHandles(PointCloud::Ptr(), hands, handles, idx, antipodal_hands_per_object);
  }

  // the call's agh_cluster_params: what setClusterParams holds, with this plane
  agh_cluster_params clusterParams(const VectorXd& plane) const
  {
    agh_cluster_params cp = cluster_;
    for (int k = 0; k < 4; k++)
      cp.plane[k] = plane(k);
    return cp;
  }

  /** The height band above the plane, the adjacency tolerance, the smallest object in voxels and the number of lists of the
   *  clustered calls (agh_cluster_params; the defaults are agh_default_cluster_params': 0.01 / 0.5, 0.01, 50, 16). */
  void setClusterParams(double min_height, double max_height, double tolerance, int min_voxels, int max_objects)
  {
    cluster_.min_height = min_height;
    cluster_.max_height = max_height;
    cluster_.tolerance = tolerance;
    cluster_.min_voxels = min_voxels;
    cluster_.max_objects = max_objects;
  }

  /** The plane finder of the fitted calls (agh_plane_fit_params; the defaults are agh_default_plane_fit_params': 128 candidates,
   *  1 cm, 3 inliers, refit on, seed 1). */
  void setPlaneFitParams(int n_candidates, double distance_threshold, int min_inliers = 3, bool refine = true, std::uint64_t seed = 1)
  {
    plane_fit_.n_candidates = n_candidates;
    plane_fit_.distance_threshold = distance_threshold;
    plane_fit_.min_inliers = min_inliers;
    plane_fit_.refine = refine ? 1 : 0;
    plane_fit_.seed = seed;
  }

  /** Additional: the depth filter of the calls that take depth images (agh_set_depth_filter; agh_default_depth_filter_params
   *  fills a record: 3 x 3 window, 3 supporters, 1 cm + 1 % of the depth, any range).  With a filter set the deprojection rejects
   *  flying pixels, speckles and readings outside [z_min, z_max] on the device; the points forms are not affected.  Sticky until
   *  clearDepthFilter, also across the setters that re-create the search.  Refused while a chain is pending.
   *  @return false (after printing) on error; the filter held before stays in force */
  bool setDepthFilter(const agh_depth_filter_params& fp)
  {
    if (chainPending("setDepthFilter"))
      return false;
    ensureSearch();
    if (!search_->setDepthFilter(fp))
      return false;
    depth_filter_ = fp;
    depth_filter_set_ = true;
    return true;
  }
  bool clearDepthFilter()
  {
    if (chainPending("clearDepthFilter") || (search_ && !search_->clearDepthFilter()))
      return false;
    depth_filter_set_ = false;
    return true;
  }
  /** the filter held; false: none */
  bool depthFilter(agh_depth_filter_params& out) const
  {
    if (depth_filter_set_)
      out = depth_filter_;
    return depth_filter_set_;
  }
  /** Additional: the voxel filter of every call that voxelises a capture (agh_set_voxel_filter; agh_default_voxel_filter_params
   *  fills a record: radius 2 voxels, 4 neighbours).  With a filter set the voxeliser prunes, on the device, the voxels with fewer
   *  occupied neighbours of their own camera -- stray returns in free space --, for points and depth images alike.  Sticky until
   *  clearVoxelFilter, also across the setters that re-create the search.  Refused while a chain is pending.
   *  @return false (after printing) on error; the filter held before stays in force */
  bool setVoxelFilter(const agh_voxel_filter_params& fp)
  {
    if (chainPending("setVoxelFilter"))
      return false;
    ensureSearch();
    if (!search_->setVoxelFilter(fp))
      return false;
    voxel_filter_ = fp;
    voxel_filter_set_ = true;
    return true;
  }
  bool clearVoxelFilter()
  {
    if (chainPending("clearVoxelFilter") || (search_ && !search_->clearVoxelFilter()))
      return false;
    voxel_filter_set_ = false;
    return true;
  }
  /** the filter held; false: none */
  bool voxelFilter(agh_voxel_filter_params& out) const
  {
    if (voxel_filter_set_)
      out = voxel_filter_;
    return voxel_filter_set_;
  }
  /** What the filter did in the last call that voxelised (agh_get_voxel_filter_counts): one record per capture; empty if that
   *  call ran without a filter, if there was none, or while a chain is pending. */
  std::vector<agh_voxel_filter_counts> voxelFilterCounts()
  {
    return search_ ? search_->voxelFilterCounts() : std::vector<agh_voxel_filter_counts>();
  }

  /** Additional: the hand filter of every localizeHandles* form (agh_set_hand_filter; agh_default_hand_filter_params fills a
   *  record with every criterion off).  With a filter set the chain drops, on the device and ahead of the classifier, the hands
   *  outside an approach cone (approach_on), outside the gripper's stroke (width_on), or with fingers in space no depth image saw
   *  (view_on: the depth forms only -- a points form then fails, it does not silently skip the test).  The handles are those of
   *  the surviving hands.  Sticky until clearHandFilter, also across the setters that re-create the search.  Refused while a
   *  chain is pending.
   *  @return false (after printing) on error; the filter held before stays in force */
  bool setHandFilter(const agh_hand_filter_params& fp)
  {
    if (chainPending("setHandFilter"))
      return false;
    ensureSearch();
    if (!search_->setHandFilter(fp))
      return false;
    hand_filter_ = fp;
    hand_filter_set_ = true;
    return true;
  }
  bool clearHandFilter()
  {
    if (chainPending("clearHandFilter") || (search_ && !search_->clearHandFilter()))
      return false;
    hand_filter_set_ = false;
    return true;
  }
  /** the filter held; false: none */
  bool handFilter(agh_hand_filter_params& out) const
  {
    if (hand_filter_set_)
      out = hand_filter_;
    return hand_filter_set_;
  }
  /** What the filter did in the last localizeHandles* call (agh_get_hand_filter_counts): one record per list of its results;
   *  empty if that call ran without a filter, if there was none, or while a chain is pending. */
  std::vector<agh_hand_filter_counts> handFilterCounts()
  {
    return search_ ? search_->handFilterCounts() : std::vector<agh_hand_filter_counts>();
  }

  /** Additional: the hand clearance of every localizeHandles* form (agh_set_hand_clearance; agh_default_hand_clearance_params
   *  fills a record with a corridor of 12 cm x +- 5 cm x +- 4 cm that must be empty).  With one set the chain drops, on the device,
   *  behind the hand filter and ahead of the classifier, the hands whose approach corridor -- the oriented box the gripper's body
   *  sweeps behind the palm on its way in -- holds more than max_points points of the capture's own voxelised cloud: the hands
   *  a real gripper would drive into the table or a neighbouring object.  The handles are those of the surviving hands.  Sticky
   *  until clearHandClearance, also across the setters that re-create the search.  Refused while a chain is pending.
   *  @return false (after printing) on error; the setting held before stays in force */
  bool setHandClearance(const agh_hand_clearance_params& cp)
  {
    if (chainPending("setHandClearance"))
      return false;
    ensureSearch();
    if (!search_->setHandClearance(cp))
      return false;
    hand_clearance_ = cp;
    hand_clearance_set_ = true;
    return true;
  }
  bool clearHandClearance()
  {
    if (chainPending("clearHandClearance") || (search_ && !search_->clearHandClearance()))
      return false;
    hand_clearance_set_ = false;
    return true;
  }
  /** the clearance held; false: none */
  bool handClearance(agh_hand_clearance_params& out) const
  {
    if (hand_clearance_set_)
      out = hand_clearance_;
    return hand_clearance_set_;
  }
  /** What the clearance did in the last localizeHandles* call (agh_get_hand_clearance_counts): one record per list of its
   *  results; empty if that call ran without one, if there was none, or while a chain is pending. */
  std::vector<agh_hand_clearance_counts> handClearanceCounts()
  {
    return search_ ? search_->handClearanceCounts() : std::vector<agh_hand_clearance_counts>();
  }

  /** Additional: the handle ranking of every localizeHandles* form (agh_set_handle_ranking; agh_default_handle_ranking_params
   *  fills a record that scores a handle by its support and its classifier margin).  With one set the chain returns each list's
   *  handles in rank order -- best first, ties in the order of discovery, the handles below min_score left out, at most
   *  max_handles per list -- sorted on the device behind the handle search; the inlier lists and the hands are untouched.  A call
   *  without a classifier (svm_filename empty) is refused while w_margin is not 0.  Sticky until clearHandleRanking, also across
   *  the setters that re-create the search.  Refused while a chain is pending.
   *  @return false (after printing) on error; the setting held before stays in force */
  bool setHandleRanking(const agh_handle_ranking_params& rp)
  {
    if (chainPending("setHandleRanking"))
      return false;
    ensureSearch();
    if (!search_->setHandleRanking(rp))
      return false;
    handle_ranking_ = rp;
    handle_ranking_set_ = true;
    return true;
  }
  bool clearHandleRanking()
  {
    if (chainPending("clearHandleRanking") || (search_ && !search_->clearHandleRanking()))
      return false;
    handle_ranking_set_ = false;
    return true;
  }
  /** the ranking held; false: none */
  bool handleRanking(agh_handle_ranking_params& out) const
  {
    if (handle_ranking_set_)
      out = handle_ranking_;
    return handle_ranking_set_;
  }
  /** The score records of the handles the last localizeHandles* call returned, in their order (agh_get_handle_scores): score, the
   *  seven terms, the handle's position in the unranked list and its best inlier; empty if that call ran without a ranking, if
   *  there was none, or while a chain is pending. */
  std::vector<agh_handle_score> handleScores()
  {
    return search_ ? search_->handleScores() : std::vector<agh_handle_score>();
  }
  /** per list of that call: handles found, left out by min_score, returned (agh_get_handle_ranking_counts) */
  std::vector<agh_handle_ranking_counts> handleRankingCounts()
  {
    return search_ ? search_->handleRankingCounts() : std::vector<agh_handle_ranking_counts>();
  }
  /** the classifier margins of the hands that call's handle search ran on (agh_get_hand_margins) */
  std::vector<double> handMargins()
  {
    return search_ ? search_->handMargins() : std::vector<double>();
  }

  /** What the filter did in the last depth call (agh_get_depth_filter_counts): one record per image, in capture order; empty if
   *  that call ran without a filter, if there was none, or while a chain is pending. */
  std::vector<agh_depth_filter_counts> depthFilterCounts()
  {
    return search_ ? search_->depthFilterCounts() : std::vector<agh_depth_filter_counts>();
  }

  /** Additional: a burst of depth frames of ONE fixed camera fused on the device ahead of the depth calls (agh_fuse_depth;
   *  agh_default_depth_fusion_params fills a record: 2 valid frames, 5 mm + 0.5 % of the depth): the lower median of a pixel's
   *  valid readings, the mean of the readings within the spread of it, and an invalid pixel where too few frames agree.  1 to 16
   *  frames into slot `slot` (0 .. 127); a frame without a pose takes camera `camera`'s transform of setCameraTransforms.
   *  fusedDepth then hands the image back for localizeHandlesDepth.  Refused while a chain is pending.
   *  @return false (after printing) on error; the slot's previous image is untouched */
  bool fuseDepth(const std::vector<DepthImage>& frames, const agh_depth_fusion_params& fp, int slot = 0, int camera = 0,
    agh_depth_image* fused_out = nullptr)
  {
    if (chainPending("fuseDepth"))
      return false;
    ensureSearch();
    return search_->fuseDepth(frames, fp, slot, camera, fused_out);
  }
  /** What the slot's last fuse did (agh_get_depth_fusion_counts); false if the slot was never fused or while a chain is pending */
  bool depthFusionCounts(int slot, agh_depth_fusion_counts& out)
  {
    return search_ && search_->depthFusionCounts(slot, out);
  }
  /** The slot's fused image in `pixels`, described by `image` (agh_get_fused_depth); keep `pixels` alive while `image` is used */
  bool fusedDepth(int slot, std::vector<std::uint8_t>& pixels, DepthImage& image)
  {
    return search_ && search_->fusedDepth(slot, pixels, image);
  }

  /** The plane the last fitted call used (agh_get_plane_fit): (a, b, c, d), the normal towards camera 0; zeros, and *found false,
   *  if it found none, if the last chain collected was not a fitted one, or while a chain is pending. */
  VectorXd fittedPlane(bool* found = nullptr)
  {
    agh_plane_fit_result r = agh_plane_fit_result();
    if (search_)
      search_->planeFit(r);
    VectorXd plane(4);
    for (int k = 0; k < 4; k++)
      plane(k) = r.plane[k];
    if (found)
      *found = r.found != 0;
    return plane;
  }

  /** The objects of the last clustered call (agh_get_cluster_info): their voxel counts, largest first, one entry per list; empty
   *  if the last chain collected was not clustered, if there was none, or while a chain is pending. */
  std::vector<std::int64_t> getClusterSizes()
  {
    agh_cluster_info info;
    std::vector<std::int64_t> m;
    std::vector<std::int32_t> ids;
    if (search_)
      search_->clusterInfo(info, m, ids);
    return m;
  }

  /** The seed of the samples a chain draws on the device (HandSearch::setSampleSeed; default: the clock, like pcl::RandomSample),
   *  and the list the last collected chain searched (HandSearch::getLastSampleIndices): together they make a masked call
   *  repeatable with explicit indices. */
  void setSampleSeed(std::uint64_t seed)
  {
    sample_seed_ = seed;
    sample_seed_set_ = true;
    if (search_)
      search_->setSampleSeed(seed);
  }
  std::vector<int> getLastSampleIndices() const
  {
    if (!search_)
      return std::vector<int>();
    return std::vector<int>(search_->getLastSampleIndices().begin(), search_->getLastSampleIndices().end());
  }

  /** The eligible voxels of the last masked chain localizeHandlesEnd collected (agh_get_sample_mask_count); -1 if that chain had
   *  no mask, if there was none, or while a chain is pending. */
  std::int64_t getSampleMaskCount()
  {
    return search_ ? search_->sampleMaskCount() : -1;
  }

  /** agh_localize_depth_stage through the adapter: the next capture's images up, beside the chain in flight */
  bool stageNextDepth(const std::vector<DepthImage>& next)
  {
    if (next.empty())
      return false;
    ensureSearch();
    return search_->localizeDepthStage(next);
  }

  /** Additional: localizeHandles over several captures in one call (localizeHandlesBatchBegin + localizeHandlesBatchEnd, one
   *  synchronisation): capture k is clouds[k] with sizes_left[k] and indices_per_cloud[k] (empty: drawn on the device, see
   *  HandSearch::localizeBatch), searched in (*workspaces)[k] -- or, without `workspaces`, in this object's workspace.  Per capture
   *  the same handles as localizeHandles on that capture and indices; (*antipodal_hands_per_cloud)[k] receives its kept hands. */
  std::vector<std::vector<Handle> > localizeHandlesBatch(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<int> >& indices_per_cloud, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_cloud = nullptr, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesBatch") ||
        !localizeHandlesBatchBegin(clouds, sizes_left, indices_per_cloud, svm_filename, min_inliers, min_length, workspaces))
      return noHandles(clouds.size(), antipodal_hands_per_cloud);
    return localizeHandlesBatchEnd(antipodal_hands_per_cloud);
  }

  /** Additional: localizeHandlesBatch as two calls, for a walk over a directory of captures, batch by batch:
   *      loc.localizeHandlesBatchBegin(batch_k, sizes_left_k, indices_k, svm, min_inliers, 0.005);  // queued, not waited for
   *      loc.stageNextBatch(batch_k1);                          // its uploads run under batch k's kernels
   *      handles = loc.localizeHandlesBatchEnd(&antipodal_hands_per_cloud);                         // the one synchronisation
   *      loc.localizeHandlesBatchBegin(batch_k1, ...);          // finds batch k + 1 on the device
   *  Same results as localizeHandlesBatch.  One chain of either kind may be pending: a Begin while one is returns false and leaves
   *  it as it was, and so does a Begin that fails for another reason.  The clouds must stay alive and unchanged until the
   *  localizeHandlesBatchEnd of their chain has returned (which then filters NaNs out of them in place). */
  bool localizeHandlesBatchBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<int> >& indices_per_cloud, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesBatchBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < clouds.size(); k++)
      if (!clouds[k] || clouds[k]->size() == 0 || k >= sizes_left.size() || sizes_left[k] == 0)
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(clouds.size(), workspace_);
    if (!search_->localizeBatchBegin(clouds, sizes_left, ws, 0.003, indices_per_cloud, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pending_batch_ = clouds;
    return true;
  }

  /** agh_localize_batch_stage through the adapter: the next batch up, beside the chain in flight */
  bool stageNextBatch(const std::vector<PointCloud::Ptr>& next)
  {
    for (std::size_t k = 0; k < next.size(); k++)
      if (!next[k] || next[k]->size() == 0)
        return false;
    if (next.empty())
      return false;
    ensureSearch();
    return search_->localizeBatchStage(next);
  }

  std::vector<std::vector<Handle> > localizeHandlesBatchEnd(std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_cloud = nullptr)
  {
    const std::vector<PointCloud::Ptr> clouds = pending_batch_;
    pending_batch_.clear();
    std::vector<std::vector<Handle> > out = noHandles(clouds.size(), antipodal_hands_per_cloud);
    std::vector<std::vector<agh_hypothesis> > hands;
    std::vector<std::vector<agh_handle> > handles;
    std::vector<std::vector<std::int32_t> > idx;
    if (clouds.empty() || !search_->localizeBatchEnd(hands, handles, idx))
      return out;
    for (std::size_t k = 0; k < clouds.size(); k++)
      out[k] = toHandles(clouds[k], hands[k], handles[k], idx[k], antipodal_hands_per_cloud ? &(*antipodal_hands_per_cloud)[k] : nullptr);
    return out;
  }

  /** Additional: the same for captures of SEVERAL rigs -- capture k was taken with the camera transforms cams_left[k] /
   *  cams_right[k] (translations only, as setCameraTransforms).  Sets the per-cloud origin table (agh_set_cloud_cam_origins),
   *  runs the batch and clears the table: per capture the same handles as localizeHandles of a Localization set up with that
   *  capture's transforms.  Hand geometry stays this object's.  The table is cleared afterwards in any case: one set before
   *  through HandSearch::setCloudCamOrigins is replaced by this call's and is NOT restored. */
  std::vector<std::vector<Handle> > localizeHandlesBatch(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<int> >& indices_per_cloud, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<Matrix4d>& cams_left, const std::vector<Matrix4d>& cams_right,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_cloud = nullptr, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (cams_left.size() != clouds.size() || cams_right.size() != clouds.size())
    {
      std::cout << " Error: localizeHandlesBatch needs one left and one right camera transform per cloud\n";
      return noHandles(clouds.size(), antipodal_hands_per_cloud);
    }
    if (chainPending("localizeHandlesBatch"))  // (a chain in flight keeps the table it has)
      return noHandles(clouds.size(), antipodal_hands_per_cloud);
    ensureSearch();
    if (!search_->setCloudCamOrigins(cams_left, cams_right))
      return noHandles(clouds.size(), antipodal_hands_per_cloud);
    const std::vector<std::vector<Handle> > out = localizeHandlesBatch(clouds, sizes_left, indices_per_cloud, svm_filename,
      min_inliers, min_length, antipodal_hands_per_cloud, workspaces);
    search_->clearCloudCamOrigins();
    return out;
  }

  /** Additional: localizeHandlesBatch straight from depth images (agh_localize_depth_batch): capture k is captures[k], one or
   *  two images as localizeHandlesDepth takes them, with indices_per_capture[k], searched in (*workspaces)[k] or this object's
   *  workspace.  No clouds are built on the host.  Per capture the same handles as localizeHandlesDepth on that capture. */
  std::vector<std::vector<Handle> > localizeHandlesDepthBatch(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<int> >& indices_per_capture, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_capture = nullptr, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatch") ||
        !localizeHandlesDepthBatchBegin(captures, indices_per_capture, svm_filename, min_inliers, min_length, workspaces))
      return noHandles(captures.size(), antipodal_hands_per_capture);
    return localizeHandlesBatchEnd(antipodal_hands_per_capture);
  }

  /** ... and as two calls: the chain queued here is collected by localizeHandlesBatchEnd (it has no host clouds).  The pixel
   *  buffers must stay alive and unchanged until then.  A Begin while a chain of any kind is pending returns false and leaves it
   *  as it was, and so does a Begin that fails for another reason. */
  bool localizeHandlesDepthBatchBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<int> >& indices_per_capture, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < captures.size(); k++)
      if (captures[k].empty())
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(captures.size(), workspace_);
    if (!search_->localizeDepthBatchBegin(captures, ws, 0.003, indices_per_capture, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pending_batch_.assign(captures.size(), PointCloud::Ptr());  // (one entry per capture, none with a host cloud)
    return true;
  }

  /** Additional: the same for captures of SEVERAL rigs, as the points batch has it: capture k was taken with the camera
   *  transforms cams_left[k] / cams_right[k], whose translations become row k of the per-cloud origin table for this call (the
   *  images' poses do not set origins).  The table is cleared afterwards in any case. */
  std::vector<std::vector<Handle> > localizeHandlesDepthBatch(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<int> >& indices_per_capture, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<Matrix4d>& cams_left, const std::vector<Matrix4d>& cams_right,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_capture = nullptr, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (cams_left.size() != captures.size() || cams_right.size() != captures.size())
    {
      std::cout << " Error: localizeHandlesDepthBatch needs one left and one right camera transform per capture\n";
      return noHandles(captures.size(), antipodal_hands_per_capture);
    }
    if (chainPending("localizeHandlesDepthBatch"))  // (a chain in flight keeps the table it has)
      return noHandles(captures.size(), antipodal_hands_per_capture);
    ensureSearch();
    if (!search_->setCloudCamOrigins(cams_left, cams_right))
      return noHandles(captures.size(), antipodal_hands_per_capture);
    const std::vector<std::vector<Handle> > out = localizeHandlesDepthBatch(captures, indices_per_capture, svm_filename, min_inliers,
      min_length, antipodal_hands_per_capture, workspaces);
    search_->clearCloudCamOrigins();
    return out;
  }

  /** Additional: localizeHandlesBatch with every capture's samples drawn UNDER ITS OWN MASK (agh_localize_batch_masked): a cell
   *  with one detector per sensor pair hands over masks[k], one byte per point of clouds[k]; num_samples samples are drawn per
   *  capture among the voxels that hold one of its masked points, and the whole capture stays in the search.  Per capture the
   *  same handles as localizeHandlesMasked on that capture and mask (seeded with the sample seed + k). */
  std::vector<std::vector<Handle> > localizeHandlesBatchMasked(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<std::uint8_t> >& masks, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_cloud = nullptr, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesBatchMasked") ||
        !localizeHandlesBatchMaskedBegin(clouds, sizes_left, masks, svm_filename, min_inliers, min_length, workspaces))
      return noHandles(clouds.size(), antipodal_hands_per_cloud);
    return localizeHandlesBatchEnd(antipodal_hands_per_cloud);
  }

  /** ... as two calls: the chain queued here is collected by localizeHandlesBatchEnd.  A Begin while a chain of any kind is
   *  pending returns false and leaves it as it was, and so does a Begin that fails for another reason.  The masks are copied by
   *  the call; the clouds must stay alive and unchanged until localizeHandlesBatchEnd has returned. */
  bool localizeHandlesBatchMaskedBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<std::uint8_t> >& masks, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesBatchMaskedBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < clouds.size(); k++)
      if (!clouds[k] || clouds[k]->size() == 0 || k >= sizes_left.size() || sizes_left[k] == 0)
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(clouds.size(), workspace_);
    if (!search_->localizeBatchMaskedBegin(clouds, sizes_left, masks, ws, 0.003, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pending_batch_ = clouds;
    return true;
  }

  /** ... and straight from depth images with one mask per image (agh_localize_depth_batch_masked): masks[k][j] belongs to
   *  captures[k][j]; a mask without data makes no pixel of its image eligible.  Per capture the same handles as
   *  localizeHandlesDepthMasked on that capture and its masks. */
  std::vector<std::vector<Handle> > localizeHandlesDepthBatchMasked(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<SampleMask> >& masks, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_capture = nullptr, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchMasked") ||
        !localizeHandlesDepthBatchMaskedBegin(captures, masks, svm_filename, min_inliers, min_length, workspaces))
      return noHandles(captures.size(), antipodal_hands_per_capture);
    return localizeHandlesBatchEnd(antipodal_hands_per_capture);
  }

  bool localizeHandlesDepthBatchMaskedBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<SampleMask> >& masks, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchMaskedBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < captures.size(); k++)
      if (captures[k].empty())
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(captures.size(), workspace_);
    if (!search_->localizeDepthBatchMaskedBegin(captures, masks, ws, 0.003, svm_filename, min_inliers, min_length, filters_boundaries_))
      return false;
    pending_batch_.assign(captures.size(), PointCloud::Ptr());  // (one entry per capture, none with a host cloud)
    return true;
  }

  /** The eligible voxels of every capture of the last masked batch localizeHandlesBatchEnd collected
   *  (agh_get_batch_mask_counts); empty if the last chain collected was no masked batch, if there was none, or while a chain is
   *  pending. */
  std::vector<std::int64_t> getBatchMaskCounts()
  {
    return search_ ? search_->batchMaskCounts() : std::vector<std::int64_t>();
  }

  /** Additional: localizeHandlesBatch with one sample list PER OBJECT of every capture's label array
   *  (agh_localize_batch_labeled): a cell with one instance segmenter per sensor pair hands over labels[k], one byte per point
   *  of clouds[k] (0 = no object, j + 1 = object j of n_objects[k]; at most 64 objects in all); num_samples samples are drawn
   *  per object.  Returns the handles per capture and object -- out[k][j] are those of localizeHandlesLabeled on capture k alone
   *  (seeded with the sample seed + k) -- and likewise the kept hands.  An error returns empty lists, per capture and object
   *  where the object counts say how many. */
  std::vector<std::vector<std::vector<Handle> > > localizeHandlesBatchLabeled(const std::vector<PointCloud::Ptr>& clouds,
    const std::vector<int>& sizes_left, const std::vector<std::vector<std::uint8_t> >& labels, const std::vector<int>& n_objects,
    const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object = nullptr,
    const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesBatchLabeled") ||
        !localizeHandlesBatchLabeledBegin(clouds, sizes_left, labels, n_objects, svm_filename, min_inliers, min_length, workspaces))
      return noLabeledHandles(n_objects, antipodal_hands_per_object);
    return localizeHandlesBatchLabeledEnd(antipodal_hands_per_object);
  }

  /** ... as two calls: the chain queued here is collected by localizeHandlesBatchLabeledEnd (or by localizeHandlesBatchEnd, which
   *  returns one entry per LIST: capture after capture, object after object).  A Begin while a chain of any kind is pending
   *  returns false and leaves it as it was, and so does a Begin that fails for another reason.  The labels are copied by the
   *  call; the clouds must stay alive and unchanged until the End has returned. */
  bool localizeHandlesBatchLabeledBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<std::uint8_t> >& labels, const std::vector<int>& n_objects, const std::string& svm_filename,
    int min_inliers, double min_length, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesBatchLabeledBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < clouds.size(); k++)
      if (!clouds[k] || clouds[k]->size() == 0 || k >= sizes_left.size() || sizes_left[k] == 0)
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(clouds.size(), workspace_);
    if (!search_->localizeBatchLabeledBegin(clouds, sizes_left, labels, n_objects, ws, 0.003, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pendingLists(clouds, n_objects);
    return true;
  }

  /** ... and straight from depth images with one label image per image (agh_localize_depth_batch_labeled): labels[k][j] belongs
   *  to captures[k][j]; a label image without data puts no pixel of its image into an object.  out[k][j] are the handles of
   *  localizeHandlesDepthLabeled on capture k alone. */
  std::vector<std::vector<std::vector<Handle> > > localizeHandlesDepthBatchLabeled(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<LabelImage> >& labels, const std::vector<int>& n_objects, const std::string& svm_filename,
    int min_inliers, double min_length, std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object = nullptr,
    const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchLabeled") ||
        !localizeHandlesDepthBatchLabeledBegin(captures, labels, n_objects, svm_filename, min_inliers, min_length, workspaces))
      return noLabeledHandles(n_objects, antipodal_hands_per_object);
    return localizeHandlesBatchLabeledEnd(antipodal_hands_per_object);
  }

  bool localizeHandlesDepthBatchLabeledBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<LabelImage> >& labels, const std::vector<int>& n_objects, const std::string& svm_filename,
    int min_inliers, double min_length, const std::vector<VectorXd>* workspaces = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchLabeledBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < captures.size(); k++)
      if (captures[k].empty())
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(captures.size(), workspace_);
    if (!search_->localizeDepthBatchLabeledBegin(captures, labels, n_objects, ws, 0.003, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pendingLists(std::vector<PointCloud::Ptr>(captures.size()), n_objects);  // (no capture with a host cloud)
    return true;
  }

  /** Additional: localizeHandlesBatchLabeled WITHOUT A SEGMENTER on any rig (agh_localize_batch_clustered): planes[k] = (a, b, c, d)
   *  is capture k's own support plane -- rigs have their own.  Capture k's objects are the connected components of its voxels
   *  above planes[k]; the height band, tolerance, smallest object and number of lists are setClusterParams' for every capture,
   *  or cluster_params[k] (its plane is replaced by planes[k]) where that vector is given.  At most 64 lists in all.  Returns the
   *  handles per capture and object, largest object first -- out[k][j] are those of localizeHandlesClustered on capture k alone
   *  (seeded with the sample seed + k) -- and likewise the kept hands.  An error returns empty lists, per capture and object
   *  where the records say how many. */
  std::vector<std::vector<std::vector<Handle> > > localizeHandlesBatchClustered(const std::vector<PointCloud::Ptr>& clouds,
    const std::vector<int>& sizes_left, const std::vector<VectorXd>& planes, const std::string& svm_filename, int min_inliers,
    double min_length, std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object = nullptr,
    const std::vector<VectorXd>* workspaces = nullptr, const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesBatchClustered") ||
        !localizeHandlesBatchClusteredBegin(clouds, sizes_left, planes, svm_filename, min_inliers, min_length, workspaces, cluster_params))
      return noLabeledHandles(HandSearch::clusterObjects(batchClusterParams(planes, cluster_params)), antipodal_hands_per_object);
    return localizeHandlesBatchLabeledEnd(antipodal_hands_per_object);
  }

  /** ... as two calls: the chain queued here is collected by localizeHandlesBatchLabeledEnd.  A Begin while a chain of any kind
   *  is pending returns false and leaves it as it was, and so does a Begin that fails for another reason.  The clouds must stay
   *  alive and unchanged until the End has returned. */
  bool localizeHandlesBatchClusteredBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<VectorXd>& planes, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<VectorXd>* workspaces = nullptr, const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesBatchClusteredBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < clouds.size(); k++)
      if (!clouds[k] || clouds[k]->size() == 0 || k >= sizes_left.size() || sizes_left[k] == 0)
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!batchPlanesGiven("localizeHandlesBatchClusteredBegin", clouds.size(), planes, cluster_params) ||
        !detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(clouds.size(), workspace_);
    const std::vector<agh_cluster_params> cp = batchClusterParams(planes, cluster_params);
    if (!search_->localizeBatchClusteredBegin(clouds, sizes_left, cp, ws, 0.003, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pendingLists(clouds, HandSearch::clusterObjects(cp));
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_batch_clustered): out[k][j] are the handles of
   *  localizeHandlesDepthClustered on capture k alone. */
  std::vector<std::vector<std::vector<Handle> > > localizeHandlesDepthBatchClustered(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<VectorXd>& planes, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object = nullptr,
    const std::vector<VectorXd>* workspaces = nullptr, const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchClustered") ||
        !localizeHandlesDepthBatchClusteredBegin(captures, planes, svm_filename, min_inliers, min_length, workspaces, cluster_params))
      return noLabeledHandles(HandSearch::clusterObjects(batchClusterParams(planes, cluster_params)), antipodal_hands_per_object);
    return localizeHandlesBatchLabeledEnd(antipodal_hands_per_object);
  }

  bool localizeHandlesDepthBatchClusteredBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<VectorXd>& planes, const std::string& svm_filename, int min_inliers, double min_length,
    const std::vector<VectorXd>* workspaces = nullptr, const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchClusteredBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < captures.size(); k++)
      if (captures[k].empty())
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!batchPlanesGiven("localizeHandlesDepthBatchClusteredBegin", captures.size(), planes, cluster_params) ||
        !detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(captures.size(), workspace_);
    const std::vector<agh_cluster_params> cp = batchClusterParams(planes, cluster_params);
    if (!search_->localizeDepthBatchClusteredBegin(captures, cp, ws, 0.003, svm_filename, min_inliers, min_length, filters_boundaries_))
      return false;
    pendingLists(std::vector<PointCloud::Ptr>(captures.size()), HandSearch::clusterObjects(cp));  // (no capture with a host cloud)
    return true;
  }

  /** Additional: localizeHandlesBatchClustered WITHOUT A CALIBRATED PLANE on any rig (agh_localize_batch_clustered_fit): every
   *  capture's dominant plane is found on the device inside the one chain, on the capture's own voxels (setPlaneFitParams, the
   *  same record for every capture; the sample seed + k is NOT added to its seed), oriented towards camera 0 of the capture's
   *  rig, and used as its support plane; fittedPlanes() reports them.  The other cluster parameters are setClusterParams' for
   *  every capture, or cluster_params[k] (its plane is not read).  out[k][j] are the handles of localizeHandlesClusteredFit on
   *  capture k alone (seeded with the sample seed + k). */
  std::vector<std::vector<std::vector<Handle> > > localizeHandlesBatchClusteredFit(const std::vector<PointCloud::Ptr>& clouds,
    const std::vector<int>& sizes_left, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object = nullptr,
    const std::vector<VectorXd>* workspaces = nullptr, const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesBatchClusteredFit") ||
        !localizeHandlesBatchClusteredFitBegin(clouds, sizes_left, svm_filename, min_inliers, min_length, workspaces, cluster_params))
      return noLabeledHandles(HandSearch::clusterObjects(batchFitClusterParams(clouds.size(), cluster_params)), antipodal_hands_per_object);
    return localizeHandlesBatchLabeledEnd(antipodal_hands_per_object);
  }

  /** ... as two calls: the chain queued here is collected by localizeHandlesBatchLabeledEnd, as a clustered Begin's. */
  bool localizeHandlesBatchClusteredFitBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::string& svm_filename, int min_inliers, double min_length, const std::vector<VectorXd>* workspaces = nullptr,
    const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesBatchClusteredFitBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < clouds.size(); k++)
      if (!clouds[k] || clouds[k]->size() == 0 || k >= sizes_left.size() || sizes_left[k] == 0)
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!batchFitRecordsGiven("localizeHandlesBatchClusteredFitBegin", clouds.size(), cluster_params) || !detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(clouds.size(), workspace_);
    const std::vector<agh_cluster_params> cp = batchFitClusterParams(clouds.size(), cluster_params);
    const std::vector<agh_plane_fit_params> fp(clouds.size(), plane_fit_);
    if (!search_->localizeBatchClusteredFitBegin(clouds, sizes_left, fp, cp, ws, 0.003, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pendingLists(clouds, HandSearch::clusterObjects(cp));
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_batch_clustered_fit): out[k][j] are the handles of
   *  localizeHandlesDepthClusteredFit on capture k alone. */
  std::vector<std::vector<std::vector<Handle> > > localizeHandlesDepthBatchClusteredFit(const std::vector<std::vector<DepthImage> >& captures,
    const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object = nullptr,
    const std::vector<VectorXd>* workspaces = nullptr, const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchClusteredFit") ||
        !localizeHandlesDepthBatchClusteredFitBegin(captures, svm_filename, min_inliers, min_length, workspaces, cluster_params))
      return noLabeledHandles(HandSearch::clusterObjects(batchFitClusterParams(captures.size(), cluster_params)), antipodal_hands_per_object);
    return localizeHandlesBatchLabeledEnd(antipodal_hands_per_object);
  }

  bool localizeHandlesDepthBatchClusteredFitBegin(const std::vector<std::vector<DepthImage> >& captures, const std::string& svm_filename,
    int min_inliers, double min_length, const std::vector<VectorXd>* workspaces = nullptr,
    const std::vector<agh_cluster_params>* cluster_params = nullptr)
  {
    if (chainPending("localizeHandlesDepthBatchClusteredFitBegin", "its End"))
      return false;
    for (std::size_t k = 0; k < captures.size(); k++)
      if (captures[k].empty())
      {
        std::cout << "Input cloud is empty!\n";
        return false;
      }
    if (!batchFitRecordsGiven("localizeHandlesDepthBatchClusteredFitBegin", captures.size(), cluster_params) ||
        !detail::svmFileExists(svm_filename))
      return false;
    ensureSearch();
    const std::vector<VectorXd> ws = workspaces ? *workspaces : std::vector<VectorXd>(captures.size(), workspace_);
    const std::vector<agh_cluster_params> cp = batchFitClusterParams(captures.size(), cluster_params);
    const std::vector<agh_plane_fit_params> fp(captures.size(), plane_fit_);
    if (!search_->localizeDepthBatchClusteredFitBegin(captures, fp, cp, ws, 0.003, svm_filename, min_inliers, min_length,
          filters_boundaries_))
      return false;
    pendingLists(std::vector<PointCloud::Ptr>(captures.size()), HandSearch::clusterObjects(cp));  // (no capture with a host cloud)
    return true;
  }

  // the cluster records of a fitted batch: cluster_params[k], or what setClusterParams holds, for every capture (no plane is read)
  std::vector<agh_cluster_params> batchFitClusterParams(std::size_t n_captures, const std::vector<agh_cluster_params>* cluster_params) const
  {
    if (cluster_params)
      return cluster_params->size() == n_captures ? *cluster_params : std::vector<agh_cluster_params>();
    return std::vector<agh_cluster_params>(n_captures, cluster_);
  }
  bool batchFitRecordsGiven(const char* fn, std::size_t n_captures, const std::vector<agh_cluster_params>* cluster_params) const
  {
    if (!cluster_params || cluster_params->size() == n_captures)
      return true;
    std::cout << " Error: " << fn << " needs, where cluster records are given, one per capture\n";
    return false;
  }

  /** The planes of the last fitted batch collected (agh_get_batch_plane_fit): one (a, b, c, d) per capture, zeros for a capture
   *  without a plane, (*found)[k] saying which; empty if the last chain collected was no fitted batch, if there was none, or
   *  while a chain is pending. */
  std::vector<VectorXd> fittedPlanes(std::vector<bool>* found = nullptr)
  {
    std::vector<agh_plane_fit_result> r;
    if (search_)
      search_->batchPlaneFit(r);
    std::vector<VectorXd> planes(r.size(), VectorXd(4));
    if (found)
      found->assign(r.size(), false);
    for (std::size_t k = 0; k < r.size(); k++)
    {
      for (int q = 0; q < 4; q++)
        planes[k](q) = r[k].plane[q];
      if (found)
        (*found)[k] = r[k].found != 0;
    }
    return planes;
  }

  // the records of a clustered batch: cluster_params[k] (or what setClusterParams holds) with planes[k]; a capture without a
  // plane or a record gets none, and the Begin refuses the batch
  std::vector<agh_cluster_params> batchClusterParams(const std::vector<VectorXd>& planes,
    const std::vector<agh_cluster_params>* cluster_params) const
  {
    std::vector<agh_cluster_params> cp;
    for (std::size_t k = 0; k < planes.size() && planes[k].size() >= 4 && (!cluster_params || k < cluster_params->size()); k++)
    {
      cp.push_back(cluster_params ? (*cluster_params)[k] : cluster_);
      for (int q = 0; q < 4; q++)
        cp.back().plane[q] = planes[k](q);
    }
    return cp;
  }
  bool batchPlanesGiven(const char* fn, std::size_t n_captures, const std::vector<VectorXd>& planes,
    const std::vector<agh_cluster_params>* cluster_params) const
  {
    if (batchClusterParams(planes, cluster_params).size() == n_captures && planes.size() == n_captures &&
        (!cluster_params || cluster_params->size() == n_captures))
      return true;
    std::cout << " Error: " << fn << " needs one plane of four entries (and, where given, one cluster record) per capture\n";
    return false;
  }

  /** The objects of the last clustered batch collected (agh_get_batch_cluster_info): per list, capture after capture, the voxel
   *  count of its object (0: none); empty if the last chain collected was no clustered batch, if there was none, or while a
   *  chain is pending. */
  std::vector<std::int64_t> getBatchClusterSizes()
  {
    std::vector<agh_cluster_info> info;
    std::vector<std::int64_t> m;
    std::vector<std::int32_t> ids;
    if (search_)
      search_->batchClusterInfo(info, m, ids);
    return m;
  }

  /** the results of the labelled batch a labelled Begin queued, per capture and object.  A pending batch of another kind is not
   *  this call's to collect: it is refused (after printing) with an empty result, and that chain stays pending for
   *  localizeHandlesBatchEnd. */
  std::vector<std::vector<std::vector<Handle> > > localizeHandlesBatchLabeledEnd(
    std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object = nullptr)
  {
    const std::vector<int> objects = search_ ? search_->batchObjects() : std::vector<int>();
    std::vector<std::vector<std::vector<Handle> > > out = noLabeledHandles(objects, antipodal_hands_per_object);
    if (!pending_batch_.empty() && objects.empty())
    {
      std::cout << " Error: localizeHandlesBatchLabeledEnd while the pending batch is not a labelled one (localizeHandlesBatchEnd "
                   "collects it)\n";
      return out;
    }
    std::vector<std::vector<GraspHypothesis> > kept;
    const std::vector<std::vector<Handle> > flat = localizeHandlesBatchEnd(antipodal_hands_per_object ? &kept : nullptr);
    std::size_t l = 0;
    for (std::size_t k = 0; k < objects.size(); k++)
      for (std::size_t j = 0; j < (std::size_t) objects[k] && l < flat.size(); j++, l++)
      {
        out[k][j] = flat[l];
        if (antipodal_hands_per_object)
          (*antipodal_hands_per_object)[k][j] = kept[l];
      }
    return out;
  }

  /** The eligible voxels of every list of the last labelled batch collected (agh_get_batch_label_counts), capture after capture,
   *  object after object; empty if the last chain collected was no labelled batch, if there was none, or while a chain is
   *  pending. */
  std::vector<std::int64_t> getBatchLabelCounts()
  {
    return search_ ? search_->batchLabelCounts() : std::vector<std::int64_t>();
  }

  /** the searched hands, handles and inlier lists of one capture as the reference's objects (the tail of localizeHandlesEnd) */
  std::vector<Handle> toHandles(const PointCloud::Ptr& cloud_in, const std::vector<agh_hypothesis>& hands,
    const std::vector<agh_handle>& handles, const std::vector<std::int32_t>& idx, std::vector<GraspHypothesis>* antipodal_hands)
  {
    std::vector<Handle> handle_list;
    if (cloud_in)  // (a chain begun from depth images has no host cloud)
      remove_nan_in_place(*cloud_in);  // localization.cpp:27 filters the caller's cloud in place
    if (filters_boundaries_)
      std::cout << "Filtering out hands close to workspace boundaries ... (on the device, ahead of the classifier)\n";
    std::shared_ptr<std::vector<GraspHypothesis> > kept(new std::vector<GraspHypothesis>());
    kept->reserve(hands.size());
    for (std::size_t i = 0; i < hands.size(); i++)
    {
      kept->push_back(GraspHypothesis(hands[i], -1));
      kept->back().setFullAntipodal(true);  // learning.cpp:240
    }
    std::cout << kept->size() << " antipodal hand configurations found\n";  // localization.cpp:153
    if (antipodal_hands)
      *antipodal_hands = *kept;
    const std::shared_ptr<const std::vector<GraspHypothesis> > shared = kept;
    for (std::size_t h = 0; h < handles.size(); h++)
    {
      const agh_handle& r = handles[h];
      std::vector<int> in(idx.begin() + r.first_inlier, idx.begin() + r.first_inlier + r.n_inliers);
      handle_list.push_back(Handle(r, shared, in));
      std::cout << "handle found with " << in.size() << " inliers\n";  // handle_search.cpp:73
    }
    std::cout << "Handle Search\n " << handle_list.size() << " handles found\n";  // handle_search.cpp:82-84
    return handle_list;
  }

  /** the voxelised cloud and camera ids the last localizeHands searched (what the reference plots) */
  const PointCloud::Ptr& getSearchedCloud() const { return last_cloud_; }
  const VectorXi& getSearchedCamSource() const { return last_cam_; }

  /** localization.cpp:364-388 */
  std::vector<GraspHypothesis> filterHands(const std::vector<GraspHypothesis>& hand_list) const
  {
    const double MIN_DIST = 0.02;
    std::vector<GraspHypothesis> filtered;
    for (std::size_t i = 0; i < hand_list.size(); i++)
    {
      const Vector3d& center = hand_list[i].getGraspSurface();
      const int n_ws = (int) workspace_.size();  // (Eigen::Index is signed, the stand-in's size() is not)
      int k;
      for (k = 0; k < n_ws; k++)
        if (std::fabs(center((int) std::floor(k / 2.0)) - workspace_(k)) < MIN_DIST)
          break;
      if (k == n_ws)
        filtered.push_back(hand_list[i]);
    }
    return filtered;
  }

private:
  // One chain at a time: a Begin (or a blocking batch call) while one is pending prints this and fails, and the chain in flight
  // stays pending for its End.
  bool chainPending(const char* who, const char* end = "localizeHandlesEnd") const
  {
    if (!pending_cloud_ && !pending_depth_ && pending_batch_.empty())
      return false;
    std::cout << " Error: " << who << " while a chain is pending (" << end << " first)\n";
    return true;
  }
  // the per-object results of a labelled call as the reference's objects (the caller's cloud is filtered once, by the first)
  std::vector<std::vector<Handle> > labeledHandles(const PointCloud::Ptr& cloud_in, const std::vector<std::vector<agh_hypothesis> >& hands,
    const std::vector<std::vector<agh_handle> >& handles, const std::vector<std::vector<std::int32_t> >& idx,
    std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_object)
  {
    std::vector<std::vector<Handle> > out = noHandles(hands.size(), antipodal_hands_per_object);
    for (std::size_t j = 0; j < hands.size(); j++)
      out[j] = toHandles(j == 0 ? cloud_in : PointCloud::Ptr(), hands[j], handles[j], idx[j],
        antipodal_hands_per_object ? &(*antipodal_hands_per_object)[j] : nullptr);
    return out;
  }
  // a labelled batch is pending with one entry per LIST: a capture's host cloud (filtered once, in place) goes with its first
  void pendingLists(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& n_objects)
  {
    pending_batch_.clear();
    for (std::size_t k = 0; k < clouds.size(); k++)
      for (int j = 0; j < n_objects[k]; j++)
        pending_batch_.push_back(j == 0 ? clouds[k] : PointCloud::Ptr());
  }
  // what a labelled batch call returns when it fails: empty lists per capture and object (object counts outside 1 .. 64: none)
  static std::vector<std::vector<std::vector<Handle> > > noLabeledHandles(const std::vector<int>& n_objects,
    std::vector<std::vector<std::vector<GraspHypothesis> > >* antipodal_hands_per_object)
  {
    std::vector<std::vector<std::vector<Handle> > > out(n_objects.size());
    if (antipodal_hands_per_object)
      antipodal_hands_per_object->assign(n_objects.size(), std::vector<std::vector<GraspHypothesis> >());
    for (std::size_t k = 0; k < n_objects.size(); k++)
    {
      const std::size_t K = n_objects[k] >= 1 && n_objects[k] <= 64 ? (std::size_t) n_objects[k] : 0;
      out[k].resize(K);
      if (antipodal_hands_per_object)
        (*antipodal_hands_per_object)[k].resize(K);
    }
    return out;
  }
  // what a batch call returns when it fails: an empty list of handles, and of kept hands, per capture
  static std::vector<std::vector<Handle> > noHandles(std::size_t C, std::vector<std::vector<GraspHypothesis> >* antipodal_hands_per_cloud)
  {
    if (antipodal_hands_per_cloud)
      antipodal_hands_per_cloud->assign(C, std::vector<GraspHypothesis>());
    return std::vector<std::vector<Handle> >(C);
  }
  void init()
  {
    workspace_ = VectorXd(6);
    const double ws[6] = { -1.0, 1.0, -1.0, 1.0, -1.0, 1.0 };  // find_grasps.cpp:19
    for (int i = 0; i < 6; i++)
      workspace_(i) = ws[i];
    agh_default_cluster_params(&cluster_);
    agh_default_plane_fit_params(&plane_fit_);
    finger_width_ = 0.01;  // find_grasps.cpp:13-17
    hand_outer_diameter_ = 0.09;
    hand_depth_ = 0.06;
    init_bite_ = 0.01;
    hand_height_ = 0.02;
    nn_radius_taubin_ = 0.03;
    nn_radius_hands_ = 0.08;
    deterministic_ = false;
    device_ = 0;
  }
  void ensureSearch()
  {
    if (search_)
      return;
    search_.reset(new HandSearch(finger_width_, hand_outer_diameter_, hand_depth_, hand_height_, init_bite_,
      num_threads_, num_samples_, cam_tf_left_, false));
    search_->setCamTfRight(cam_tf_right_);
    search_->setDeterministicNormalEstimation(deterministic_);
    search_->setDevice(device_);
    search_->setKeepsTrainingImages(keeps_training_images_);
    if (sample_seed_set_)
      search_->setSampleSeed(sample_seed_);
    if (depth_filter_set_)
      search_->setDepthFilter(depth_filter_);
    if (voxel_filter_set_)
      search_->setVoxelFilter(voxel_filter_);
    if (hand_filter_set_)
      search_->setHandFilter(hand_filter_);
    if (hand_clearance_set_)
      search_->setHandClearance(hand_clearance_);
    if (handle_ranking_set_)
      search_->setHandleRanking(handle_ranking_);
  }

  int num_threads_, num_samples_;
  bool filters_boundaries_;
  agh_cluster_params cluster_;  // setClusterParams (the plane comes with each call)
  agh_plane_fit_params plane_fit_;  // setPlaneFitParams
  agh_depth_filter_params depth_filter_ = agh_depth_filter_params();  // setDepthFilter
  bool depth_filter_set_ = false;
  agh_voxel_filter_params voxel_filter_ = agh_voxel_filter_params();  // setVoxelFilter
  bool voxel_filter_set_ = false;
  agh_hand_filter_params hand_filter_ = agh_hand_filter_params();  // setHandFilter
  bool hand_filter_set_ = false;
  agh_hand_clearance_params hand_clearance_ = agh_hand_clearance_params();  // setHandClearance
  bool hand_clearance_set_ = false;
  agh_handle_ranking_params handle_ranking_ = agh_handle_ranking_params();  // setHandleRanking
  bool handle_ranking_set_ = false;
  int plotting_mode_;
  Matrix4d cam_tf_left_, cam_tf_right_;
  VectorXd workspace_;
  double finger_width_, hand_outer_diameter_, hand_depth_, init_bite_, hand_height_, nn_radius_taubin_, nn_radius_hands_;
  bool deterministic_;
  int device_;
  bool keeps_training_images_ = false;
  std::uint64_t sample_seed_ = 1;
  bool sample_seed_set_ = false;
  // localizeHandlesBegin -> localizeHandlesEnd
  PointCloud::Ptr pending_cloud_;
  bool pending_depth_ = false;  // (localizeHandlesDepthBegin -> localizeHandlesEnd: a chain without a host cloud)
  // localizeHandlesBatchBegin -> localizeHandlesBatchEnd (localizeHandlesDepthBatchBegin: one empty pointer per capture)
  std::vector<PointCloud::Ptr> pending_batch_;
  std::unique_ptr<HandSearch> search_;
  PointCloud::Ptr last_cloud_;
  VectorXi last_cam_;
};

}  // namespace agile_grasp_amd
#endif
