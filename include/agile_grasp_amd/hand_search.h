// hand_search.h -- HandSearch with the reference's constructor and findHands signature
// (include/agile_grasp/hand_search.h:77-85, 101-104) running on the MI355X through the agh C ABI.
//
// Differences a maintainer should know (all documented in DESIGN.md / INTEGRATION.md):
//  * no Plot member (hand_search.h:145 pulls in ROS + PCL visualisation); cloud_plot and plots_hands are accepted and
//    ignored;
//  * both camera poses are needed (the reference's HandSearch never initialises cam_tf_right_, hand_search.h:77-85):
//    pass it with setCamTfRight(), as Localization holds it (localization.h:343);
//  * uses_determinstic_normal_estimation_ (hand_search.h:84, hard-wired false) is exposed by
//    setDeterministicNormalEstimation(); `false` reproduces the reference's 50 x rand() % n subsample for ONE thread;
//  * explicit `indices` define hands_cam_source(i) = pts_cam_source(indices[i]) (the reference reads an empty vector
//    there, hand_search.cpp:166); an empty `indices` draws num_samples indices like pcl::RandomSample (hand_search.cpp:
//    36-39; PCL 1.7's algorithm restated, see randomSample) -- time-seeded like PCL unless setSampleSeed() is called.
//  * errors follow the reference's convention: a message on std::cout and an empty vector.
#ifndef AGILE_GRASP_AMD_HAND_SEARCH_H
#define AGILE_GRASP_AMD_HAND_SEARCH_H

#include <cstdint>
#include <cstdlib>
#include <ctime>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../agh.h"
#include "grasp_hypothesis.h"
#include "types.h"

namespace agile_grasp_amd
{

namespace detail
{
/** The two SVM-file steps of Learning::classify, shared by every call that classifies (Learning, HandSearch, Localization). */
inline bool svmFileExists(const std::string& svm_filename)
{
  std::ifstream f(svm_filename.c_str());
  if (!f.good())
    std::cout << " Error: File " << svm_filename << " does not exist!\n";  // learning.cpp:172-178
  return f.good();
}
inline bool loadSvm(agh_ctx* ctx, const std::string& svm_filename)
{
  if (agh_load_svm_file(ctx, svm_filename.c_str()) == AGH_OK)
    return true;
  std::cout << " Exception: " << agh_last_error(ctx) << "\n";  // learning.cpp:187-191
  return false;
}
}  // namespace detail

class HandSearch
{
public:
  HandSearch(double finger_width, double hand_outer_diameter, double hand_depth, double hand_height, double init_bite,
    int num_threads, int num_samples, const Matrix4d& cam_tf_left, bool plots_hands)
    : ctx_(nullptr), cam_tf_left_(cam_tf_left), cam_tf_right_(cam_tf_left), num_threads_(num_threads),
      num_samples_(num_samples), plots_hands_(plots_hands), deterministic_(false), sample_seed_(1), device_(0),
      dirty_(true), link_(new detail::SearchLink)
  {
    agh_default_params(&params_);
    params_.finger_width = finger_width;
    params_.hand_outer_diameter = hand_outer_diameter;
    params_.hand_depth = hand_depth;
    params_.hand_height = hand_height;
    params_.init_bite = init_bite;
    (void) num_threads_;
    (void) plots_hands_;
  }
  ~HandSearch()
  {
    link_->ctx = nullptr;  // hypotheses that outlive the search see that their device state is gone
    agh_destroy(ctx_);
  }
  HandSearch(const HandSearch&) = delete;
  HandSearch& operator=(const HandSearch&) = delete;

  void setCamTfRight(const Matrix4d& cam_tf_right)
  {
    cam_tf_right_ = cam_tf_right;
    dirty_ = true;
  }
  void setDeterministicNormalEstimation(bool b)
  {
    deterministic_ = b;
    dirty_ = true;
  }
  void setRandSeed(unsigned seed)  // srand() seed of the 50-point normal subsample (glibc default: 1)
  {
    params_.rand_seed = seed;
    dirty_ = true;
  }
  void setSampleSeed(std::uint64_t seed)  // pcl::RandomSample::setSeed; default: time(NULL) like PCL
  {
    sample_seed_ = seed;
    sample_seed_set_ = true;
  }
  void setDevice(int device)
  {
    device_ = device;
    dirty_ = true;
  }
  agh_ctx* context() { return ctx_; }
  /** GraspHypothesis::getPointsForLearning / getIndicesPointsForLearningCam1 / ...Cam2 (grasp_hypothesis.h:149-170) for
   *  a hypothesis of the most recent findHands of this search, into caller-owned containers (the hypothesis' own lazy
   *  getters do the same and cache the result).  Returns false (after printing why) on error, e.g. for a hypothesis of
   *  an earlier call or of another search. */
  bool getPointsForLearning(const GraspHypothesis& h, Matrix3Xd& points_for_learning, std::vector<int>& indices_cam1,
    std::vector<int>& indices_cam2)
  {
    indices_cam1.clear();
    indices_cam2.clear();
    resize_3xn(points_for_learning, 0);
    if (!ctx_ || h.getLiveContext() != ctx_)
    {
      std::cout << " Error: the hypothesis does not come from the most recent findHands of this search\n";
      return false;
    }
    const std::size_t n_b = (std::size_t) h.getNumPointsForLearning();
    std::vector<std::int32_t> cam(n_b + 1);
    std::int64_t n = 0;
    double* dst = resize_3xn(points_for_learning, n_b);
    std::vector<double> dummy(3);
    if (agh_get_learning_points(ctx_, h.getLocalIndex(), n_b ? dst : dummy.data(), cam.data(), (std::int64_t) n_b, &n) != AGH_OK)
    {
      std::cout << " Error in agh_get_learning_points: " << agh_last_error(ctx_) << "\n";
      resize_3xn(points_for_learning, 0);
      return false;
    }
    for (std::size_t k = 0; k < n_b; k++)  // rotating_hand.cpp:143-151
      if (cam[k] == 0)
        indices_cam1.push_back((int) k);
      else if (cam[k] == 1)
        indices_cam2.push_back((int) k);
    return true;
  }
  // pcl::RandomSample<PointT>::applyFilter(std::vector<int>&) as hand_search.cpp:36-39 uses it (setSample(num_samples_),
  // no input indices => all points).  PCL is THIRD PARTY and absent from /root/reference; this restates PCL 1.7's
  // filters/impl/random_sample.hpp: every index if num_samples >= N, else std::srand(seed) and Vitter's "Algorithm A"
  // (J. S. Vitter, ACM TOMS 13(1), 1987) with unifRand() = (float) (rand() / double(RAND_MAX)); the result is ascending.
  // PCL seeds with time(NULL) by default -- so does this unless setSampleSeed() was called -- hence the reference's own
  // samples are never reproducible and explicit `indices` are what parity tests use.  The srand() side effect on the
  // process-wide rand() stream is kept (it is the host's libc, as in the reference).
  static std::vector<std::int32_t> randomSample(std::int64_t n_points, int num_samples, unsigned seed)
  {
    std::vector<std::int32_t> idx;
    unsigned N = (unsigned) n_points;
    const unsigned sample = num_samples < 0 ? 0u : (unsigned) num_samples;
    if (sample >= N)
    {
      idx.resize((std::size_t) N);
      for (unsigned i = 0; i < N; i++)
        idx[i] = (std::int32_t) i;
      return idx;
    }
    if (sample == 0)
      return idx;
    idx.resize((std::size_t) sample);
    std::srand(seed);
    unsigned top = N - sample, i = 0, index = 0;
    for (std::size_t n = sample; n >= 2; n--)
    {
      const float V = (float) (std::rand() / double(RAND_MAX));
      unsigned S = 0;
      float quot = (float) top / (float) N;
      while (quot > V)
      {
        S++;
        top--;
        N--;
        quot = quot * (float) top / (float) N;
      }
      index += S;
      idx[i++] = (std::int32_t) index++;
      N--;
    }
    index += N * (unsigned) (float) (std::rand() / double(RAND_MAX));  // (PCL's cast truncates the variate, not the product)
    idx[i++] = (std::int32_t) index++;
    return idx;
  }

  /** The sample indices of the most recent findHands (the given ones, or the ones drawn for an empty list). */
  const std::vector<std::int32_t>& getLastSampleIndices() const { return last_samples_; }

  /** Multi-GPU (one process -- or, with joinLocalCommunicator, one host thread -- per GPU): after this call findHands is a
   *  COLLECTIVE: every rank passes the same cloud and the same `indices`, searches the slice [rank S / n, (rank + 1) S / n)
   *  of the samples (the reference's OpenMP fan-out over samples, hand_search.cpp:78,136, across GPUs) and receives the
   *  complete list through one RCCL all-gather issued by the library (agh_find_hands_sharded).  `id`: the bytes of
   *  agh_comm_unique_id() from ONE rank, handed to the others out of band.  Returns false (after printing why) on error. */
  bool joinCommunicator(int rank, int n_ranks, const std::uint8_t id[AGH_COMM_ID_BYTES])
  {
    if (!ensureContext())
      return false;
    if (agh_comm_init(ctx_, rank, n_ranks, id) != AGH_OK)
    {
      std::cout << " Error in agh_comm_init: " << agh_last_error(ctx_) << "\n";
      return false;
    }
    sharded_ = true;
    return true;
  }
  /** The same for searches that live in ONE process (one host thread each; they may share a GPU): the exchange is device
   *  copies instead of RCCL -- how the sharded schedule is validated on a single-GPU machine. */
  static bool joinLocalCommunicator(const std::vector<HandSearch*>& searches)
  {
    std::vector<agh_ctx*> ctxs;
    for (std::size_t i = 0; i < searches.size(); i++)
    {
      if (!searches[i] || !searches[i]->ensureContext())
        return false;
      ctxs.push_back(searches[i]->ctx_);
    }
    if (agh_comm_init_local(ctxs.data(), (std::int32_t) ctxs.size()) != AGH_OK)
    {
      std::cout << " Error in agh_comm_init_local\n";
      return false;
    }
    for (std::size_t i = 0; i < searches.size(); i++)
      searches[i]->sharded_ = true;
    return true;
  }
  bool isSharded() const { return sharded_; }

  /** Training runs (src/nodes/train.cpp): every findHands(calculates_antipodal = true) also attaches the three
   *  instance images to its hypotheses (GraspHypothesis::getTrainingImage), the input of Learning::train*. */
  void setKeepsTrainingImages(bool b) { keeps_training_images_ = b; }
  /** Default true: every hypothesis carries its packed 80x100 occupancy image (1000 bytes), which makes
   *  Learning::classify independent of this search's device state (any list, any time, like the reference's).  With
   *  false, only hypotheses of the most recent findHands can be classified (no image download). */
  void setKeepsImages(bool b) { keeps_images_ = b; }

  std::vector<GraspHypothesis> findHands(const PointCloud::Ptr cloud, const VectorXi& pts_cam_source,
    const std::vector<int>& indices, const PointCloud::Ptr cloud_plot, bool calculates_antipodal, bool uses_clustering)
  {
    (void) cloud_plot;
    (void) uses_clustering;
    std::vector<GraspHypothesis> hand_list;
    if (!cloud || cloud->size() == 0)
    {
      std::cout << "Input cloud is empty!\n";
      return hand_list;
    }
    if (!ensureContext())
      return hand_list;
    const std::int64_t n = (std::int64_t) cloud->size();
    std::vector<std::int32_t> cam((std::size_t) n, 0);
    for (std::int64_t i = 0; i < n && i < (std::int64_t) pts_cam_source.size(); i++)
      cam[(std::size_t) i] = pts_cam_source((std::size_t) i);
    int rc = agh_set_cloud(ctx_, &cloud->points[0].x, (std::int64_t) sizeof(cloud->points[0]), cam.data(), n);
    if (rc != AGH_OK)
      return fail("agh_set_cloud");
    return findHandsInSearchedCloud(indices, calculates_antipodal);
  }

  /** The head of Localization::localizeHands on the GPU (localization.cpp:17-45: camera ids, NaN removal, workspace
   *  box, per-camera voxelisation) followed by the search-structure build.  The voxelised cloud stays on the device as
   *  the cloud findHandsInSearchedCloud works on; a host copy is returned for the caller (plots, sample indices).
   *  @return false (after printing) on error */
  bool preprocess(const PointCloud::Ptr& cloud_in, int size_left, const VectorXd& workspace, double cell_size,
    PointCloud::Ptr& voxels_out, VectorXi& pts_cam_source_out)
  {
    if (!ensureContext())
      return false;
    double ws[6];
    for (int i = 0; i < 6; i++)
      ws[i] = workspace(i);
    std::int64_t nv = 0;
    const RawPoints in = rawPoints(*cloud_in);
    if (agh_preprocess(ctx_, in.xyz, in.stride, in.n, (std::int64_t) size_left, cloud_is_dense(*cloud_in) ? 1 : 0, ws, cell_size,
          &nv) != AGH_OK)
    {
      fail("agh_preprocess");
      return false;
    }
    return readBackCloud(nv, voxels_out, pts_cam_source_out);
  }

  /** The table-plane removal of localization.cpp:51-98 (pcl::SACSegmentation, RANSAC plane, then ExtractIndices with
   *  setNegative(true)) on the cloud the context holds (after preprocess): agh_remove_plane with the reference's settings.
   *  The non-planar points become the searched cloud; a host copy is returned.  As in the reference, the search then gives
   *  kept point i the camera id of point i of the UNSEGMENTED cloud (localization.cpp:88-94 builds cluster_cam_source but
   *  never uses it).  @return false (after printing) on error; result.found == 0 when no model was found */
  bool removePlane(agh_plane_result& result, PointCloud::Ptr& cloud_out, VectorXi& pts_cam_source_out)
  {
    if (!ensureContext())
      return false;
    agh_plane_params pp;
    agh_default_plane_params(&pp);  // setMaxIterations(100), setDistanceThreshold(0.01), PCL's seed / probability
    pp.cam_ids_by_position = 1;
    if (agh_remove_plane(ctx_, &pp, &result) != AGH_OK)
    {
      fail("agh_remove_plane");
      return false;
    }
    return readBackCloud(result.n_remaining, cloud_out, pts_cam_source_out);
  }

  /** The online chain of grasp_localizer.cpp:95-103 -- preprocessing, search, Learning::classify, HandleSearch -- as ONE device
   *  call with one synchronisation (agh_localize): the raw capture goes in, the hands the classifier kept, the handles and
   *  their inlier lists come out as records.  indices empty: num_samples indices are drawn ON THE DEVICE (one per stratum of
   *  the voxelised cloud, seeded like randomSample: setSampleSeed or the clock).  filters_boundaries: Localization::filterHands
   *  (the hands within 2 cm of a face of `workspace`) between the search and the classifier, on the device.
   *  @return false (after printing) on error */
  bool localize(const PointCloud::Ptr& cloud_in, int size_left, const VectorXd& workspace, double cell_size,
    const std::vector<int>& indices, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<agh_hypothesis>& hands_out, std::vector<agh_handle>& handles_out, std::vector<std::int32_t>& inliers_out,
    bool filters_boundaries = false)
  {
    hands_out.clear();
    handles_out.clear();
    inliers_out.clear();
    return localizeBegin(cloud_in, size_left, workspace, cell_size, indices, svm_filename, min_inliers, min_length,
             filters_boundaries) &&
           localizeEnd(hands_out, handles_out, inliers_out);
  }

  /** The same chain as two calls (agh_localize_begin / agh_localize_end), for a caller that holds the NEXT capture while this
   *  one is searched: between the two, localizeStage(next) uploads it on a second stream under this capture's kernels, and the
   *  localizeBegin that is later handed the same cloud object finds it on the device.  One chain may be in flight; `cloud_in`
   *  must stay alive and unchanged until localizeEnd has returned. */
  bool localizeBegin(const PointCloud::Ptr& cloud_in, int size_left, const VectorXd& workspace, double cell_size,
    const std::vector<int>& indices, const std::string& svm_filename, int min_inliers, double min_length,
    bool filters_boundaries = false)
  {
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    const std::vector<std::int32_t> idx(indices.begin(), indices.end());  // (copied by agh_localize_begin)
    const agh_localize_params lp = chainParams(size_left, cloud_is_dense(*cloud_in), workspace, cell_size, idx, sampleSeed(),
      min_inliers, min_length, filters_boundaries);
    const RawPoints in = rawPoints(*cloud_in);
    if (agh_localize_begin(ctx_, in.xyz, in.stride, in.n, &lp) != AGH_OK)
    {
      fail("agh_localize_begin");
      return false;
    }
    chainBegun(lp.n_samples);
    return true;
  }

  /** Additional: the chain of localize straight from the sensor's depth images (agh_localize_depth): one or two images, image k
   *  is camera k; no host-side expansion to points, and 2 or 4 bytes per pixel go up instead of a 32-byte point.  An image
   *  without a pose takes this search's k-th camera transform.  Outputs as for localize.  @return false (after printing) on error */
  bool localizeDepth(const std::vector<DepthImage>& images, const VectorXd& workspace, double cell_size,
    const std::vector<int>& indices, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<agh_hypothesis>& hands_out, std::vector<agh_handle>& handles_out, std::vector<std::int32_t>& inliers_out,
    bool filters_boundaries = false)
  {
    hands_out.clear();
    handles_out.clear();
    inliers_out.clear();
    return localizeDepthBegin(images, workspace, cell_size, indices, svm_filename, min_inliers, min_length, filters_boundaries) &&
           localizeEnd(hands_out, handles_out, inliers_out);
  }

  /** agh_localize_depth_begin: the chain queued, collected by localizeEnd; between the two, localizeDepthStage(next) uploads the
   *  next capture's images on a second stream, and the localizeDepthBegin that is later handed the same pixel buffers finds them
   *  on the device.  The pixel buffers must stay alive and unchanged until localizeEnd has returned. */
  bool localizeDepthBegin(const std::vector<DepthImage>& images, const VectorXd& workspace, double cell_size,
    const std::vector<int>& indices, const std::string& svm_filename, int min_inliers, double min_length,
    bool filters_boundaries = false)
  {
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    const std::vector<std::int32_t> idx(indices.begin(), indices.end());  // (copied by agh_localize_depth_begin)
    // (size_left is ignored: the first image's pixels are camera 0's)
    const agh_localize_params lp = chainParams(0, true, workspace, cell_size, idx, sampleSeed(), min_inliers, min_length,
      filters_boundaries);
    const std::vector<agh_depth_image> recs = depthRecords(images);
    if (agh_localize_depth_begin(ctx_, recs.empty() ? nullptr : recs.data(), (std::int32_t) recs.size(), &lp) != AGH_OK)
    {
      fail("agh_localize_depth_begin");
      return false;
    }
    chainBegun(lp.n_samples);
    return true;
  }

  /** Additional: the chain of localizeBegin with its num_samples drawn UNDER A MASK (agh_localize_masked_begin): `mask` holds one
   *  byte per point of cloud_in, non-zero = a sample may be drawn in the voxel this point falls into.  The whole cloud stays in
   *  the search.  Collected by localizeEnd; sampleMaskCount() then tells how many voxels were eligible.  `mask` is copied by the
   *  call; cloud_in must stay alive and unchanged until localizeEnd has returned. */
  bool localizeMaskedBegin(const PointCloud::Ptr& cloud_in, int size_left, const std::vector<std::uint8_t>& mask,
    const VectorXd& workspace, double cell_size, const std::string& svm_filename, int min_inliers, double min_length,
    bool filters_boundaries = false)
  {
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    if (mask.size() != cloud_in->points.size())
    {
      std::cout << " Error: localizeMaskedBegin needs one mask byte per point of the cloud\n";
      return false;
    }
    const agh_localize_params lp = chainParams(size_left, cloud_is_dense(*cloud_in), workspace, cell_size, std::vector<std::int32_t>(),
      sampleSeed(), min_inliers, min_length, filters_boundaries);
    const RawPoints in = rawPoints(*cloud_in);
    if (agh_localize_masked_begin(ctx_, in.xyz, in.stride, in.n, mask.data(), &lp) != AGH_OK)
    {
      fail("agh_localize_masked_begin");
      return false;
    }
    chainBegun(lp.n_samples);
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_masked_begin): masks[k] belongs to images[k]; a mask without data
   *  makes no pixel of its image eligible. */
  bool localizeDepthMaskedBegin(const std::vector<DepthImage>& images, const std::vector<SampleMask>& masks, const VectorXd& workspace,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    if (masks.size() != images.size())
    {
      std::cout << " Error: localizeDepthMaskedBegin needs one mask per image\n";
      return false;
    }
    const agh_localize_params lp = chainParams(0, true, workspace, cell_size, std::vector<std::int32_t>(), sampleSeed(), min_inliers,
      min_length, filters_boundaries);
    const std::vector<agh_depth_image> recs = depthRecords(images);
    std::vector<agh_sample_mask> mrecs(masks.size());
    for (std::size_t k = 0; k < masks.size(); k++)
    {
      mrecs[k].data = masks[k].data;
      mrecs[k].row_stride_bytes = masks[k].row_stride_bytes;
    }
    if (agh_localize_depth_masked_begin(ctx_, recs.empty() ? nullptr : recs.data(), mrecs.empty() ? nullptr : mrecs.data(),
          (std::int32_t) recs.size(), &lp) != AGH_OK)
    {
      fail("agh_localize_depth_masked_begin");
      return false;
    }
    chainBegun(lp.n_samples);
    return true;
  }

  /** agh_get_sample_mask_count: the eligible voxels of the last masked chain localizeEnd collected, -1 if it had no mask */
  std::int64_t sampleMaskCount()
  {
    std::int64_t m = -1;
    if (!ctx_ || agh_get_sample_mask_count(ctx_, &m) != AGH_OK)
      return -1;
    return m;
  }

  /** Additional: one capture, one sample list PER OBJECT of a label array (agh_localize_labeled): `labels` holds one byte per
   *  point of cloud_in, 0 = no object, j + 1 = object j of n_objects (1 .. 64); num_samples samples are drawn for EACH object
   *  among the voxels that hold one of its points, the search runs once over all of them on the whole cloud, and the handle
   *  search once per object, side by side.  Outputs per object, as localizeBatch's per capture; labelCounts() then gives the
   *  eligible voxels per object.  One blocking call.  @return false (after printing) on error */
  bool localizeLabeled(const PointCloud::Ptr& cloud_in, int size_left, const std::vector<std::uint8_t>& labels, int n_objects,
    const VectorXd& workspace, double cell_size, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<agh_hypothesis> >& hands_out, std::vector<std::vector<agh_handle> >& handles_out,
    std::vector<std::vector<std::int32_t> >& inliers_out, bool filters_boundaries = false)
  {
    labeledClear(n_objects, hands_out, handles_out, inliers_out);
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    if (!cloud_in || labels.size() != cloud_in->points.size())
    {
      std::cout << " Error: localizeLabeled needs one label byte per point of the cloud\n";
      return false;
    }
    const agh_localize_params lp = chainParams(size_left, cloud_is_dense(*cloud_in), workspace, cell_size, std::vector<std::int32_t>(),
      sampleSeed(), min_inliers, min_length, filters_boundaries);
    const RawPoints in = rawPoints(*cloud_in);
    LabeledOutputs o(n_objects, lp.n_samples);
    if (agh_localize_labeled(ctx_, in.xyz, in.stride, in.n, labels.data(), (std::int32_t) n_objects, &lp, o.handles.data(), o.cap,
          o.inl.data(), o.cap, o.hands.data(), o.cap, o.samples.data(), o.res.data()) != AGH_OK)
    {
      fail("agh_localize_labeled");
      return false;
    }
    labeledCollect(o, hands_out, handles_out, inliers_out);
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_labeled): labels[k] belongs to images[k]; a label image without data
   *  puts no pixel of its image into an object. */
  bool localizeDepthLabeled(const std::vector<DepthImage>& images, const std::vector<LabelImage>& labels, int n_objects,
    const VectorXd& workspace, double cell_size, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<agh_hypothesis> >& hands_out, std::vector<std::vector<agh_handle> >& handles_out,
    std::vector<std::vector<std::int32_t> >& inliers_out, bool filters_boundaries = false)
  {
    labeledClear(n_objects, hands_out, handles_out, inliers_out);
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    if (labels.size() != images.size())
    {
      std::cout << " Error: localizeDepthLabeled needs one label image per depth image\n";
      return false;
    }
    const agh_localize_params lp = chainParams(0, true, workspace, cell_size, std::vector<std::int32_t>(), sampleSeed(), min_inliers,
      min_length, filters_boundaries);
    const std::vector<agh_depth_image> recs = depthRecords(images);
    std::vector<agh_label_image> lrecs(labels.size());
    for (std::size_t k = 0; k < labels.size(); k++)
    {
      lrecs[k].data = labels[k].data;
      lrecs[k].row_stride_bytes = labels[k].row_stride_bytes;
    }
    LabeledOutputs o(n_objects, lp.n_samples);
    if (agh_localize_depth_labeled(ctx_, recs.empty() ? nullptr : recs.data(), lrecs.empty() ? nullptr : lrecs.data(),
          (std::int32_t) recs.size(), (std::int32_t) n_objects, &lp, o.handles.data(), o.cap, o.inl.data(), o.cap, o.hands.data(),
          o.cap, o.samples.data(), o.res.data()) != AGH_OK)
    {
      fail("agh_localize_depth_labeled");
      return false;
    }
    labeledCollect(o, hands_out, handles_out, inliers_out);
    return true;
  }

  /** agh_get_label_counts: the eligible voxels of every object of the last labelled call; empty if the last chain collected
   *  was not labelled */
  std::vector<std::int64_t> labelCounts()
  {
    std::vector<std::int64_t> m(64, -1);
    if (!ctx_ || agh_get_label_counts(ctx_, m.data(), 64) != AGH_OK)
      return std::vector<std::int64_t>();
    std::size_t k = 0;
    while (k < m.size() && m[k] >= 0)
      k++;
    m.resize(k);
    return m;
  }

  /** Additional: one capture, one sample list PER OBJECT THE CALL FINDS (agh_localize_clustered): the objects are the connected
   *  components of the voxels that stand above the support plane of `cp` (include/agh.h has the rules), at most cp.max_objects
   *  of them, largest first; from there on the call is localizeLabeled's.  Outputs per object (cp.max_objects lists);
   *  clusterInfo() and clusterLabels() then describe the objects.  One blocking call.  With `fp` the support plane is found on
   *  the device inside the call (agh_localize_clustered_fit: cp.plane is not read; planeFit() then reports it).
   *  @return false (after printing) on error */
  bool localizeClustered(const PointCloud::Ptr& cloud_in, int size_left, const agh_cluster_params& cp, const VectorXd& workspace,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<agh_hypothesis> >& hands_out, std::vector<std::vector<agh_handle> >& handles_out,
    std::vector<std::vector<std::int32_t> >& inliers_out, bool filters_boundaries = false, const agh_plane_fit_params* fp = nullptr)
  {
    labeledClear(cp.max_objects, hands_out, handles_out, inliers_out);
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    if (!cloud_in)
    {
      std::cout << " Error: localizeClustered needs a cloud\n";
      return false;
    }
    const agh_localize_params lp = chainParams(size_left, cloud_is_dense(*cloud_in), workspace, cell_size, std::vector<std::int32_t>(),
      sampleSeed(), min_inliers, min_length, filters_boundaries);
    const RawPoints in = rawPoints(*cloud_in);
    LabeledOutputs o(cp.max_objects, lp.n_samples);
    const int rc = fp ? agh_localize_clustered_fit(ctx_, in.xyz, in.stride, in.n, fp, &cp, &lp, o.handles.data(), o.cap, o.inl.data(),
                          o.cap, o.hands.data(), o.cap, o.samples.data(), o.res.data())
                      : agh_localize_clustered(ctx_, in.xyz, in.stride, in.n, &cp, &lp, o.handles.data(), o.cap, o.inl.data(), o.cap,
                          o.hands.data(), o.cap, o.samples.data(), o.res.data());
    if (rc != AGH_OK)
    {
      fail(fp ? "agh_localize_clustered_fit" : "agh_localize_clustered");
      return false;
    }
    labeledCollect(o, hands_out, handles_out, inliers_out);
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_clustered; with `fp`: agh_localize_depth_clustered_fit) */
  bool localizeDepthClustered(const std::vector<DepthImage>& images, const agh_cluster_params& cp, const VectorXd& workspace,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length,
    std::vector<std::vector<agh_hypothesis> >& hands_out, std::vector<std::vector<agh_handle> >& handles_out,
    std::vector<std::vector<std::int32_t> >& inliers_out, bool filters_boundaries = false, const agh_plane_fit_params* fp = nullptr)
  {
    labeledClear(cp.max_objects, hands_out, handles_out, inliers_out);
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    const agh_localize_params lp = chainParams(0, true, workspace, cell_size, std::vector<std::int32_t>(), sampleSeed(), min_inliers,
      min_length, filters_boundaries);
    const std::vector<agh_depth_image> recs = depthRecords(images);
    LabeledOutputs o(cp.max_objects, lp.n_samples);
    const agh_depth_image* im = recs.empty() ? nullptr : recs.data();
    const int rc = fp ? agh_localize_depth_clustered_fit(ctx_, im, (std::int32_t) recs.size(), fp, &cp, &lp, o.handles.data(), o.cap,
                          o.inl.data(), o.cap, o.hands.data(), o.cap, o.samples.data(), o.res.data())
                      : agh_localize_depth_clustered(ctx_, im, (std::int32_t) recs.size(), &cp, &lp, o.handles.data(), o.cap,
                          o.inl.data(), o.cap, o.hands.data(), o.cap, o.samples.data(), o.res.data());
    if (rc != AGH_OK)
    {
      fail(fp ? "agh_localize_depth_clustered_fit" : "agh_localize_depth_clustered");
      return false;
    }
    labeledCollect(o, hands_out, handles_out, inliers_out);
    return true;
  }

  /** agh_get_cluster_info: the counts of the last clustered call, the voxels M_j and the smallest voxel index of every list
   *  (0 and -1 for a list without an object); false, with everything cleared, if the last chain collected was not clustered */
  bool clusterInfo(agh_cluster_info& info, std::vector<std::int64_t>& n_voxels, std::vector<std::int32_t>& ids)
  {
    std::vector<std::int64_t> m(64, -2);
    std::vector<std::int32_t> id(64, -2);
    info = agh_cluster_info();
    n_voxels.clear();
    ids.clear();
    if (!ctx_ || agh_get_cluster_info(ctx_, &info, m.data(), id.data(), 64) != AGH_OK)
      return false;
    std::size_t k = 0;
    while (k < m.size() && m[k] > -2)
      k++;
    n_voxels.assign(m.begin(), m.begin() + (std::ptrdiff_t) k);
    ids.assign(id.begin(), id.begin() + (std::ptrdiff_t) k);
    return true;
  }

  /** agh_get_plane_fit: the plane, the counts and the flags of the last fitted call; false, with a zeroed record, if the last
   *  chain collected was not a fitted one */
  bool planeFit(agh_plane_fit_result& result)
  {
    result = agh_plane_fit_result();
    return ctx_ && agh_get_plane_fit(ctx_, &result) == AGH_OK;
  }

  /** agh_get_cluster_labels: per voxel of the searched cloud 0 or object + 1; empty if the last chain was not clustered */
  std::vector<std::uint8_t> clusterLabels()
  {
    std::vector<std::uint8_t> out((std::size_t) (searched_n_ > 0 ? searched_n_ : 0) + 1);
    const int nv = ctx_ ? agh_get_cluster_labels(ctx_, out.data(), (std::int64_t) out.size()) : -1;
    out.resize(nv > 0 ? (std::size_t) nv : 0);
    return out;
  }

  /** agh_localize_depth_stage: the NEXT capture's images up, beside the chain in flight */
  bool localizeDepthStage(const std::vector<DepthImage>& next)
  {
    if (!ensureContext())
      return false;
    const std::vector<agh_depth_image> recs = depthRecords(next);
    if (agh_localize_depth_stage(ctx_, recs.empty() ? nullptr : recs.data(), (std::int32_t) recs.size()) != AGH_OK)
    {
      fail("agh_localize_depth_stage");
      return false;
    }
    return true;
  }

  /** Additional: localizeBatch straight from depth images (agh_localize_depth_batch = localizeDepthBatchBegin +
   *  localizeBatchEnd): capture k is captures[k], one or two images (image j is camera j; an image without a pose takes this
   *  search's j-th camera transform), with workspaces[k] and indices[k] (empty: num_samples drawn on the device, seeded with
   *  the sample seed + k).  Outputs per capture as for localizeBatch.  @return false (after printing) on error */
  bool localizeDepthBatch(const std::vector<std::vector<DepthImage> >& captures, const std::vector<VectorXd>& workspaces,
    double cell_size, const std::vector<std::vector<int> >& indices, const std::string& svm_filename, int min_inliers,
    double min_length, std::vector<std::vector<agh_hypothesis> >& hands_out, std::vector<std::vector<agh_handle> >& handles_out,
    std::vector<std::vector<std::int32_t> >& inliers_out, bool filters_boundaries = false)
  {
    const std::size_t C = captures.size();
    hands_out.assign(C, std::vector<agh_hypothesis>());
    handles_out.assign(C, std::vector<agh_handle>());
    inliers_out.assign(C, std::vector<std::int32_t>());
    return localizeDepthBatchBegin(captures, workspaces, cell_size, indices, svm_filename, min_inliers, min_length,
             filters_boundaries) &&
           localizeBatchEnd(hands_out, handles_out, inliers_out);
  }

  /** agh_localize_depth_batch_begin: the batch's chain queued, collected by localizeBatchEnd.  The pixel buffers must stay alive
   *  and unchanged until localizeBatchEnd has returned.  A Begin that fails leaves a chain in flight as it was. */
  bool localizeDepthBatchBegin(const std::vector<std::vector<DepthImage> >& captures, const std::vector<VectorXd>& workspaces,
    double cell_size, const std::vector<std::vector<int> >& indices, const std::string& svm_filename, int min_inliers,
    double min_length, bool filters_boundaries = false)
  {
    const std::size_t C = captures.size();
    if (C == 0 || workspaces.size() != C || indices.size() != C)
    {
      std::cout << " Error: localizeDepthBatchBegin needs one workspace and index list per capture\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_depth_image> recs;  // (the flat array in capture order; copied by the library's begin, like the arrays below)
    std::vector<std::int32_t> n_images(C);
    std::vector<agh_localize_params> lp(C);
    std::vector<std::vector<std::int32_t> > idx(C);
    std::int64_t cap = 1, n_samples = 0;
    for (std::size_t k = 0; k < C; k++)
    {
      const std::vector<agh_depth_image> r = depthRecords(captures[k]);
      recs.insert(recs.end(), r.begin(), r.end());
      n_images[k] = (std::int32_t) r.size();
      idx[k].assign(indices[k].begin(), indices[k].end());
      // (size_left and dense are ignored: each capture's first image holds its camera 0's pixels)
      lp[k] = chainParams(0, true, workspaces[k], cell_size, idx[k], seed + (std::uint64_t) k, min_inliers, min_length,
        filters_boundaries);
      cap += handsRoom(lp[k].n_samples);
      n_samples += lp[k].n_samples;
    }
    if (agh_localize_depth_batch_begin(ctx_, recs.empty() ? nullptr : recs.data(), n_images.data(), lp.data(), (std::int32_t) C) !=
        AGH_OK)
    {
      fail("agh_localize_depth_batch_begin");
      return false;
    }
    batch_captures_ = C;
    batch_cap_ = cap;
    batch_samples_ = n_samples;
    batch_objects_.clear();
    return true;
  }

  /** Additional: the chain of localize over several captures in one call (localizeBatchBegin + localizeBatchEnd): capture k is clouds[k] with
   *  sizes_left[k], workspaces[k] and indices[k] (empty: num_samples drawn on the device, seeded with the sample seed + k).
   *  Per capture the hands the classifier kept, the handles and their inlier lists (indices into that capture's hands), exactly
   *  what localize returns for it.  @return false (after printing) on error */
  bool localizeBatch(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<VectorXd>& workspaces, double cell_size, const std::vector<std::vector<int> >& indices,
    const std::string& svm_filename, int min_inliers, double min_length, std::vector<std::vector<agh_hypothesis> >& hands_out,
    std::vector<std::vector<agh_handle> >& handles_out, std::vector<std::vector<std::int32_t> >& inliers_out,
    bool filters_boundaries = false)
  {
    const std::size_t C = clouds.size();
    hands_out.assign(C, std::vector<agh_hypothesis>());
    handles_out.assign(C, std::vector<agh_handle>());
    inliers_out.assign(C, std::vector<std::int32_t>());
    if (C == 0 || sizes_left.size() != C || workspaces.size() != C || indices.size() != C)
    {
      std::cout << " Error: localizeBatch needs one size_left, workspace and index list per cloud\n";
      return false;
    }
    return localizeBatchBegin(clouds, sizes_left, workspaces, cell_size, indices, svm_filename, min_inliers, min_length,
             filters_boundaries) &&
           localizeBatchEnd(hands_out, handles_out, inliers_out);
  }

  /** Additional: localizeBatch as two calls (agh_localize_batch_begin / agh_localize_batch_end), for a caller that walks over
   *  many batches: between the two, localizeBatchStage(next clouds) uploads the next batch on a second stream under this batch's
   *  kernels, and the localizeBatchBegin that is later handed the same cloud objects finds them on the device.  Arguments as for
   *  localizeBatch.  One chain may be in flight: a Begin that fails (a chain in flight included) leaves the one in flight, and
   *  what localizeBatchEnd needs for it, as they were.  The clouds must stay alive and unchanged until localizeBatchEnd has
   *  returned.  @return false (after printing) on error */
  bool localizeBatchBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<VectorXd>& workspaces, double cell_size, const std::vector<std::vector<int> >& indices,
    const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    const std::size_t C = clouds.size();
    if (C == 0 || sizes_left.size() != C || workspaces.size() != C || indices.size() != C)
    {
      std::cout << " Error: localizeBatchBegin needs one size_left, workspace and index list per cloud\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    RawBatch in;
    if (!rawPoints(clouds, in))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_localize_params> lp(C);
    std::vector<std::vector<std::int32_t> > idx(C);  // (copied by agh_localize_batch_begin, like the arrays below)
    std::int64_t cap = 1, n_samples = 0;
    for (std::size_t k = 0; k < C; k++)
    {
      idx[k].assign(indices[k].begin(), indices[k].end());
      lp[k] = chainParams(sizes_left[k], cloud_is_dense(*clouds[k]), workspaces[k], cell_size, idx[k], seed + (std::uint64_t) k,
        min_inliers, min_length, filters_boundaries);
      cap += handsRoom(lp[k].n_samples);
      n_samples += lp[k].n_samples;
    }
    if (agh_localize_batch_begin(ctx_, in.xyz.data(), in.stride.data(), in.n.data(), lp.data(), (std::int32_t) C) != AGH_OK)
    {
      fail("agh_localize_batch_begin");
      return false;
    }
    batch_captures_ = C;
    batch_cap_ = cap;
    batch_samples_ = n_samples;
    batch_objects_.clear();
    return true;
  }

  /** Additional: localizeBatchBegin with every capture's num_samples drawn UNDER ITS OWN MASK (agh_localize_batch_masked_begin):
   *  masks[k] holds one byte per point of clouds[k], non-zero = a sample may be drawn in the voxel this point falls into; the
   *  whole capture stays in the search.  Capture k is seeded with the sample seed + k.  Collected by localizeBatchEnd;
   *  batchMaskCounts() then gives the eligible voxels per capture.  The masks are copied by the call; the clouds must stay alive
   *  and unchanged until localizeBatchEnd has returned.  A Begin that fails leaves a chain in flight as it was. */
  bool localizeBatchMaskedBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<std::uint8_t> >& masks, const std::vector<VectorXd>& workspaces, double cell_size,
    const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    const std::size_t C = clouds.size();
    if (C == 0 || sizes_left.size() != C || workspaces.size() != C || masks.size() != C)
    {
      std::cout << " Error: localizeBatchMaskedBegin needs one size_left, workspace and mask per cloud\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    RawBatch in;
    if (!rawPoints(clouds, in))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_localize_params> lp(C);
    std::vector<const std::uint8_t*> mptr(C);
    std::int64_t cap = 1, n_samples = 0;
    for (std::size_t k = 0; k < C; k++)
    {
      if (masks[k].size() != clouds[k]->points.size())
      {
        std::cout << " Error: localizeBatchMaskedBegin needs one mask byte per point of every cloud\n";
        return false;
      }
      mptr[k] = masks[k].data();
      lp[k] = chainParams(sizes_left[k], cloud_is_dense(*clouds[k]), workspaces[k], cell_size, std::vector<std::int32_t>(),
        seed + (std::uint64_t) k, min_inliers, min_length, filters_boundaries);
      cap += handsRoom(lp[k].n_samples);
      n_samples += lp[k].n_samples;
    }
    if (agh_localize_batch_masked_begin(ctx_, in.xyz.data(), in.stride.data(), in.n.data(), mptr.data(), lp.data(), (std::int32_t) C) !=
        AGH_OK)
    {
      fail("agh_localize_batch_masked_begin");
      return false;
    }
    batch_captures_ = C;
    batch_cap_ = cap;
    batch_samples_ = n_samples;
    batch_objects_.clear();
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_batch_masked_begin): masks[k][j] belongs to captures[k][j]; a mask
   *  without data makes no pixel of its image eligible, and every capture needs at least one mask with data. */
  bool localizeDepthBatchMaskedBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<SampleMask> >& masks, const std::vector<VectorXd>& workspaces, double cell_size,
    const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    const std::size_t C = captures.size();
    if (C == 0 || workspaces.size() != C || masks.size() != C)
    {
      std::cout << " Error: localizeDepthBatchMaskedBegin needs one workspace and mask list per capture\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_depth_image> recs;  // (the flat arrays in capture order; copied by the library's begin, like the arrays below)
    std::vector<agh_sample_mask> mrecs;
    std::vector<std::int32_t> n_images(C);
    std::vector<agh_localize_params> lp(C);
    std::int64_t cap = 1, n_samples = 0;
    for (std::size_t k = 0; k < C; k++)
    {
      if (masks[k].size() != captures[k].size())
      {
        std::cout << " Error: localizeDepthBatchMaskedBegin needs one mask per image\n";
        return false;
      }
      const std::vector<agh_depth_image> r = depthRecords(captures[k]);
      recs.insert(recs.end(), r.begin(), r.end());
      for (std::size_t j = 0; j < masks[k].size(); j++)
      {
        agh_sample_mask m;
        m.data = masks[k][j].data;
        m.row_stride_bytes = masks[k][j].row_stride_bytes;
        mrecs.push_back(m);
      }
      n_images[k] = (std::int32_t) r.size();
      lp[k] = chainParams(0, true, workspaces[k], cell_size, std::vector<std::int32_t>(), seed + (std::uint64_t) k, min_inliers,
        min_length, filters_boundaries);
      cap += handsRoom(lp[k].n_samples);
      n_samples += lp[k].n_samples;
    }
    if (agh_localize_depth_batch_masked_begin(ctx_, recs.empty() ? nullptr : recs.data(), mrecs.empty() ? nullptr : mrecs.data(),
          n_images.data(), lp.data(), (std::int32_t) C) != AGH_OK)
    {
      fail("agh_localize_depth_batch_masked_begin");
      return false;
    }
    batch_captures_ = C;
    batch_cap_ = cap;
    batch_samples_ = n_samples;
    batch_objects_.clear();
    return true;
  }

  /** agh_get_batch_mask_counts: the eligible voxels of every capture of the last masked batch localizeBatchEnd collected; empty
   *  if the last chain collected was no masked batch */
  std::vector<std::int64_t> batchMaskCounts()
  {
    std::vector<std::int64_t> m(64, -1);
    if (!ctx_ || agh_get_batch_mask_counts(ctx_, m.data(), 64) != AGH_OK)
      return std::vector<std::int64_t>();
    std::size_t k = 0;
    while (k < m.size() && m[k] >= 0)
      k++;
    m.resize(k);
    return m;
  }

  /** Additional: localizeBatchBegin with one sample list PER OBJECT of every capture's label array
   *  (agh_localize_batch_labeled_begin): labels[k] holds one byte per point of clouds[k] (0 = no object, j + 1 = object j of
   *  n_objects[k]), num_samples samples are drawn per object, capture k's objects seeded with the sample seed + k.  The call has
   *  a LIST per (capture, object), at most 64 in all: localizeBatchEnd returns one entry per list, capture after capture, object
   *  after object (batchObjects() says how many of them belong to each capture), and batchLabelCounts() then gives the eligible
   *  voxels per list.  The labels are copied by the call; the clouds must stay alive and unchanged until localizeBatchEnd has
   *  returned.  A Begin that fails leaves a chain in flight as it was. */
  bool localizeBatchLabeledBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<std::vector<std::uint8_t> >& labels, const std::vector<int>& n_objects, const std::vector<VectorXd>& workspaces,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    const std::size_t C = clouds.size();
    if (C == 0 || sizes_left.size() != C || workspaces.size() != C || labels.size() != C || n_objects.size() != C)
    {
      std::cout << " Error: localizeBatchLabeledBegin needs one size_left, workspace, label array and object count per cloud\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    RawBatch in;
    if (!rawPoints(clouds, in))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_localize_params> lp(C);
    std::vector<const std::uint8_t*> lptr(C);
    std::vector<std::int32_t> objects(n_objects.begin(), n_objects.end());
    for (std::size_t k = 0; k < C; k++)
    {
      if (labels[k].size() != clouds[k]->points.size())
      {
        std::cout << " Error: localizeBatchLabeledBegin needs one label byte per point of every cloud\n";
        return false;
      }
      lptr[k] = labels[k].data();
      lp[k] = chainParams(sizes_left[k], cloud_is_dense(*clouds[k]), workspaces[k], cell_size, std::vector<std::int32_t>(),
        seed + (std::uint64_t) k, min_inliers, min_length, filters_boundaries);
    }
    if (agh_localize_batch_labeled_begin(ctx_, in.xyz.data(), in.stride.data(), in.n.data(), lptr.data(), objects.data(), lp.data(),
          (std::int32_t) C) != AGH_OK)
    {
      fail("agh_localize_batch_labeled_begin");
      return false;
    }
    labeledBatchQueued(n_objects, lp);
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_batch_labeled_begin): labels[k][j] belongs to captures[k][j]; a
   *  label image without data puts no pixel of its image into an object, and every capture needs at least one with data. */
  bool localizeDepthBatchLabeledBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<std::vector<LabelImage> >& labels, const std::vector<int>& n_objects, const std::vector<VectorXd>& workspaces,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    const std::size_t C = captures.size();
    if (C == 0 || workspaces.size() != C || labels.size() != C || n_objects.size() != C)
    {
      std::cout << " Error: localizeDepthBatchLabeledBegin needs one workspace, label image list and object count per capture\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_depth_image> recs;  // (the flat arrays in capture order; copied by the library's begin, like the arrays below)
    std::vector<agh_label_image> lrecs;
    std::vector<std::int32_t> n_images(C);
    std::vector<std::int32_t> objects(n_objects.begin(), n_objects.end());
    std::vector<agh_localize_params> lp(C);
    for (std::size_t k = 0; k < C; k++)
    {
      if (labels[k].size() != captures[k].size())
      {
        std::cout << " Error: localizeDepthBatchLabeledBegin needs one label image per image\n";
        return false;
      }
      const std::vector<agh_depth_image> r = depthRecords(captures[k]);
      recs.insert(recs.end(), r.begin(), r.end());
      for (std::size_t j = 0; j < labels[k].size(); j++)
      {
        agh_label_image m;
        m.data = labels[k][j].data;
        m.row_stride_bytes = labels[k][j].row_stride_bytes;
        lrecs.push_back(m);
      }
      n_images[k] = (std::int32_t) r.size();
      lp[k] = chainParams(0, true, workspaces[k], cell_size, std::vector<std::int32_t>(), seed + (std::uint64_t) k, min_inliers,
        min_length, filters_boundaries);
    }
    if (agh_localize_depth_batch_labeled_begin(ctx_, recs.empty() ? nullptr : recs.data(), lrecs.empty() ? nullptr : lrecs.data(),
          n_images.data(), objects.data(), lp.data(), (std::int32_t) C) != AGH_OK)
    {
      fail("agh_localize_depth_batch_labeled_begin");
      return false;
    }
    labeledBatchQueued(n_objects, lp);
    return true;
  }

  /** Additional: localizeBatchLabeledBegin WITHOUT A SEGMENTER (agh_localize_batch_clustered_begin): capture k's objects are the
   *  connected components of its own voxels above the support plane of cp[k], cp[k].max_objects lists each (at most 64 in all),
   *  found on the device inside the one chain; num_samples samples are drawn per object, capture k's objects seeded with the
   *  sample seed + k.  localizeBatchEnd returns one entry per list (batchObjects() says how many belong to each capture), and
   *  batchClusterInfo() then describes the objects.  The records are copied by the call; the clouds must stay alive and unchanged
   *  until localizeBatchEnd has returned.  A Begin that fails leaves a chain in flight as it was. */
  bool localizeBatchClusteredBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<agh_cluster_params>& cp, const std::vector<VectorXd>& workspaces, double cell_size,
    const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    return batchClusteredBegin(clouds, sizes_left, nullptr, cp, workspaces, cell_size, svm_filename, min_inliers, min_length,
      filters_boundaries);
  }

  /** Additional: localizeBatchClusteredBegin WITHOUT A CALIBRATED PLANE (agh_localize_batch_clustered_fit_begin): capture k's
   *  support plane is found on the device inside the chain, on its own voxels, with fp[k] (one record per capture: rigs have
   *  their own thresholds and seeds); cp[k].plane is not read, and batchPlaneFit() then reports the planes. */
  bool localizeBatchClusteredFitBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<agh_plane_fit_params>& fp, const std::vector<agh_cluster_params>& cp, const std::vector<VectorXd>& workspaces,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    return batchClusteredBegin(clouds, sizes_left, &fp, cp, workspaces, cell_size, svm_filename, min_inliers, min_length,
      filters_boundaries);
  }

  // the two calls above (fp: the fitted one's records, or nullptr)
  bool batchClusteredBegin(const std::vector<PointCloud::Ptr>& clouds, const std::vector<int>& sizes_left,
    const std::vector<agh_plane_fit_params>* fp, const std::vector<agh_cluster_params>& cp, const std::vector<VectorXd>& workspaces,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries)
  {
    const std::size_t C = clouds.size();
    if (C == 0 || sizes_left.size() != C || workspaces.size() != C || cp.size() != C || (fp && fp->size() != C))
    {
      std::cout << " Error: localizeBatchClusteredBegin needs one size_left, workspace and cluster record per cloud\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    RawBatch in;
    if (!rawPoints(clouds, in))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_localize_params> lp(C);
    for (std::size_t k = 0; k < C; k++)
      lp[k] = chainParams(sizes_left[k], cloud_is_dense(*clouds[k]), workspaces[k], cell_size, std::vector<std::int32_t>(),
        seed + (std::uint64_t) k, min_inliers, min_length, filters_boundaries);
    const int rc = fp ? agh_localize_batch_clustered_fit_begin(ctx_, in.xyz.data(), in.stride.data(), in.n.data(), fp->data(),
                          cp.data(), lp.data(), (std::int32_t) C)
                      : agh_localize_batch_clustered_begin(ctx_, in.xyz.data(), in.stride.data(), in.n.data(), cp.data(), lp.data(),
                          (std::int32_t) C);
    if (rc != AGH_OK)
    {
      fail(fp ? "agh_localize_batch_clustered_fit_begin" : "agh_localize_batch_clustered_begin");
      return false;
    }
    labeledBatchQueued(clusterObjects(cp), lp);
    return true;
  }

  /** ... and straight from depth images (agh_localize_depth_batch_clustered_begin) */
  bool localizeDepthBatchClusteredBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<agh_cluster_params>& cp, const std::vector<VectorXd>& workspaces, double cell_size,
    const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    return depthBatchClusteredBegin(captures, nullptr, cp, workspaces, cell_size, svm_filename, min_inliers, min_length,
      filters_boundaries);
  }

  /** ... and localizeBatchClusteredFitBegin straight from depth images (agh_localize_depth_batch_clustered_fit_begin) */
  bool localizeDepthBatchClusteredFitBegin(const std::vector<std::vector<DepthImage> >& captures,
    const std::vector<agh_plane_fit_params>& fp, const std::vector<agh_cluster_params>& cp, const std::vector<VectorXd>& workspaces,
    double cell_size, const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries = false)
  {
    return depthBatchClusteredBegin(captures, &fp, cp, workspaces, cell_size, svm_filename, min_inliers, min_length,
      filters_boundaries);
  }

  bool depthBatchClusteredBegin(const std::vector<std::vector<DepthImage> >& captures, const std::vector<agh_plane_fit_params>* fp,
    const std::vector<agh_cluster_params>& cp, const std::vector<VectorXd>& workspaces, double cell_size,
    const std::string& svm_filename, int min_inliers, double min_length, bool filters_boundaries)
  {
    const std::size_t C = captures.size();
    if (C == 0 || workspaces.size() != C || cp.size() != C || (fp && fp->size() != C))
    {
      std::cout << " Error: localizeDepthBatchClusteredBegin needs one workspace and cluster record per capture\n";
      return false;
    }
    if (!ensureContext() || !detail::loadSvm(ctx_, svm_filename))
      return false;
    const std::uint64_t seed = sampleSeed();
    std::vector<agh_depth_image> recs;  // (the flat array in capture order; copied by the library's begin, like the arrays below)
    std::vector<std::int32_t> n_images(C);
    std::vector<agh_localize_params> lp(C);
    for (std::size_t k = 0; k < C; k++)
    {
      const std::vector<agh_depth_image> r = depthRecords(captures[k]);
      recs.insert(recs.end(), r.begin(), r.end());
      n_images[k] = (std::int32_t) r.size();
      lp[k] = chainParams(0, true, workspaces[k], cell_size, std::vector<std::int32_t>(), seed + (std::uint64_t) k, min_inliers,
        min_length, filters_boundaries);
    }
    const agh_depth_image* images = recs.empty() ? nullptr : recs.data();
    const int rc = fp ? agh_localize_depth_batch_clustered_fit_begin(ctx_, images, n_images.data(), fp->data(), cp.data(), lp.data(),
                          (std::int32_t) C)
                      : agh_localize_depth_batch_clustered_begin(ctx_, images, n_images.data(), cp.data(), lp.data(), (std::int32_t) C);
    if (rc != AGH_OK)
    {
      fail(fp ? "agh_localize_depth_batch_clustered_fit_begin" : "agh_localize_depth_batch_clustered_begin");
      return false;
    }
    labeledBatchQueued(clusterObjects(cp), lp);
    return true;
  }

  /** the lists per capture of a clustered batch: max_objects of every record */
  static std::vector<int> clusterObjects(const std::vector<agh_cluster_params>& cp)
  {
    std::vector<int> objects(cp.size());
    for (std::size_t k = 0; k < cp.size(); k++)
      objects[k] = (int) cp[k].max_objects;
    return objects;
  }

  /** agh_get_batch_cluster_info: per capture of the last clustered batch localizeBatchEnd collected its counts, and per list, in
   *  list order, the object's voxel count and its smallest capture-local voxel index (0 and -1: a list without an object).
   *  @return false if the last chain collected was no clustered batch */
  bool batchClusterInfo(std::vector<agh_cluster_info>& info, std::vector<std::int64_t>& n_voxels, std::vector<std::int32_t>& ids)
  {
    std::size_t lists = 0;
    for (std::size_t k = 0; k < batch_objects_.size(); k++)
      lists += (std::size_t) batch_objects_[k];
    info.assign(64, agh_cluster_info());
    n_voxels.assign(64, 0);
    ids.assign(64, -1);
    if (!ctx_ || agh_get_batch_cluster_info(ctx_, info.data(), n_voxels.data(), ids.data(), 64, 64) != AGH_OK)
    {
      info.clear();
      n_voxels.clear();
      ids.clear();
      return false;
    }
    info.resize(batch_objects_.size());
    n_voxels.resize(lists);
    ids.resize(lists);
    return true;
  }

  /** agh_get_batch_plane_fit: one record per capture of the last fitted batch localizeBatchEnd collected.
   *  @return false (and no record) if the last chain collected was no fitted batch */
  bool batchPlaneFit(std::vector<agh_plane_fit_result>& results)
  {
    results.assign(64, agh_plane_fit_result());
    const int n = ctx_ ? agh_get_batch_plane_fit(ctx_, results.data(), 64) : -1;
    results.resize(n > 0 ? (std::size_t) n : 0);
    return n > 0;
  }

  /** the objects per capture of the labelled batch in flight or last collected (empty: that batch was not labelled) */
  const std::vector<int>& batchObjects() const { return batch_objects_; }

  /** agh_get_batch_label_counts: the eligible voxels of every list of the last labelled batch localizeBatchEnd collected, in
   *  list order; empty if the last chain collected was no labelled batch */
  std::vector<std::int64_t> batchLabelCounts()
  {
    std::vector<std::int64_t> m(64, -1);
    if (!ctx_ || agh_get_batch_label_counts(ctx_, m.data(), 64) != AGH_OK)
      return std::vector<std::int64_t>();
    std::size_t k = 0;
    while (k < m.size() && m[k] >= 0)
      k++;
    m.resize(k);
    return m;
  }

  /** agh_localize_batch_stage: the NEXT batch's clouds up, beside the chain in flight (keep them alive and unchanged until the
   *  localizeBatchEnd of the chain that searches them has returned). */
  bool localizeBatchStage(const std::vector<PointCloud::Ptr>& next)
  {
    if (next.empty() || !ensureContext())
      return false;
    RawBatch in;
    if (!rawPoints(next, in))
      return false;
    if (agh_localize_batch_stage(ctx_, in.xyz.data(), in.stride.data(), in.n.data(), (std::int32_t) next.size()) != AGH_OK)
    {
      fail("agh_localize_batch_stage");
      return false;
    }
    return true;
  }

  /** agh_localize_batch_end: the one synchronisation and the results of the batch localizeBatchBegin queued, per capture as
   *  localizeBatch returns them. */
  bool localizeBatchEnd(std::vector<std::vector<agh_hypothesis> >& hands_out, std::vector<std::vector<agh_handle> >& handles_out,
    std::vector<std::vector<std::int32_t> >& inliers_out)
  {
    const std::size_t C = batch_captures_;
    hands_out.assign(C, std::vector<agh_hypothesis>());
    handles_out.assign(C, std::vector<agh_handle>());
    inliers_out.assign(C, std::vector<std::int32_t>());
    if (!ctx_)
      return false;
    const std::int64_t cap = batch_cap_, n_samples = batch_samples_;
    std::vector<agh_hypothesis> hands((std::size_t) cap);
    std::vector<agh_handle> handles((std::size_t) cap);
    std::vector<std::int32_t> inl((std::size_t) cap);
    std::vector<std::int32_t> samples((std::size_t) n_samples + 1);
    std::vector<agh_localize_batch_result> res(C + 1);
    batch_captures_ = 0;
    if (agh_localize_batch_end(ctx_, handles.data(), cap, inl.data(), cap, hands.data(), cap, samples.data(), res.data()) != AGH_OK)
    {
      fail("agh_localize_batch_end");
      return false;
    }
    searched_n_ = 0;
    for (std::size_t k = 0; k < C; k++)
    {
      const agh_localize_batch_result& r = res[k];
      hands_out[k].assign(hands.begin() + r.first_hand, hands.begin() + r.first_hand + r.r.n_hands);
      handles_out[k].assign(handles.begin() + r.first_handle, handles.begin() + r.first_handle + r.r.n_handles);
      inliers_out[k].assign(inl.begin() + r.first_inlier_idx, inl.begin() + r.first_inlier_idx + r.r.n_inlier_idx);
      searched_n_ += r.r.n_voxels;
    }
    last_samples_.assign(samples.begin(), samples.begin() + n_samples);
    return true;
  }

  /** Additional: camera origins per cloud of a batch (agh_set_cloud_cam_origins): row k = the translations of cams_left[k] /
   *  cams_right[k], as setCamTfLeft / setCamTfRight take them for the whole context.  Sticky until clearCloudCamOrigins.
   *  @return false (after printing) on error */
  bool setCloudCamOrigins(const std::vector<Matrix4d>& cams_left, const std::vector<Matrix4d>& cams_right)
  {
    if (cams_left.empty() || cams_left.size() != cams_right.size())
    {
      std::cout << " Error: setCloudCamOrigins needs one left and one right transform per cloud\n";
      return false;
    }
    if (!ensureContext())
      return false;
    std::vector<double> tab(cams_left.size() * 6);
    for (std::size_t k = 0; k < cams_left.size(); k++)
      for (int r = 0; r < 3; r++)
      {
        tab[k * 6 + (std::size_t) r] = mat4(cams_left[k], r, 3);
        tab[k * 6 + 3 + (std::size_t) r] = mat4(cams_right[k], r, 3);
      }
    if (agh_set_cloud_cam_origins(ctx_, tab.data(), (std::int32_t) cams_left.size()) != AGH_OK)
    {
      fail("agh_set_cloud_cam_origins");
      return false;
    }
    return true;
  }
  void clearCloudCamOrigins()
  {
    if (ctx_)
      (void) agh_set_cloud_cam_origins(ctx_, nullptr, 0);
  }

  /** Additional: the depth filter (agh_set_depth_filter) -- every later call of this search that back-projects depth images
   *  rejects flying pixels, speckles and readings outside [z_min, z_max] on the device.  Sticky until clearDepthFilter, also
   *  across a context this search re-creates (a changed hand geometry or device).  Refused while a chain is pending.
   *  @return false (after printing) on error; the filter held before stays in force */
  bool setDepthFilter(const agh_depth_filter_params& fp)
  {
    if (!ensureContext())
      return false;
    if (agh_set_depth_filter(ctx_, &fp) != AGH_OK)
    {
      fail("agh_set_depth_filter");
      return false;
    }
    depth_filter_ = fp;
    depth_filter_set_ = true;
    return true;
  }
  bool clearDepthFilter()
  {
    if (ctx_ && agh_set_depth_filter(ctx_, nullptr) != AGH_OK)
    {
      fail("agh_set_depth_filter");
      return false;
    }
    depth_filter_set_ = false;
    return true;
  }
  /** the filter held (agh_get_depth_filter); false: none */
  bool depthFilter(agh_depth_filter_params& out) const
  {
    if (depth_filter_set_)
      out = depth_filter_;
    return depth_filter_set_;
  }
  /** Additional: the voxel filter (agh_set_voxel_filter) -- every later call of this search that voxelises a capture (points
   *  or depth images, single or batch) prunes the voxels with fewer than min_neighbors occupied voxels of their own camera
   *  within `radius` voxels, on the device.  Sticky until clearVoxelFilter, also across a context this search re-creates.
   *  Refused while a chain is pending.
   *  @return false (after printing) on error; the filter held before stays in force */
  bool setVoxelFilter(const agh_voxel_filter_params& fp)
  {
    if (!ensureContext())
      return false;
    if (agh_set_voxel_filter(ctx_, &fp) != AGH_OK)
    {
      fail("agh_set_voxel_filter");
      return false;
    }
    voxel_filter_ = fp;
    voxel_filter_set_ = true;
    return true;
  }
  bool clearVoxelFilter()
  {
    if (ctx_ && agh_set_voxel_filter(ctx_, nullptr) != AGH_OK)
    {
      fail("agh_set_voxel_filter");
      return false;
    }
    voxel_filter_set_ = false;
    return true;
  }
  /** the filter held (agh_get_voxel_filter); false: none */
  bool voxelFilter(agh_voxel_filter_params& out) const
  {
    if (voxel_filter_set_)
      out = voxel_filter_;
    return voxel_filter_set_;
  }
  /** agh_get_voxel_filter_counts: per capture of the last voxelisation what the filter did; empty if that voxelisation ran
   *  without a filter, if there was none, or while a chain is pending */
  std::vector<agh_voxel_filter_counts> voxelFilterCounts()
  {
    std::vector<agh_voxel_filter_counts> out(64);
    const int n = ctx_ ? agh_get_voxel_filter_counts(ctx_, out.data(), (std::int32_t) out.size()) : 0;
    out.resize(n > 0 ? (std::size_t) n : 0);
    return out;
  }
  /** Additional: the hand filter (agh_set_hand_filter) -- every later localize chain of this search (points or depth images,
   *  single or batch) drops, on the device and ahead of the classifier, the hands outside an approach cone, outside the
   *  gripper's stroke, or with fingers in space no depth image saw (that criterion: the depth forms only; a points form then
   *  fails).  Sticky until clearHandFilter, also across a context this search re-creates.  Refused while a chain is pending.
   *  @return false (after printing) on error; the filter held before stays in force */
  bool setHandFilter(const agh_hand_filter_params& fp)
  {
    if (!ensureContext())
      return false;
    if (agh_set_hand_filter(ctx_, &fp) != AGH_OK)
    {
      fail("agh_set_hand_filter");
      return false;
    }
    hand_filter_ = fp;
    hand_filter_set_ = true;
    return true;
  }
  bool clearHandFilter()
  {
    if (ctx_ && agh_set_hand_filter(ctx_, nullptr) != AGH_OK)
    {
      fail("agh_set_hand_filter");
      return false;
    }
    hand_filter_set_ = false;
    return true;
  }
  /** the filter held (agh_get_hand_filter); false: none */
  bool handFilter(agh_hand_filter_params& out) const
  {
    if (hand_filter_set_)
      out = hand_filter_;
    return hand_filter_set_;
  }
  /** agh_get_hand_filter_counts: per list of the last chain collected (the call, a batch's captures, or the (capture, object)
   *  pairs, in the order of its results) what the filter did; empty if that chain ran without a filter, if there was none, or
   *  while a chain is pending */
  std::vector<agh_hand_filter_counts> handFilterCounts()
  {
    std::vector<agh_hand_filter_counts> out(64);
    const int n = ctx_ ? agh_get_hand_filter_counts(ctx_, out.data(), (std::int32_t) out.size()) : 0;
    out.resize(n > 0 ? (std::size_t) n : 0);
    return out;
  }
  /** Additional: the hand clearance (agh_set_hand_clearance) -- every later localize chain of this search (points or depth
   *  images, single or batch) drops, on the device, behind the hand filter and ahead of the classifier, the hands whose approach
   *  corridor (an oriented box behind the palm, swept backwards along the approach) holds more than max_points points of the
   *  capture's own voxelised cloud.  Sticky until clearHandClearance, also across a context this search re-creates.  Refused while
   *  a chain is pending.
   *  @return false (after printing) on error; the setting held before stays in force */
  bool setHandClearance(const agh_hand_clearance_params& cp)
  {
    if (!ensureContext())
      return false;
    if (agh_set_hand_clearance(ctx_, &cp) != AGH_OK)
    {
      fail("agh_set_hand_clearance");
      return false;
    }
    hand_clearance_ = cp;
    hand_clearance_set_ = true;
    return true;
  }
  bool clearHandClearance()
  {
    if (ctx_ && agh_set_hand_clearance(ctx_, nullptr) != AGH_OK)
    {
      fail("agh_set_hand_clearance");
      return false;
    }
    hand_clearance_set_ = false;
    return true;
  }
  /** the clearance held (agh_get_hand_clearance); false: none */
  bool handClearance(agh_hand_clearance_params& out) const
  {
    if (hand_clearance_set_)
      out = hand_clearance_;
    return hand_clearance_set_;
  }
  /** agh_get_hand_clearance_counts: per list of the last chain collected (the call, a batch's captures, or the (capture, object)
   *  pairs, in the order of its results) what the clearance did; empty if that chain ran without one, if there was none, or
   *  while a chain is pending */
  std::vector<agh_hand_clearance_counts> handClearanceCounts()
  {
    std::vector<agh_hand_clearance_counts> out(64);
    const int n = ctx_ ? agh_get_hand_clearance_counts(ctx_, out.data(), (std::int32_t) out.size()) : 0;
    out.resize(n > 0 ? (std::size_t) n : 0);
    return out;
  }
  /** Additional: the handle ranking (agh_set_handle_ranking) -- every later localize chain of this search (points or depth
   *  images, single or batch) returns each list's handles in rank order: score descending (support, classifier margin, approach,
   *  position, distance, width and length under the record's weights), ties by the order of discovery, the handles below
   *  min_score left out, at most max_handles per list.  Sticky until clearHandleRanking, also across a context this search
   *  re-creates.  Refused while a chain is pending.
   *  @return false (after printing) on error; the setting held before stays in force */
  bool setHandleRanking(const agh_handle_ranking_params& rp)
  {
    if (!ensureContext())
      return false;
    if (agh_set_handle_ranking(ctx_, &rp) != AGH_OK)
    {
      fail("agh_set_handle_ranking");
      return false;
    }
    handle_ranking_ = rp;
    handle_ranking_set_ = true;
    return true;
  }
  bool clearHandleRanking()
  {
    if (ctx_ && agh_set_handle_ranking(ctx_, nullptr) != AGH_OK)
    {
      fail("agh_set_handle_ranking");
      return false;
    }
    handle_ranking_set_ = false;
    return true;
  }
  /** the ranking held (agh_get_handle_ranking); false: none */
  bool handleRanking(agh_handle_ranking_params& out) const
  {
    if (handle_ranking_set_)
      out = handle_ranking_;
    return handle_ranking_set_;
  }
  /** agh_get_handle_scores: the score record of every handle the last chain collected returned, laid out as its handles (all
   *  lists, list after list); empty if that chain ran without a ranking, if there was none, or while a chain is pending */
  std::vector<agh_handle_score> handleScores()
  {
    std::vector<agh_handle_score> out(8192);
    int n = ctx_ ? agh_get_handle_scores(ctx_, out.data(), (std::int64_t) out.size()) : 0;
    if (n == AGH_ERR_CAPACITY)  // (several full lists)
    {
      out.resize((std::size_t) 8192 * 64);
      n = agh_get_handle_scores(ctx_, out.data(), (std::int64_t) out.size());
    }
    out.resize(n > 0 ? (std::size_t) n : 0);
    return out;
  }
  /** agh_get_handle_ranking_counts: per list of the last chain collected how many handles were found, left out by min_score and
   *  returned; empty as handleScores */
  std::vector<agh_handle_ranking_counts> handleRankingCounts()
  {
    std::vector<agh_handle_ranking_counts> out(64);
    const int n = ctx_ ? agh_get_handle_ranking_counts(ctx_, out.data(), (std::int32_t) out.size()) : 0;
    out.resize(n > 0 ? (std::size_t) n : 0);
    return out;
  }
  /** agh_get_hand_margins: the classifier margin (minus its decision sum; 0 without a classifier) of every hand the last chain's
   *  handle search ran on, laid out as the hands; empty as handleScores */
  std::vector<double> handMargins()
  {
    std::vector<double> out(8192);
    int n = ctx_ ? agh_get_hand_margins(ctx_, out.data(), (std::int64_t) out.size()) : 0;
    if (n == AGH_ERR_CAPACITY)
    {
      out.resize((std::size_t) 8192 * 64);
      n = agh_get_hand_margins(ctx_, out.data(), (std::int64_t) out.size());
    }
    out.resize(n > 0 ? (std::size_t) n : 0);
    return out;
  }
  /** agh_get_depth_filter_counts: per view of the last deprojection, in launch order, what the filter did; empty if that
   *  deprojection ran without a filter, if there was none, or while a chain is pending */
  std::vector<agh_depth_filter_counts> depthFilterCounts()
  {
    std::vector<agh_depth_filter_counts> out(128);
    const int n = ctx_ ? agh_get_depth_filter_counts(ctx_, out.data(), (std::int32_t) out.size()) : 0;
    out.resize(n > 0 ? (std::size_t) n : 0);
    return out;
  }

  /** Additional: a burst of depth frames of ONE fixed camera fused on the device (agh_fuse_depth, include/agh.h "DEPTH FUSION"):
   *  1 to 16 frames, equal in everything but the pixels and the row stride, into slot `slot` (0 .. 127) of this search's
   *  context.  A frame without a pose takes the transform of camera `camera` (0: left, 1: right).  The call is queued, not
   *  waited for; *fused_out receives the fused image's record, whose data is a DEVICE pointer (the C ABI's _device calls take
   *  it).  This adapter's depth chains take host images: fusedDepth brings the image back for them.  Refused while a chain is
   *  pending; the slots do not survive a context this search re-creates (a changed hand geometry or device).
   *  @return false (after printing) on error; the slot's previous image is untouched */
  bool fuseDepth(const std::vector<DepthImage>& frames, const agh_depth_fusion_params& fp, int slot = 0, int camera = 0,
    agh_depth_image* fused_out = nullptr)
  {
    if (!ensureContext())
      return false;
    std::vector<DepthImage> burst(frames);
    for (std::size_t t = 0; t < burst.size(); t++)
      if (!burst[t].has_pose)
      {
        burst[t].pose = camera == 0 ? cam_tf_left_ : cam_tf_right_;
        burst[t].has_pose = true;
      }
    const std::vector<agh_depth_image> recs = depthRecords(burst);
    agh_depth_image fused;
    if (agh_fuse_depth(ctx_, recs.empty() ? nullptr : recs.data(), (std::int32_t) recs.size(), &fp, (std::int32_t) slot, &fused) != AGH_OK)
    {
      fail("agh_fuse_depth");
      return false;
    }
    if (fused_out)
      *fused_out = fused;
    return true;
  }
  /** agh_get_depth_fusion_counts: what the slot's last fuse did; false if the slot was never fused, or while a chain is pending */
  bool depthFusionCounts(int slot, agh_depth_fusion_counts& out)
  {
    return ctx_ && agh_get_depth_fusion_counts(ctx_, (std::int32_t) slot, &out) == 1;
  }
  /** agh_get_fused_depth: the slot's fused image into `pixels` (rows tight), and `image` describing it over those bytes with its
   *  own pose -- what localizeDepth* and Localization::localizeHandlesDepth take.  Keep `pixels` alive and unchanged as long as
   *  `image` is used.  false if the slot was never fused, or while a chain is pending */
  bool fusedDepth(int slot, std::vector<std::uint8_t>& pixels, DepthImage& image)
  {
    agh_depth_fusion_counts counts;
    if (!depthFusionCounts(slot, counts))
      return false;
    pixels.resize((std::size_t) counts.n_pixels * 4);  // (enough for either format)
    agh_depth_image rec;
    const int got = agh_get_fused_depth(ctx_, (std::int32_t) slot, pixels.data(), (std::int64_t) pixels.size(), &rec);
    if (got <= 0)
    {
      if (got < 0)
        fail("agh_get_fused_depth");
      return false;
    }
    pixels.resize((std::size_t) got);
    image = DepthImage();
    image.data = pixels.data();
    image.width = rec.width;
    image.height = rec.height;
    image.row_stride_bytes = rec.row_stride_bytes;
    image.is_float = rec.format == AGH_DEPTH_F32;
    image.depth_scale = rec.depth_scale;
    image.fx = rec.fx;
    image.fy = rec.fy;
    image.cx = rec.cx;
    image.cy = rec.cy;
    image.has_pose = true;
    image.pose = cam_tf_left_;  // (the last row of a transform; the three above it are the record's)
    for (int row = 0; row < 3; row++)
      for (int col = 0; col < 4; col++)
        image.pose(row, col) = rec.pose[4 * row + col];
    return true;
  }

  /** agh_localize_stage: the NEXT capture up, beside the chain in flight (keep `next` alive and unchanged until the
   *  localizeEnd of the chain that searches it has returned). */
  bool localizeStage(const PointCloud::Ptr& next)
  {
    if (!ensureContext() || !next)
      return false;
    const RawPoints in = rawPoints(*next);
    if (agh_localize_stage(ctx_, in.xyz, in.stride, in.n) != AGH_OK)
    {
      fail("agh_localize_stage");
      return false;
    }
    return true;
  }

  bool localizeEnd(std::vector<agh_hypothesis>& hands_out, std::vector<agh_handle>& handles_out, std::vector<std::int32_t>& inliers_out)
  {
    hands_out.clear();
    handles_out.clear();
    inliers_out.clear();
    if (!ctx_)
      return false;
    const std::int64_t cap = loc_cap_;
    hands_out.resize((std::size_t) cap);
    handles_out.resize((std::size_t) cap);
    inliers_out.resize((std::size_t) cap);
    agh_localize_result res;
    const int rc = agh_localize_end(ctx_, handles_out.data(), cap, inliers_out.data(), cap, hands_out.data(), cap,
      last_samples_.empty() ? nullptr : last_samples_.data(), &res);
    if (rc != AGH_OK)
    {
      hands_out.clear();
      handles_out.clear();
      inliers_out.clear();
      fail("agh_localize");
      return false;
    }
    hands_out.resize((std::size_t) res.n_hands);
    handles_out.resize((std::size_t) res.n_handles);
    inliers_out.resize((std::size_t) res.n_inlier_idx);
    searched_n_ = res.n_voxels;
    return true;
  }

  /** hand_search.cpp:31-62 on the cloud the context already holds (after findHands' upload or preprocess). */
  std::vector<GraspHypothesis> findHandsInSearchedCloud(const std::vector<int>& indices, bool calculates_antipodal)
  {
    std::vector<GraspHypothesis> hand_list;
    if (!ctx_)
      return hand_list;
    const std::int64_t n = (std::int64_t) agh_get_cloud(ctx_, nullptr, nullptr, 0);
    if (n <= 0)
    {
      std::cout << "Input cloud is empty!\n";
      return hand_list;
    }
    std::vector<std::int32_t> idx;
    if (indices.empty())
    {
      std::cout << "Generating uniform random indices ...\n";  // hand_search.cpp:34
      idx = randomSample(n, num_samples_, (unsigned) sampleSeed());
    }
    else
      idx.assign(indices.begin(), indices.end());
    last_samples_ = idx;
    if (calculates_antipodal)
      std::cout << "Calculating normals for all points\n";  // hand_search.cpp:19
    std::cout << "Estimating local axes ...\nFinding hand poses ...\n";  // hand_search.cpp:52,58
    const bool training = keeps_training_images_ && calculates_antipodal;
    if (agh_set_training_images(ctx_, training ? 1 : 0) != AGH_OK)
      return fail("agh_set_training_images");
    std::vector<agh_hypothesis> out(8 * idx.size() + 1);
    std::int64_t n_out = 0;
    const int rc = sharded_
      ? agh_find_hands_sharded(ctx_, idx.data(), (std::int64_t) idx.size(), calculates_antipodal ? 1 : 0, out.data(),
          (std::int64_t) out.size(), &n_out)
      : agh_find_hands(ctx_, idx.data(), (std::int64_t) idx.size(), calculates_antipodal ? 1 : 0, out.data(),
          (std::int64_t) out.size(), &n_out);
    if (rc != AGH_OK)
      return fail(sharded_ ? "agh_find_hands_sharded" : "agh_find_hands");
    if (sharded_)
    {
      // every rank holds the complete list; the device-side state (images, points) of a hypothesis lives on the rank that
      // searched its sample, so the hypotheses carry no image here and Learning::classify goes through the collective
      // agh_classify_sharded (see learning.h)
      // The records of THIS rank's samples (a contiguous run of the merged list: slices are contiguous and the list is
      // sample-major) keep their position in this rank's own device-side list, so getPointsForLearning() and the index
      // getters work for them; the others say that their points live on another rank.
      std::int32_t rank = 0, n_ranks = 1;
      std::int64_t lo = 0, hi = 0;
      agh_comm_rank(ctx_, &rank, &n_ranks);
      agh_shard_slice((std::int64_t) idx.size(), rank, n_ranks, &lo, &hi);
      std::int64_t first = 0;
      while (first < n_out && out[(std::size_t) first].sample < lo)
        first++;
      hand_list.reserve((std::size_t) n_out);
      for (std::int64_t i = 0; i < n_out; i++)
      {
        const std::int64_t smp = out[(std::size_t) i].sample;
        hand_list.push_back(GraspHypothesis(out[(std::size_t) i], (long) i, link_, (smp >= lo && smp < hi) ? (long) (i - first) : -1L));
      }
      std::cout << " Found " << hand_list.size() << " robot hand poses\n";
      return hand_list;
    }
    hand_list.reserve((std::size_t) n_out);
    for (std::int64_t i = 0; i < n_out; i++)
      hand_list.push_back(GraspHypothesis(out[(std::size_t) i], (long) i, link_));
    if (keeps_images_ && n_out > 0)
    {
      std::shared_ptr<std::vector<std::uint32_t> > block(new std::vector<std::uint32_t>((std::size_t) n_out * 250));
      if (agh_get_packed_images(ctx_, block->data(), n_out) != (int) n_out)
        return fail("agh_get_packed_images");
      for (std::int64_t i = 0; i < n_out; i++)
        hand_list[(std::size_t) i].setImage(block, (std::size_t) i * 250);
    }
    if (training && n_out > 0)
    {
      std::shared_ptr<std::vector<std::uint32_t> > block(new std::vector<std::uint32_t>((std::size_t) n_out * 750));
      if (agh_get_training_images(ctx_, block->data(), n_out) != (int) n_out)
        return fail("agh_get_training_images");
      for (std::int64_t i = 0; i < n_out; i++)
        hand_list[(std::size_t) i].setTrainingImages(block, (std::size_t) i * 750);
    }
    std::cout << " Found " << hand_list.size() << " robot hand poses\n";  // hand_search.cpp:203
    return hand_list;
  }

private:
  // the sample seed of a draw: setSampleSeed's, else the clock like pcl::RandomSample
  std::uint64_t sampleSeed() const { return sample_seed_set_ ? sample_seed_ : (std::uint64_t) std::time(nullptr); }

  // room for the hands (and so the handles and inlier indices) a chain over n_samples samples can return
  static std::int64_t handsRoom(std::int64_t n_samples) { return n_samples * 8 < 8192 ? n_samples * 8 : 8192; }

  // the one place that fills the library's chain record.  `idx`: the explicit samples (the library's begin copies them, so
  // they only have to outlive that call); empty: num_samples_ indices drawn on the device with `seed`
  agh_localize_params chainParams(std::int64_t size_left, bool dense, const VectorXd& workspace, double cell_size,
    const std::vector<std::int32_t>& idx, std::uint64_t seed, int min_inliers, double min_length, bool filters_boundaries) const
  {
    agh_localize_params lp;
    lp.size_left = size_left;
    lp.dense = dense ? 1 : 0;
    lp.classify = 1;
    for (int i = 0; i < 6; i++)
      lp.workspace[i] = workspace(i);
    lp.cell_size = cell_size;
    lp.sample_idx = idx.empty() ? nullptr : idx.data();
    lp.n_samples = idx.empty() ? (std::int64_t) (num_samples_ < 0 ? 0 : num_samples_) : (std::int64_t) idx.size();
    lp.sample_seed = seed;
    lp.min_inliers = min_inliers;
    lp.filters_boundaries = filters_boundaries ? 1 : 0;
    lp.min_length = min_length;
    return lp;
  }

  // a single-capture chain is queued: what localizeEnd reads for it
  void chainBegun(std::int64_t n_samples)
  {
    loc_cap_ = handsRoom(n_samples) + 1;
    last_samples_.assign((std::size_t) n_samples, 0);
  }

  // the output buffers of a labelled call (the library refuses an n_objects outside 1 .. 64: room for one then), and their
  // spans per object
  struct LabeledOutputs
  {
    std::size_t K;
    std::int64_t n_samples, cap;
    std::vector<agh_hypothesis> hands;
    std::vector<agh_handle> handles;
    std::vector<std::int32_t> inl, samples;
    std::vector<agh_localize_batch_result> res;
    LabeledOutputs(int n_objects, std::int64_t S)
      : K(n_objects >= 1 && n_objects <= 64 ? (std::size_t) n_objects : 1), n_samples(S), cap((std::int64_t) K * handsRoom(S) + 1),
        hands((std::size_t) cap), handles((std::size_t) cap), inl((std::size_t) cap), samples(K * (std::size_t) S + 1), res(K + 1)
    {
    }
  };
  static void labeledClear(int n_objects, std::vector<std::vector<agh_hypothesis> >& hands_out,
    std::vector<std::vector<agh_handle> >& handles_out, std::vector<std::vector<std::int32_t> >& inliers_out)
  {
    const std::size_t K = n_objects >= 1 && n_objects <= 64 ? (std::size_t) n_objects : 0;
    hands_out.assign(K, std::vector<agh_hypothesis>());
    handles_out.assign(K, std::vector<agh_handle>());
    inliers_out.assign(K, std::vector<std::int32_t>());
  }
  // what localizeBatchEnd needs for the labelled batch just queued: a list per (capture, object), n_samples each
  void labeledBatchQueued(const std::vector<int>& n_objects, const std::vector<agh_localize_params>& lp)
  {
    std::size_t lists = 0;
    std::int64_t cap = 1, n_samples = 0;
    for (std::size_t k = 0; k < n_objects.size(); k++)
    {
      lists += (std::size_t) n_objects[k];
      cap += (std::int64_t) n_objects[k] * handsRoom(lp[k].n_samples);
      n_samples += (std::int64_t) n_objects[k] * lp[k].n_samples;
    }
    batch_captures_ = lists;
    batch_cap_ = cap;
    batch_samples_ = n_samples;
    batch_objects_ = n_objects;
  }
  void labeledCollect(const LabeledOutputs& o, std::vector<std::vector<agh_hypothesis> >& hands_out,
    std::vector<std::vector<agh_handle> >& handles_out, std::vector<std::vector<std::int32_t> >& inliers_out)
  {
    for (std::size_t k = 0; k < o.K; k++)
    {
      const agh_localize_batch_result& r = o.res[k];
      hands_out[k].assign(o.hands.begin() + r.first_hand, o.hands.begin() + r.first_hand + r.r.n_hands);
      handles_out[k].assign(o.handles.begin() + r.first_handle, o.handles.begin() + r.first_handle + r.r.n_handles);
      inliers_out[k].assign(o.inl.begin() + r.first_inlier_idx, o.inl.begin() + r.first_inlier_idx + r.r.n_inlier_idx);
    }
    searched_n_ = o.res[0].r.n_voxels;  // (one cloud, whose voxel count every object reports)
    last_samples_.assign(o.samples.begin(), o.samples.begin() + (std::ptrdiff_t) (o.K * (std::size_t) o.n_samples));
  }

  // a host cloud as the library takes it: no pointer for an empty one
  struct RawPoints
  {
    const float* xyz;
    std::int64_t stride, n;
  };
  static RawPoints rawPoints(const PointCloud& cloud)
  {
    RawPoints r;
    r.n = (std::int64_t) cloud.size();
    r.xyz = r.n > 0 ? &cloud.points[0].x : nullptr;
    r.stride = (std::int64_t) sizeof(cloud.points[0]);
    return r;
  }
  struct RawBatch
  {
    std::vector<const float*> xyz;
    std::vector<std::int64_t> stride, n;
  };
  static bool rawPoints(const std::vector<PointCloud::Ptr>& clouds, RawBatch& out)  // false: a cloud is missing
  {
    for (std::size_t k = 0; k < clouds.size(); k++)
    {
      if (!clouds[k])
        return false;
      const RawPoints r = rawPoints(*clouds[k]);
      out.xyz.push_back(r.xyz);
      out.stride.push_back(r.stride);
      out.n.push_back(r.n);
    }
    return true;
  }

  // the cloud the context holds (n points) as a host cloud with its camera ids; it is the searched cloud from here on
  bool readBackCloud(std::int64_t n, PointCloud::Ptr& cloud_out, VectorXi& pts_cam_source_out)
  {
    std::vector<float> xyz(3 * (std::size_t) n + 3);
    std::vector<std::int32_t> cam((std::size_t) n + 1);
    if (agh_get_cloud(ctx_, xyz.data(), cam.data(), n) < 0)
    {
      fail("agh_get_cloud");
      return false;
    }
    cloud_out.reset(new PointCloud);
    cloud_out->points.resize((std::size_t) n);
    pts_cam_source_out = VectorXi((std::size_t) n);
    for (std::int64_t i = 0; i < n; i++)
    {
      cloud_out->points[(std::size_t) i].x = xyz[3 * (std::size_t) i];
      cloud_out->points[(std::size_t) i].y = xyz[3 * (std::size_t) i + 1];
      cloud_out->points[(std::size_t) i].z = xyz[3 * (std::size_t) i + 2];
      pts_cam_source_out((std::size_t) i) = cam[(std::size_t) i];
    }
    searched_n_ = n;
    return true;
  }

  // the ABI's records of the images (the library checks them, and their number)
  std::vector<agh_depth_image> depthRecords(const std::vector<DepthImage>& images) const
  {
    std::vector<agh_depth_image> recs(images.size());
    for (std::size_t k = 0; k < images.size(); k++)
    {
      const DepthImage& im = images[k];
      agh_depth_image& r = recs[k];
      r.data = im.data;
      r.width = (std::int32_t) im.width;
      r.height = (std::int32_t) im.height;
      r.row_stride_bytes = im.row_stride_bytes;
      r.format = im.is_float ? AGH_DEPTH_F32 : AGH_DEPTH_U16;
      r.depth_scale = im.depth_scale;
      r.fx = im.fx;
      r.fy = im.fy;
      r.cx = im.cx;
      r.cy = im.cy;
      const Matrix4d& tf = im.has_pose ? im.pose : (k == 0 ? cam_tf_left_ : cam_tf_right_);
      for (int row = 0; row < 3; row++)
        for (int col = 0; col < 4; col++)
          r.pose[4 * row + col] = mat4(tf, row, col);
    }
    return recs;
  }

  std::vector<GraspHypothesis> fail(const char* what)
  {
    std::cout << " Error in " << what << ": " << agh_last_error(ctx_) << "\n";
    return std::vector<GraspHypothesis>();
  }

  bool ensureContext()
  {
    if (ctx_ && !dirty_)
      return true;
    link_->ctx = nullptr;  // hypotheses of the old context are cut loose
    link_.reset(new detail::SearchLink);
    agh_destroy(ctx_);
    ctx_ = nullptr;
    for (int r = 0; r < 3; r++)
    {
      params_.cam_origin[0][r] = mat4(cam_tf_left_, r, 3);   // hand_search.cpp:72-74 -> quadric.cpp:8-11
      params_.cam_origin[1][r] = mat4(cam_tf_right_, r, 3);
    }
    params_.normals_mode = deterministic_ ? AGH_NORMALS_DETERMINISTIC : AGH_NORMALS_RAND50;
    params_.device = device_;
    const int rc = agh_create(&params_, &ctx_);
    if (rc != AGH_OK)
    {
      std::cout << " Error: cannot create the MI355X grasp-search context: " << agh_last_error(nullptr) << "\n";
      ctx_ = nullptr;
      return false;
    }
    dirty_ = false;
    link_->ctx = ctx_;
    if (depth_filter_set_ && agh_set_depth_filter(ctx_, &depth_filter_) != AGH_OK)  // (the setting follows the search, not the context)
    {
      fail("agh_set_depth_filter");
      return false;
    }
    if (voxel_filter_set_ && agh_set_voxel_filter(ctx_, &voxel_filter_) != AGH_OK)
    {
      fail("agh_set_voxel_filter");
      return false;
    }
    if (hand_filter_set_ && agh_set_hand_filter(ctx_, &hand_filter_) != AGH_OK)
    {
      fail("agh_set_hand_filter");
      return false;
    }
    if (hand_clearance_set_ && agh_set_hand_clearance(ctx_, &hand_clearance_) != AGH_OK)
    {
      fail("agh_set_hand_clearance");
      return false;
    }
    if (handle_ranking_set_ && agh_set_handle_ranking(ctx_, &handle_ranking_) != AGH_OK)
    {
      fail("agh_set_handle_ranking");
      return false;
    }
    return true;
  }

  agh_ctx* ctx_;
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
  std::int64_t searched_n_ = 0;
  // What an End reads of the chain in flight.  The rule for every Begin: these (and last_samples_, sized by chainBegun for
  // localizeEnd) are written only after the library's begin has returned AGH_OK, so a Begin that fails for any reason -- a
  // chain in flight included -- leaves that chain's End what it needs.
  std::int64_t loc_cap_ = 1;  // room for the results of the chain localizeBegin / localizeDepthBegin queued
  std::size_t batch_captures_ = 0;  // ... and of the batch localizeBatchBegin queued: its captures, room, samples
  std::vector<int> batch_objects_;  // a labelled batch: the objects per capture (batch_captures_ then counts its LISTS)
  std::int64_t batch_cap_ = 1, batch_samples_ = 0;
  agh_params params_;
  Matrix4d cam_tf_left_, cam_tf_right_;
  int num_threads_, num_samples_;
  bool plots_hands_, deterministic_;
  std::uint64_t sample_seed_;
  bool sample_seed_set_ = false;
  std::vector<std::int32_t> last_samples_;
  int device_;
  bool dirty_;
  bool keeps_training_images_ = false;
  bool keeps_images_ = true;
  bool sharded_ = false;
  std::shared_ptr<detail::SearchLink> link_;
};

namespace detail
{
/** A device context for work that follows a search (classification, training, handle search) when the caller -- like the
 *  reference's Learning(int) and HandleSearch() -- names none: the given search's, else one a hypothesis of the list
 *  still links to, else a context of the finder's own (created on first use with default parameters). */
class ContextFinder
{
public:
  agh_ctx* find(HandSearch* search, const std::vector<GraspHypothesis>& hands_list)
  {
    if (search && search->context())
      return search->context();
    for (std::size_t i = 0; i < hands_list.size(); i++)
      if (hands_list[i].getAnyContext())
        return hands_list[i].getAnyContext();
    if (!own_)
    {
      agh_params p;
      agh_default_params(&p);
      agh_ctx* c = nullptr;
      if (agh_create(&p, &c) != AGH_OK)
      {
        std::cout << " Error: cannot create the MI355X grasp-search context: " << agh_last_error(nullptr) << "\n";
        return nullptr;
      }
      own_.reset(c, agh_destroy);
    }
    return own_.get();
  }

private:
  std::shared_ptr<agh_ctx> own_;
};
}  // namespace detail

}  // namespace agile_grasp_amd
#endif
