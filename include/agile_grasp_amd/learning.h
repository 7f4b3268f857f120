// learning.h -- Learning (include/agile_grasp/learning.h:57-205).
//
// Prediction (learning.h:122-123, learning.cpp:165-247): classify(hands_list, svm_filename, cam_pos) keeps the
// hypotheses the SVM labels antipodal.
//
// Training (learning.h:87-113, 180-182; learning.cpp:3-163, 249-318): train / trainBalanced select the instances exactly
// as the reference does (three per hand: all points, camera 0's, camera 1's; std::rand() for the max_positive draws and
// the negatives of trainBalanced) and convertData turns them into HOG descriptors, runs CvSVM::train's solver and writes
// CvSVM::save's file -- all three on the GPU through agh_train_svm.  Like the reference, train* call convertData with
// its default uses_linear_kernel = false, i.e. the quadratic kernel; pass true for the shipped model's linear shape.
// The hands must come from a HandSearch with setKeepsTrainingImages(true) and calculates_antipodal = true.
//
// classify is stateless like the reference's: every hypothesis carries its packed 80x100 occupancy image (what
// convertToImage builds from points_for_learning_; rasterised by the hand sweep, attached by HandSearch), so any list --
// filtered, re-ordered, accumulated over several clouds or searches -- can be classified at any later time.  When the
// whole list belongs to the most recent findHands of one live search, the images that search left on the GPU are used
// directly (no upload).  cam_pos is accepted for signature compatibility: the images were rasterised with the camera
// origins the search holds (localization.cpp:147-150 passes the same two).
#ifndef AGILE_GRASP_AMD_LEARNING_H
#define AGILE_GRASP_AMD_LEARNING_H

#include <cstdlib>
#include <iostream>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../agh.h"
#include "grasp_hypothesis.h"
#include "hand_search.h"

namespace agile_grasp_amd
{

class Learning
{
public:
  Learning() : search_(nullptr), num_threads_(1) {}                                 // learning.h:64-67
  explicit Learning(int num_threads) : search_(nullptr), num_threads_(num_threads) {}  // learning.h:73-76
  /** Additional: work on the device context of `search` instead of finding one through the hypotheses. */
  explicit Learning(HandSearch& search, int num_threads = 1) : search_(&search), num_threads_(num_threads) {}

  std::vector<GraspHypothesis> classify(const std::vector<GraspHypothesis>& hands_list, const std::string& svm_filename,
    const Matrix3Xd& cam_pos, bool is_plotting = false)
  {
    (void) cam_pos;
    (void) is_plotting;
    (void) num_threads_;
    std::cout << "Predicting ...\n";
    std::vector<GraspHypothesis> antipodal_hands;
    if (!detail::svmFileExists(svm_filename))
      return antipodal_hands;
    agh_ctx* ctx = contextFor(hands_list);
    if (!ctx || !detail::loadSvm(ctx, svm_filename))
      return antipodal_hands;
    const std::size_t n = hands_list.size();
    std::vector<unsigned char> keep_of(n, 0);  // per list entry
    // the list of a sharded findHands (HandSearch::joinCommunicator)?  Then classify is a COLLECTIVE like that search was:
    // each rank scores the hypotheses of its own samples, the labels travel with a second all-gather of the lists
    std::int64_t n_merged = -1;
    bool sharded_now = n > 0 && agh_comm_last_count(ctx, &n_merged) == AGH_OK && n_merged >= 0;
    for (std::size_t i = 0; i < n && sharded_now; i++)
      sharded_now = hands_list[i].getContextAtEpoch() == ctx && hands_list[i].getDeviceIndex() < n_merged;
    if (sharded_now)
    {
      std::vector<unsigned char> keep((std::size_t) n_merged + 1, 0);
      std::int64_t n_kept = 0;
      if (agh_classify_sharded(ctx, nullptr, keep.data(), (std::int64_t) keep.size(), &n_kept) != AGH_OK)
      {
        std::cout << " Error: " << agh_last_error(ctx) << "\n";
        return antipodal_hands;
      }
      for (std::size_t i = 0; i < n; i++)
        keep_of[i] = keep[(std::size_t) hands_list[i].getDeviceIndex()];
    }
    bool all_live = n > 0 && !sharded_now;
    for (std::size_t i = 0; i < n && all_live; i++)
      all_live = hands_list[i].getLiveContext() == ctx;
    if (all_live)
    {
      // the list is (a subset of) the most recent findHands of this context: its images are still on the device
      std::int32_t epoch = 0;
      std::int64_t n_dev = 0, n_kept = 0;
      if (agh_get_epoch(ctx, &epoch, &n_dev) != AGH_OK || n_dev < 0)
      {
        std::cout << " Error: " << agh_last_error(ctx) << "\n";
        return antipodal_hands;
      }
      std::vector<unsigned char> keep((std::size_t) n_dev + 1, 0);
      if (agh_classify(ctx, keep.data(), (std::int64_t) keep.size(), &n_kept) != AGH_OK)
      {
        std::cout << " Error: " << agh_last_error(ctx) << "\n";
        return antipodal_hands;
      }
      for (std::size_t i = 0; i < n; i++)
        keep_of[i] = keep[(std::size_t) hands_list[i].getDeviceIndex()];
    }
    else if (n > 0 && !sharded_now)
    {
      std::vector<std::uint32_t> images(n * 250);
      for (std::size_t i = 0; i < n; i++)
      {
        const std::uint32_t* im = hands_list[i].getImage();
        if (!im)
        {
          std::cout << " Error: hypothesis " << i << " carries no occupancy image and its search has moved on "
                       "(HandSearch::setKeepsImages(false), or a hand-made hypothesis)\n";
          return antipodal_hands;
        }
        for (int w = 0; w < 250; w++)
          images[i * 250 + (std::size_t) w] = im[w];
      }
      if (agh_classify_images(ctx, images.data(), (std::int64_t) n, keep_of.data(), nullptr) != AGH_OK)
      {
        std::cout << " Error: " << agh_last_error(ctx) << "\n";
        return antipodal_hands;
      }
    }
    for (std::size_t i = 0; i < n; i++)  // input order preserved (learning.cpp:236-243)
      if (keep_of[i])
      {
        antipodal_hands.push_back(hands_list[i]);
        antipodal_hands.back().setFullAntipodal(true);
      }
    std::cout << " " << antipodal_hands.size() << " antipodal grasps found.\n";
    return antipodal_hands;
  }

  /** learning.h:130-136: what convertToImage needs of a hand -- here the rasterised image itself. */
  struct Instance
  {
    const std::uint32_t* image;  // 250 packed words (80 x 100 pixels)
    bool label;
  };

  /** learning.cpp:375-400.  cam_pos is implied by the search (the image was rasterised with its camera origins). */
  Instance createInstance(const GraspHypothesis& h, const Matrix3Xd& cam_pos, int cam = -1) const
  {
    (void) cam_pos;
    Instance ins;
    ins.image = h.getTrainingImage(cam);
    ins.label = h.isFullAntipodal();
    return ins;
  }

  /** learning.cpp:3-74 */
  void trainBalanced(const std::vector<GraspHypothesis>& hands_list, const std::vector<int>& sizes,
    const std::string& file_name, const Matrix3Xd& cam_pos, int max_positive = 1000000000, bool is_plotting = false)
  {
    std::vector<int> positives, negatives, indices_selected, positives_sub;
    std::size_t k = 0;
    for (int i = 0; i < (int) hands_list.size(); i++)
    {
      if (hands_list[(std::size_t) i].isFullAntipodal())
        positives_sub.push_back(i);
      else if (!hands_list[(std::size_t) i].isHalfAntipodal())
        negatives.push_back(i);
      if (k < sizes.size() && i == sizes[k])
      {
        selectPositives(positives_sub, max_positive, positives);
        positives_sub.resize(0);
        k++;
      }
    }
    indices_selected.insert(indices_selected.end(), positives.begin(), positives.end());
    std::set<int> indices;
    while (!negatives.empty() && indices.size() < positives.size() && indices.size() < negatives.size())
      indices.insert(indices.end(), std::rand() % (int) negatives.size());
    for (std::set<int>::iterator it = indices.begin(); it != indices.end(); it++)
      indices_selected.push_back(negatives[(std::size_t) *it]);
    std::cout << "size(positives): " << positives.size() << std::endl;
    std::cout << "indices_selected.size: " << indices_selected.size() << std::endl;
    std::vector<Instance> instances;
    for (std::size_t i = 0; i < indices_selected.size(); i++)
      pushInstances(hands_list[(std::size_t) indices_selected[i]], cam_pos, instances);
    std::cout << "Converting " << instances.size() << " training examples (grasps) to images\n";
    hint_ctx_ = anyContextOf(hands_list);
    convertData(instances, file_name, is_plotting);
    hint_ctx_ = nullptr;
  }

  /** learning.cpp:76-141 */
  void train(const std::vector<GraspHypothesis>& hands_list, const std::vector<int>& sizes, const std::string& file_name,
    const Matrix3Xd& cam_pos, int max_positive = 1000000000, bool is_plotting = false)
  {
    std::vector<int> positives, chosen;
    std::vector<Instance> instances;
    std::size_t k = 0;
    for (int i = 0; i < (int) hands_list.size(); i++)
    {
      const GraspHypothesis& h = hands_list[(std::size_t) i];
      if (h.isFullAntipodal())
        positives.push_back(i);
      else if (!h.isHalfAntipodal())
        pushInstances(h, cam_pos, instances);
      if (k < sizes.size() && i == sizes[k])
      {
        chosen.clear();
        selectPositives(positives, max_positive, chosen);
        for (std::size_t j = 0; j < chosen.size(); j++)
          pushInstances(hands_list[(std::size_t) chosen[j]], cam_pos, instances);
        positives.resize(0);
        k++;
      }
    }
    std::cout << "Converting " << instances.size() << " training examples (grasps) to images\n";
    hint_ctx_ = anyContextOf(hands_list);
    convertData(instances, file_name, is_plotting);
    hint_ctx_ = nullptr;
  }

  /** learning.cpp:143-163 */
  void train(const std::vector<GraspHypothesis>& hands_list, const std::string& file_name, const Matrix3Xd& cam_pos,
    bool is_plotting = false)
  {
    std::vector<Instance> instances;
    for (std::size_t i = 0; i < hands_list.size(); i++)
      if (!hands_list[i].isHalfAntipodal() || hands_list[i].isFullAntipodal())  // skip the merely half-antipodal
        pushInstances(hands_list[i], cam_pos, instances);
    std::cout << "Converting " << instances.size() << " training examples (grasps) to images\n";
    hint_ctx_ = anyContextOf(hands_list);
    convertData(instances, file_name, is_plotting);
    hint_ctx_ = nullptr;
  }

  /** learning.cpp:249-318: images -> HOG -> CvSVM::train -> CvSVM::save.  Returns false (after printing why) where the
   *  reference would throw inside OpenCV or write nothing useful. */
  bool convertData(const std::vector<Instance>& instances, const std::string& file_name, bool is_plotting = false,
    bool uses_linear_kernel = false)
  {
    (void) is_plotting;
    agh_ctx* ctx = contextFor(std::vector<GraspHypothesis>());
    if (!ctx)
      return false;
    const std::size_t n = instances.size();
    std::vector<std::uint32_t> images(n * 250);
    std::vector<signed char> labels(n);
    int num_positives = 0;
    for (std::size_t i = 0; i < n; i++)
    {
      if (!instances[i].image)
      {
        std::cout << " Error: hypothesis without training images (HandSearch::setKeepsTrainingImages, "
                     "calculates_antipodal)\n";
        return false;
      }
      for (int w = 0; w < 250; w++)
        images[i * 250 + (std::size_t) w] = instances[i].image[w];
      labels[i] = instances[i].label ? 1 : -1;  // learning.cpp:282-288
      num_positives += instances[i].label ? 1 : 0;
    }
    const int kernel = uses_linear_kernel ? AGH_SVM_LINEAR : AGH_SVM_POLY2;  // learning.cpp:303-309
    const std::size_t sv_cap = uses_linear_kernel ? 1 : (n > 0 ? n : 1);
    std::vector<float> sv(sv_cap * 3528);
    std::vector<double> alpha(sv_cap);
    std::int32_t n_sv = 0, info[6] = { 0, 0, 0, 0, 0, 0 };
    double rho = 0;
    // CvSVMParams defaults (learning.cpp:297): C = 1, term_crit = 1000 iterations / FLT_EPSILON
    if (agh_train_svm(ctx, images.data(), labels.data(), (std::int64_t) n, kernel, 1.0, 1000, 1.1920928955078125e-07,
          sv.data(), (std::int64_t) sv_cap, alpha.data(), &n_sv, &rho, info) != AGH_OK)
    {
      std::cout << " Error: " << agh_last_error(ctx) << "\n";
      return false;
    }
    if (agh_save_svm_file_ex(file_name.c_str(), kernel, sv.data(), n_sv, 3528, alpha.data(), rho, 1.0, 1000,
          1.1920928955078125e-07) != AGH_OK)
    {
      std::cout << " Error: cannot write " << file_name << "\n";
      return false;
    }
    std::cout << "# training examples: " << n << " (# positives: " << num_positives << ", # negatives: "
              << n - (std::size_t) num_positives << ")\n";
    std::cout << "Saved trained SVM as " << file_name << "\n";
    return true;
  }

private:
  agh_ctx* contextFor(const std::vector<GraspHypothesis>& hands_list)
  {
    return hint_ctx_ ? hint_ctx_ : finder_.find(search_, hands_list);
  }

  static agh_ctx* anyContextOf(const std::vector<GraspHypothesis>& hands_list)
  {
    for (std::size_t i = 0; i < hands_list.size(); i++)
      if (hands_list[i].getAnyContext())
        return hands_list[i].getAnyContext();
    return nullptr;
  }

  // the instance for the hand as it is plus the two simulated single-camera views (learning.cpp:64-69, 92-97, 154-158)
  void pushInstances(const GraspHypothesis& h, const Matrix3Xd& cam_pos, std::vector<Instance>& instances) const
  {
    instances.push_back(createInstance(h, cam_pos));
    instances.push_back(createInstance(h, cam_pos, 0));
    instances.push_back(createInstance(h, cam_pos, 1));
  }

  // learning.cpp:21-41 / 100-133: all of `from` if it has at most max_positive entries, else max_positive distinct
  // std::rand() draws in ascending order
  static void selectPositives(const std::vector<int>& from, int max_positive, std::vector<int>& to)
  {
    if ((long) from.size() <= (long) max_positive)
    {
      to.insert(to.end(), from.begin(), from.end());
      return;
    }
    std::set<int> indices;
    while ((long) indices.size() < (long) max_positive)
      indices.insert(indices.end(), std::rand() % (int) from.size());
    std::cout << from.size() << " positive examples found\n";
    std::cout << " randomly selected indices:";
    for (std::set<int>::iterator it = indices.begin(); it != indices.end(); it++)
    {
      std::cout << " " << *it;
      to.push_back(from[(std::size_t) *it]);
    }
    std::cout << std::endl;
  }

  HandSearch* search_;
  int num_threads_;
  agh_ctx* hint_ctx_ = nullptr;         // a live context of the hands being trained on (set around convertData)
  detail::ContextFinder finder_;
};

}  // namespace agile_grasp_amd
#endif
