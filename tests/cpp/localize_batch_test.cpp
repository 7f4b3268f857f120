// localize_batch_test.cpp -- Localization::localizeHandlesBatch against localizeHandles per capture: the same kept hands and
// handles, every double exactly; then localizeHandlesBatchBegin / stageNextBatch / localizeHandlesBatchEnd against the blocking call.
// raw.bin as chain_common.h reads it (the camera origins of the first file hold for all).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chain_common.h"

int main(int argc, char** argv)
{
  // localize_batch_test <filters 0|1> <svm file> <raw.bin>...: localizeHandlesBatch on one object against localizeHandles per
  // capture on another, once with a workspace per capture and once with the object's own workspace for all; then the streamed
  // calls on the first object, one STREAM row per check
  if (argc < 4)
    return 2;
  const bool filters = std::atoi(argv[1]) != 0;
  const char* svm = argv[2];
  const int C = argc - 3;
  std::vector<Capture> c((size_t) C);
  for (int k = 0; k < C; k++)
    if (!read_capture(argv[3 + k], c[(size_t) k]))
      return 2;
  Localization ref(4, filters, 0), loc(4, filters, 0);
  setup(ref, c[0]);
  setup(loc, c[0]);
  std::vector<PointCloud::Ptr> clouds;
  std::vector<int> sizes_left;
  std::vector<std::vector<int> > idx;
  std::vector<VectorXd> ws;
  for (int k = 0; k < C; k++)
  {
    clouds.push_back(PointCloud::Ptr(new PointCloud(*c[(size_t) k].cloud)));
    sizes_left.push_back(c[(size_t) k].size_left);
    idx.push_back(c[(size_t) k].idx);
    VectorXd w(6);
    for (int i = 0; i < 6; i++)
      w(i) = c[(size_t) k].ws[i];
    ws.push_back(w);
  }
  std::vector<std::vector<GraspHypothesis> > kept;
  std::vector<std::vector<Handle> > got = loc.localizeHandlesBatch(clouds, sizes_left, idx, svm, 2, 0.005, &kept, &ws);
  if ((int) got.size() != C || (int) kept.size() != C)
    return 3;
  std::vector<GraspHypothesis> kept_ref0;  // (capture 0's reference, for the last STREAM row)
  std::vector<Handle> handles_ref0;
  for (int k = 0; k < C; k++)
  {
    ref.setWorkspace(ws[(size_t) k]);
    std::vector<GraspHypothesis> kept_ref;
    PointCloud::Ptr copy(new PointCloud(*c[(size_t) k].cloud));
    std::vector<Handle> h = ref.localizeHandles(copy, c[(size_t) k].size_left, c[(size_t) k].idx, svm, 2, 0.005, &kept_ref);
    std::printf("BATCH %d %zu %zu %d\n", k, kept[(size_t) k].size(), got[(size_t) k].size(),
      same_chain(kept[(size_t) k], got[(size_t) k], kept_ref, h) ? 1 : 0);
    if (k == 0)
    {
      kept_ref0 = kept_ref;
      handles_ref0 = h;
    }
  }
  // without workspaces: every capture in the object's workspace (capture 0's)
  std::vector<PointCloud::Ptr> clouds2;
  for (int k = 0; k < C; k++)
    clouds2.push_back(PointCloud::Ptr(new PointCloud(*c[(size_t) k].cloud)));
  std::vector<std::vector<GraspHypothesis> > kept2;
  std::vector<std::vector<Handle> > got2 = loc.localizeHandlesBatch(clouds2, sizes_left, idx, svm, 2, 0.005, &kept2);
  ref.setWorkspace(ws[0]);
  for (int k = 0; k < C; k++)
  {
    std::vector<GraspHypothesis> kept_ref;
    PointCloud::Ptr copy(new PointCloud(*c[(size_t) k].cloud));
    std::vector<Handle> h = ref.localizeHandles(copy, c[(size_t) k].size_left, c[(size_t) k].idx, svm, 2, 0.005, &kept_ref);
    std::printf("OWNWS %d %zu %zu %d\n", k, kept2[(size_t) k].size(), got2[(size_t) k].size(),
      same_chain(kept2[(size_t) k], got2[(size_t) k], kept_ref, h) ? 1 : 0);
  }
  // the streamed calls, with the blocking call's results (kept, got: a workspace per capture) as the expectation: batch A is the
  // captures, batch B the same captures in reverse order (fresh cloud objects: an End filters the NaNs out of its clouds in place)
  std::vector<PointCloud::Ptr> a, b;
  std::vector<int> sizes_left_b;
  std::vector<std::vector<int> > idx_b;
  std::vector<VectorXd> ws_b;
  for (int k = 0; k < C; k++)
  {
    a.push_back(PointCloud::Ptr(new PointCloud(*c[(size_t) k].cloud)));
    b.push_back(PointCloud::Ptr(new PointCloud(*c[(size_t) (C - 1 - k)].cloud)));
    sizes_left_b.push_back(sizes_left[(size_t) (C - 1 - k)]);
    idx_b.push_back(idx[(size_t) (C - 1 - k)]);
    ws_b.push_back(ws[(size_t) (C - 1 - k)]);
  }
  std::printf("STREAM begin_a %d\n", loc.localizeHandlesBatchBegin(a, sizes_left, idx, svm, 2, 0.005, &ws) ? 1 : 0);
  std::printf("STREAM rebegin_refused %d\n", loc.localizeHandlesBatchBegin(b, sizes_left_b, idx_b, svm, 2, 0.005, &ws_b) ? 0 : 1);
  std::printf("STREAM stage_b %d\n", loc.stageNextBatch(b) ? 1 : 0);
  std::vector<std::vector<GraspHypothesis> > kept_a, kept_b;
  std::vector<std::vector<Handle> > got_a = loc.localizeHandlesBatchEnd(&kept_a);
  bool same = (int) got_a.size() == C && (int) kept_a.size() == C;
  for (int k = 0; same && k < C; k++)
    same = same_chain(kept_a[(size_t) k], got_a[(size_t) k], kept[(size_t) k], got[(size_t) k]);
  std::printf("STREAM end_a %d\n", same ? 1 : 0);
  same = loc.localizeHandlesBatchBegin(b, sizes_left_b, idx_b, svm, 2, 0.005, &ws_b);  // (adopts the staged set)
  std::vector<std::vector<Handle> > got_b = loc.localizeHandlesBatchEnd(&kept_b);
  same = same && (int) got_b.size() == C && (int) kept_b.size() == C;
  for (int k = 0; same && k < C; k++)
    same = same_chain(kept_b[(size_t) k], got_b[(size_t) k], kept[(size_t) (C - 1 - k)], got[(size_t) (C - 1 - k)]);
  std::printf("STREAM batch_b %d\n", same ? 1 : 0);
  // the object is usable afterwards: capture 0 in one call (the object's workspace is capture 0's)
  std::vector<GraspHypothesis> kept0;
  PointCloud::Ptr copy0(new PointCloud(*c[0].cloud));
  std::vector<Handle> handles0 = loc.localizeHandles(copy0, c[0].size_left, c[0].idx, svm, 2, 0.005, &kept0);
  std::printf("STREAM after %d\n", same_chain(kept0, handles0, kept_ref0, handles_ref0) ? 1 : 0);
  return 0;
}
