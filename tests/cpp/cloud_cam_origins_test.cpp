// cloud_cam_origins_test.cpp -- Localization::localizeHandlesBatch with camera transforms PER CAPTURE (the per-cloud origin table,
// agh_set_cloud_cam_origins, through the adapter) against localizeHandles on a Localization set up with each capture's own
// transforms: the same kept hands and handles, every double exactly.
// raw.bin as chain_common.h reads it; here every file's own camera origins are used.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chain_common.h"

static void transforms(const Capture& c, Matrix4d& tl, Matrix4d& tr)
{
  for (int r = 0; r < 3; r++)
  {
    tl(r, 3) = c.cl[r];
    tr(r, 3) = c.cr[r];
  }
}

int main(int argc, char** argv)
{
  // cloud_cam_origins_test <svm file> <raw.bin>...: prints, per capture k,
  //   MIXED k <kept> <handles> <1 if equal to localizeHandles under capture k's transforms>
  //   SHARED k <1 if the plain overload (capture 0's transforms for all) gives capture k the same result as MIXED>
  // and a last MIXED run after the plain one (the table was cleared, and is set again).
  if (argc < 3)
    return 2;
  const char* svm = argv[1];
  const int C = argc - 2;
  std::vector<Capture> c((size_t) C);
  for (int k = 0; k < C; k++)
    if (!read_capture(argv[2 + k], c[(size_t) k]))
      return 2;
  Localization loc(4, false, 0);
  setup(loc, c[0]);
  std::vector<int> sizes_left;
  std::vector<std::vector<int> > idx;
  std::vector<VectorXd> ws;
  std::vector<Matrix4d> tl((size_t) C), tr((size_t) C);
  for (int k = 0; k < C; k++)
  {
    sizes_left.push_back(c[(size_t) k].size_left);
    idx.push_back(c[(size_t) k].idx);
    VectorXd w(6);
    for (int i = 0; i < 6; i++)
      w(i) = c[(size_t) k].ws[i];
    ws.push_back(w);
    transforms(c[(size_t) k], tl[(size_t) k], tr[(size_t) k]);
  }
  std::vector<std::vector<GraspHypothesis> > kept_first;
  std::vector<std::vector<Handle> > got_first;
  for (int round = 0; round < 2; round++)
  {
    std::vector<PointCloud::Ptr> clouds;
    for (int k = 0; k < C; k++)
      clouds.push_back(PointCloud::Ptr(new PointCloud(*c[(size_t) k].cloud)));
    std::vector<std::vector<GraspHypothesis> > kept;
    std::vector<std::vector<Handle> > got = loc.localizeHandlesBatch(clouds, sizes_left, idx, svm, 2, 0.005, tl, tr, &kept, &ws);
    if ((int) got.size() != C || (int) kept.size() != C)
      return 3;
    for (int k = 0; k < C; k++)
    {
      Localization ref(4, false, 0);
      setup(ref, c[(size_t) k]);
      std::vector<GraspHypothesis> kept_ref;
      PointCloud::Ptr copy(new PointCloud(*c[(size_t) k].cloud));
      std::vector<Handle> h = ref.localizeHandles(copy, c[(size_t) k].size_left, c[(size_t) k].idx, svm, 2, 0.005, &kept_ref);
      std::printf("MIXED %d %zu %zu %d\n", k, kept[(size_t) k].size(), got[(size_t) k].size(),
        same_chain(kept[(size_t) k], got[(size_t) k], kept_ref, h) ? 1 : 0);
    }
    if (round == 0)
    {
      kept_first = kept;
      got_first = got;
      // the plain overload afterwards: no table left behind, capture 0's transforms for every capture
      std::vector<PointCloud::Ptr> clouds2;
      for (int k = 0; k < C; k++)
        clouds2.push_back(PointCloud::Ptr(new PointCloud(*c[(size_t) k].cloud)));
      std::vector<std::vector<GraspHypothesis> > kept2;
      std::vector<std::vector<Handle> > got2 = loc.localizeHandlesBatch(clouds2, sizes_left, idx, svm, 2, 0.005, &kept2, &ws);
      if ((int) got2.size() != C)
        return 3;
      for (int k = 0; k < C; k++)
        std::printf("SHARED %d %d\n", k, same_chain(kept2[(size_t) k], got2[(size_t) k], kept_first[(size_t) k], got_first[(size_t) k]) ? 1 : 0);
    }
  }
  // one transform too few: printed, empty lists
  std::vector<PointCloud::Ptr> clouds3;
  for (int k = 0; k < C; k++)
    clouds3.push_back(PointCloud::Ptr(new PointCloud(*c[(size_t) k].cloud)));
  std::vector<Matrix4d> tl_short(tl.begin(), tl.end() - 1);
  std::vector<std::vector<Handle> > got3 = loc.localizeHandlesBatch(clouds3, sizes_left, idx, svm, 2, 0.005, tl_short, tr);
  size_t n3 = 0;
  for (size_t k = 0; k < got3.size(); k++)
    n3 += got3[k].size();
  std::printf("SHORT %zu %zu\n", got3.size(), n3);
  return 0;
}
