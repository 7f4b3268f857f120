// cloud_cam_origins_test.cpp -- Localization::localizeHandlesBatch with camera transforms PER CAPTURE (the per-cloud origin table,
// agh_set_cloud_cam_origins, through the adapter) against localizeHandles on a Localization set up with each capture's own
// transforms: the same kept hands and handles, every double exactly.
// raw.bin as localize_batch_test.cpp reads it; here every file's own camera origins are used.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "agile_grasp_amd/localization.h"

using namespace agile_grasp_amd;

struct Capture
{
  PointCloud::Ptr cloud;
  int size_left = 0;
  std::vector<int> idx;
  double ws[6], cl[3], cr[3];
};

static bool read_capture(const char* path, Capture& c)
{
  FILE* f = std::fopen(path, "rb");
  if (!f)
    return false;
  long long n = 0, size_left = 0, n_idx = 0;
  bool ok = std::fread(&n, 8, 1, f) == 1 && std::fread(&size_left, 8, 1, f) == 1 && std::fread(&n_idx, 8, 1, f) == 1 &&
            std::fread(c.ws, 8, 6, f) == 6 && std::fread(c.cl, 8, 3, f) == 3 && std::fread(c.cr, 8, 3, f) == 3;
  std::vector<float> xyz(ok ? 3 * (size_t) n : 0);
  c.idx.resize(ok ? (size_t) n_idx : 0);
  ok = ok && std::fread(xyz.data(), 4, xyz.size(), f) == xyz.size() && std::fread(c.idx.data(), 4, c.idx.size(), f) == c.idx.size();
  std::fclose(f);
  if (!ok)
    return false;
  c.size_left = (int) size_left;
  c.cloud = PointCloud::Ptr(new PointCloud);
  c.cloud->points.resize((size_t) n);
  for (long long i = 0; i < n; i++)
  {
    c.cloud->points[(size_t) i].x = xyz[3 * i];
    c.cloud->points[(size_t) i].y = xyz[3 * i + 1];
    c.cloud->points[(size_t) i].z = xyz[3 * i + 2];
  }
  return true;
}

static void transforms(const Capture& c, Matrix4d& tl, Matrix4d& tr)
{
  for (int r = 0; r < 3; r++)
  {
    tl(r, 3) = c.cl[r];
    tr(r, 3) = c.cr[r];
  }
}

static void setup(Localization& loc, const Capture& c)
{
  Matrix4d tl, tr;
  transforms(c, tl, tr);
  loc.setCameraTransforms(tl, tr);
  VectorXd w(6);
  for (int i = 0; i < 6; i++)
    w(i) = c.ws[i];
  loc.setWorkspace(w);
  loc.setDeterministicNormalEstimation(true);
}

// every double of every kept hand and handle, exactly
static bool same_chain(const std::vector<GraspHypothesis>& ka, const std::vector<Handle>& ha, const std::vector<GraspHypothesis>& kb,
  const std::vector<Handle>& hb)
{
  bool same = ka.size() == kb.size() && ha.size() == hb.size();
  for (size_t i = 0; same && i < ka.size(); i++)
    for (int r = 0; same && r < 3; r++)
      same = ka[i].getGraspSurface()(r) == kb[i].getGraspSurface()(r) && ka[i].getGraspBottom()(r) == kb[i].getGraspBottom()(r) &&
             ka[i].getApproach()(r) == kb[i].getApproach()(r) && ka[i].getAxis()(r) == kb[i].getAxis()(r) &&
             ka[i].getGraspWidth() == kb[i].getGraspWidth() && ka[i].isFullAntipodal() == kb[i].isFullAntipodal();
  for (size_t i = 0; same && i < ha.size(); i++)
    for (int r = 0; same && r < 3; r++)
      same = ha[i].getInliers() == hb[i].getInliers() && ha[i].getAxis()(r) == hb[i].getAxis()(r) &&
             ha[i].getCenter()(r) == hb[i].getCenter()(r) && ha[i].getApproach()(r) == hb[i].getApproach()(r) &&
             ha[i].getBinormal()(r) == hb[i].getBinormal()(r) && ha[i].getWidth() == hb[i].getWidth();
  return same;
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
