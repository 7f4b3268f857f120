// depth_batch_adapter_test.cpp -- runs the adapter's depth-batch calls (include/agile_grasp_amd/localization.h):
//   depth_batch_adapter_test <batch.bin> <svm>   localizeHandlesDepthBatch, localizeHandlesDepthBatchBegin /
//                                                localizeHandlesBatchEnd and the overload with per-capture camera transforms,
//                                                each against localizeHandlesBatch on the clouds agh_deproject makes
// batch.bin: int64 n_captures; double ws[6]; per capture int64 n_images, per image int64 width, height, row_stride_bytes,
// double fx, fy, cx, cy, pose[12], then height * row_stride_bytes bytes of uint16 pixels; then int64 n_idx and n_idx int32
// indices (into the capture's voxelised cloud).
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_common.h"

static void set_up(Localization& loc, const Matrix4d& tl, const Matrix4d& tr, const VectorXd& w)
{
  loc.setCameraTransforms(tl, tr);
  loc.setWorkspace(w);
  loc.setDeterministicNormalEstimation(true);
}

static bool same_batch(const std::vector<std::vector<GraspHypothesis> >& ka, const std::vector<std::vector<Handle> >& ha,
  const std::vector<std::vector<GraspHypothesis> >& kb, const std::vector<std::vector<Handle> >& hb)
{
  bool same = ka.size() == kb.size() && ha.size() == hb.size() && ka.size() == ha.size();
  for (size_t k = 0; same && k < ka.size(); k++)
    same = same_chain(ka[k], ha[k], kb[k], hb[k]);
  return same;
}

int main(int argc, char** argv)
{
  if (argc < 3)
    return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f)
    return 2;
  long long C = 0;
  double ws[6];
  if (std::fread(&C, 8, 1, f) != 1 || C < 1 || C > 64 || std::fread(ws, 8, 6, f) != 6)
    return 2;
  std::vector<std::vector<std::vector<unsigned char> > > pixels((size_t) C);
  std::vector<std::vector<DepthImage> > captures((size_t) C);
  std::vector<std::vector<agh_depth_image> > recs((size_t) C);
  std::vector<std::vector<int> > idx((size_t) C);
  Matrix4d tf[2];
  for (long long c = 0; c < C; c++)
  {
    long long n_images = 0, n_idx = 0;
    if (std::fread(&n_images, 8, 1, f) != 1 || n_images < 1 || n_images > 2)
      return 2;
    pixels[(size_t) c].resize((size_t) n_images);
    for (long long k = 0; k < n_images; k++)
    {
      long long whs[3];
      double kp[16];
      if (std::fread(whs, 8, 3, f) != 3 || std::fread(kp, 8, 16, f) != 16)
        return 2;
      std::vector<unsigned char>& px = pixels[(size_t) c][(size_t) k];
      px.resize((size_t) (whs[1] * whs[2]));
      if (std::fread(px.data(), 1, px.size(), f) != px.size())
        return 2;
      DepthImage im;
      im.data = px.data();
      im.width = (int) whs[0];
      im.height = (int) whs[1];
      im.row_stride_bytes = whs[2];
      im.fx = kp[0];
      im.fy = kp[1];
      im.cx = kp[2];
      im.cy = kp[3];
      for (int r = 0; r < 3; r++)
        for (int q = 0; q < 4; q++)
          tf[k](r, q) = kp[4 + 4 * r + q];  // (every capture of the file was taken by the same rig)
      captures[(size_t) c].push_back(im);
      agh_depth_image r;
      r.data = im.data;
      r.width = im.width;
      r.height = im.height;
      r.row_stride_bytes = im.row_stride_bytes;
      r.format = AGH_DEPTH_U16;
      r.depth_scale = im.depth_scale;
      r.fx = im.fx;
      r.fy = im.fy;
      r.cx = im.cx;
      r.cy = im.cy;
      std::memcpy(r.pose, kp + 4, sizeof(r.pose));
      recs[(size_t) c].push_back(r);
    }
    if (std::fread(&n_idx, 8, 1, f) != 1)
      return 2;
    idx[(size_t) c].resize((size_t) n_idx);
    if (std::fread(idx[(size_t) c].data(), 4, idx[(size_t) c].size(), f) != idx[(size_t) c].size())
      return 2;
  }
  std::fclose(f);
  VectorXd w(6);
  for (int i = 0; i < 6; i++)
    w(i) = ws[i];

  // the reference: the points agh_deproject makes of each capture, through localizeHandlesBatch (size_left = W0 x H0, dense)
  agh_params p;
  agh_default_params(&p);
  agh_ctx* ctx = nullptr;
  if (agh_create(&p, &ctx) != AGH_OK)
    return 3;
  std::vector<PointCloud::Ptr> clouds;
  std::vector<int> sizes_left;
  for (size_t c = 0; c < captures.size(); c++)
  {
    size_t total = 0;
    for (size_t k = 0; k < captures[c].size(); k++)
      total += (size_t) captures[c][k].width * (size_t) captures[c][k].height;
    std::vector<float> xyz(3 * total);
    if (agh_deproject(ctx, recs[c].data(), (std::int32_t) recs[c].size(), xyz.data(), (std::int64_t) total) != (int) total)
    {
      std::printf("agh_deproject: %s\n", agh_last_error(ctx));
      return 3;
    }
    PointCloud::Ptr cloud(new PointCloud);
    cloud->points.resize(total);
    cloud->is_dense = true;
    for (size_t i = 0; i < total; i++)
    {
      cloud->points[i].x = xyz[3 * i];
      cloud->points[i].y = xyz[3 * i + 1];
      cloud->points[i].z = xyz[3 * i + 2];
    }
    clouds.push_back(cloud);
    sizes_left.push_back(captures[c][0].width * captures[c][0].height);
  }
  agh_destroy(ctx);
  Localization ref(1, false, 0);
  set_up(ref, tf[0], tf[1], w);
  std::vector<std::vector<GraspHypothesis> > kept1;
  const std::vector<std::vector<Handle> > handles1 = ref.localizeHandlesBatch(clouds, sizes_left, idx, argv[2], 2, 0.005, &kept1);
  size_t n_kept = 0, n_handles = 0, least = (size_t) -1;
  for (size_t c = 0; c < kept1.size(); c++)
  {
    n_kept += kept1[c].size();
    n_handles += handles1[c].size();
    least = kept1[c].size() < least ? kept1[c].size() : least;
  }
  std::printf("POINTS %zu %zu %zu %zu\n", kept1.size(), least, n_kept, n_handles);

  // one call; the images take the transforms of setCameraTransforms as their poses
  Localization loc(1, false, 0);
  set_up(loc, tf[0], tf[1], w);
  std::vector<std::vector<GraspHypothesis> > kept;
  std::vector<std::vector<Handle> > handles = loc.localizeHandlesDepthBatch(captures, idx, argv[2], 2, 0.005, &kept);
  std::printf("DEPTH %d\n", same_batch(kept, handles, kept1, handles1) ? 1 : 0);

  // the two halves: a second Begin of either kind is refused while the chain is pending
  if (!loc.localizeHandlesDepthBatchBegin(captures, idx, argv[2], 2, 0.005))
    return 4;
  const bool refused = !loc.localizeHandlesDepthBatchBegin(captures, idx, argv[2], 2, 0.005) &&
                       !loc.localizeHandlesBatchBegin(clouds, sizes_left, idx, argv[2], 2, 0.005);
  handles = loc.localizeHandlesBatchEnd(&kept);
  std::printf("HALVES %d %d\n", refused ? 1 : 0, same_batch(kept, handles, kept1, handles1) ? 1 : 0);

  // per-capture transforms (the same rig for every capture here): the images carry their poses, the object's own transforms
  // are elsewhere, and the origins come from the table
  Matrix4d far_l, far_r;
  far_l(0, 3) = 5.0;
  far_r(1, 3) = -5.0;
  Localization rigs(1, false, 0);
  set_up(rigs, far_l, far_r, w);
  std::vector<std::vector<DepthImage> > with_pose = captures;
  for (size_t c = 0; c < with_pose.size(); c++)
    for (size_t k = 0; k < with_pose[c].size(); k++)
    {
      with_pose[c][k].has_pose = true;
      with_pose[c][k].pose = tf[k];
    }
  const std::vector<Matrix4d> cams_left(captures.size(), tf[0]), cams_right(captures.size(), tf[1]);
  handles = rigs.localizeHandlesDepthBatch(with_pose, idx, argv[2], 2, 0.005, cams_left, cams_right, &kept);
  std::printf("RIGS %d\n", same_batch(kept, handles, kept1, handles1) ? 1 : 0);
  // ... and without the table the far origins give other hands
  handles = rigs.localizeHandlesDepthBatch(with_pose, idx, argv[2], 2, 0.005, &kept);
  std::printf("FAR %d\n", same_batch(kept, handles, kept1, handles1) ? 1 : 0);
  return 0;
}
