// depth_adapter_test.cpp -- runs the adapter's depth-image calls (include/agile_grasp_amd/localization.h):
//   depth_adapter_test host                      Localization::toHandles for a chain without a host cloud (needs no GPU)
//   depth_adapter_test gpu <capture.bin> <svm>   localizeHandlesDepth, localizeHandlesDepthBegin / stageNextDepth /
//                                                localizeHandlesEnd and images with poses of their own, each against
//                                                localizeHandles on the cloud agh_deproject makes of the same images
// capture.bin: int64 n_images; per image int64 width, height, row_stride_bytes, double fx, fy, cx, cy, pose[12], then
// height * row_stride_bytes bytes of uint16 pixels; double ws[6]; int64 n_idx; n_idx int32 indices (into the voxelised cloud).
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

int main(int argc, char** argv)
{
  if (argc >= 2 && std::strcmp(argv[1], "host") == 0)
  {
    // what localizeHandlesEnd hands over for a chain begun from depth images: no cloud, here with empty result lists
    Localization loc(1, true, 0);
    std::vector<GraspHypothesis> kept(3);
    const std::vector<Handle> handles = loc.toHandles(PointCloud::Ptr(), std::vector<agh_hypothesis>(), std::vector<agh_handle>(),
      std::vector<std::int32_t>(), &kept);
    std::printf("HOST %zu %zu\n", kept.size(), handles.size());
    return 0;
  }
  if (argc < 4 || std::strcmp(argv[1], "gpu") != 0)
    return 2;
  FILE* f = std::fopen(argv[2], "rb");
  if (!f)
    return 2;
  long long n_images = 0;
  if (std::fread(&n_images, 8, 1, f) != 1 || n_images < 1 || n_images > 2)
    return 2;
  std::vector<std::vector<unsigned char> > pixels((size_t) n_images);
  std::vector<DepthImage> images((size_t) n_images);
  std::vector<agh_depth_image> recs((size_t) n_images);
  Matrix4d tf[2];
  for (long long k = 0; k < n_images; k++)
  {
    long long whs[3];
    double kp[16];
    if (std::fread(whs, 8, 3, f) != 3 || std::fread(kp, 8, 16, f) != 16)
      return 2;
    pixels[(size_t) k].resize((size_t) (whs[1] * whs[2]));
    if (std::fread(pixels[(size_t) k].data(), 1, pixels[(size_t) k].size(), f) != pixels[(size_t) k].size())
      return 2;
    DepthImage& im = images[(size_t) k];
    im.data = pixels[(size_t) k].data();
    im.width = (int) whs[0];
    im.height = (int) whs[1];
    im.row_stride_bytes = whs[2];
    im.fx = kp[0];
    im.fy = kp[1];
    im.cx = kp[2];
    im.cy = kp[3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++)
        tf[k](r, c) = kp[4 + 4 * r + c];
    agh_depth_image& r = recs[(size_t) k];
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
  }
  if (n_images == 1)
    tf[1] = tf[0];
  double ws[6];
  long long n_idx = 0;
  if (std::fread(ws, 8, 6, f) != 6 || std::fread(&n_idx, 8, 1, f) != 1)
    return 2;
  std::vector<int> idx((size_t) n_idx);
  if (std::fread(idx.data(), 4, idx.size(), f) != idx.size())
    return 2;
  std::fclose(f);
  VectorXd w(6);
  for (int i = 0; i < 6; i++)
    w(i) = ws[i];

  // the reference: the points agh_deproject makes of the images, through localizeHandles (size_left = W0 x H0, a dense cloud)
  agh_params p;
  agh_default_params(&p);
  agh_ctx* ctx = nullptr;
  if (agh_create(&p, &ctx) != AGH_OK)
    return 3;
  size_t total = 0;
  for (size_t k = 0; k < images.size(); k++)
    total += (size_t) images[k].width * (size_t) images[k].height;
  std::vector<float> xyz(3 * total);
  if (agh_deproject(ctx, recs.data(), (std::int32_t) recs.size(), xyz.data(), (std::int64_t) total) != (int) total)
  {
    std::printf("agh_deproject: %s\n", agh_last_error(ctx));
    return 3;
  }
  agh_destroy(ctx);
  PointCloud::Ptr cloud(new PointCloud);
  cloud->points.resize(total);
  cloud->is_dense = true;
  for (size_t i = 0; i < total; i++)
  {
    cloud->points[i].x = xyz[3 * i];
    cloud->points[i].y = xyz[3 * i + 1];
    cloud->points[i].z = xyz[3 * i + 2];
  }
  Localization ref(1, false, 0);
  set_up(ref, tf[0], tf[1], w);
  std::vector<GraspHypothesis> kept1;
  const std::vector<Handle> handles1 = ref.localizeHandles(cloud, images[0].width * images[0].height, idx, argv[3], 2, 0.005, &kept1);
  std::printf("POINTS %zu %zu\n", kept1.size(), handles1.size());

  // one call; the images take the transforms of setCameraTransforms as their poses
  Localization loc(1, false, 0);
  set_up(loc, tf[0], tf[1], w);
  std::vector<GraspHypothesis> kept;
  std::vector<Handle> handles = loc.localizeHandlesDepth(images, idx, argv[3], 2, 0.005, &kept);
  std::printf("DEPTH %zu %zu %d\n", kept.size(), handles.size(), same_chain(kept, handles, kept1, handles1) ? 1 : 0);

  // the stream: the next pair of images staged while this one is searched
  std::vector<std::vector<unsigned char> > pixels2 = pixels;
  std::vector<DepthImage> next = images;
  for (size_t k = 0; k < next.size(); k++)
    next[k].data = pixels2[k].data();
  if (!loc.localizeHandlesDepthBegin(images, idx, argv[3], 2, 0.005))
    return 4;
  const bool refused = !loc.localizeHandlesDepthBegin(next, idx, argv[3], 2, 0.005);  // (a chain is pending)
  const bool staged = loc.stageNextDepth(next);
  handles = loc.localizeHandlesEnd(&kept);
  std::printf("STREAM 0 %d %d %d\n", refused ? 1 : 0, staged ? 1 : 0, same_chain(kept, handles, kept1, handles1) ? 1 : 0);
  if (!loc.localizeHandlesDepthBegin(next, idx, argv[3], 2, 0.005))
    return 4;
  handles = loc.localizeHandlesEnd(&kept);
  std::printf("STREAM 1 %d\n", same_chain(kept, handles, kept1, handles1) ? 1 : 0);

  // images with poses of their own; the camera transforms then only give the origins (their translations)
  Matrix4d tl, tr;
  for (int r = 0; r < 3; r++)
  {
    tl(r, 3) = tf[0](r, 3);
    tr(r, 3) = tf[1](r, 3);
  }
  Localization posed(1, false, 0);
  set_up(posed, tl, tr, w);
  std::vector<DepthImage> with_pose = images;
  for (size_t k = 0; k < with_pose.size(); k++)
  {
    with_pose[k].has_pose = true;
    with_pose[k].pose = tf[k];
  }
  handles = posed.localizeHandlesDepth(with_pose, idx, argv[3], 2, 0.005, &kept);
  std::printf("POSED %d\n", same_chain(kept, handles, kept1, handles1) ? 1 : 0);
  return 0;
}
