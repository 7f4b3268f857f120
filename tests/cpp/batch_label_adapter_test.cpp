// batch_label_adapter_test.cpp -- runs the adapter's labelled batch calls (include/agile_grasp_amd/localization.h):
//   batch_label_adapter_test <batch.bin> <svm>  localizeHandlesDepthBatchLabeled and localizeHandlesBatchLabeled against the C
//                                               call (agh_localize_depth_batch_labeled: the same counts, handle records and
//                                               M_{k,j} per list); a labelled Begin while a chain is pending; the labelled
//                                               End while a batch of another kind is pending
// batch.bin: int64 n_captures; double ws[6]; int64 n_samples; int64 seed; per capture int64 n_objects, int64 n_images, per image
// int64 width, height, row_stride_bytes, double fx, fy, cx, cy, pose[12], height * row_stride_bytes bytes of uint16 pixels, int64
// label_row_stride (0: no label image for this image) and height * label_row_stride label bytes.
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_common.h"

static void set_up(Localization& loc, const Matrix4d& tl, const Matrix4d& tr, const VectorXd& w, int n_samples, long long seed)
{
  loc.setCameraTransforms(tl, tr);
  loc.setWorkspace(w);
  loc.setDeterministicNormalEstimation(true);
  loc.setNumSamples(n_samples);
  loc.setSampleSeed((std::uint64_t) seed);
}

typedef std::vector<std::vector<std::vector<GraspHypothesis> > > KeptLists;
typedef std::vector<std::vector<std::vector<Handle> > > HandleLists;

static bool same_batch(const KeptLists& ka, const HandleLists& ha, const KeptLists& kb, const HandleLists& hb)
{
  bool same = ka.size() == kb.size() && ha.size() == hb.size() && ka.size() == ha.size();
  for (size_t k = 0; same && k < ka.size(); k++)
  {
    same = ka[k].size() == kb[k].size() && ha[k].size() == hb[k].size() && ka[k].size() == ha[k].size();
    for (size_t j = 0; same && j < ka[k].size(); j++)
      same = same_chain(ka[k][j], ha[k][j], kb[k][j], hb[k][j]);
  }
  return same;
}

int main(int argc, char** argv)
{
  if (argc < 3)
    return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f)
    return 2;
  long long C = 0, n_samples = 0, seed = 0;
  double ws[6];
  if (std::fread(&C, 8, 1, f) != 1 || C < 1 || C > 64 || std::fread(ws, 8, 6, f) != 6 || std::fread(&n_samples, 8, 1, f) != 1 ||
      std::fread(&seed, 8, 1, f) != 1)
    return 2;
  std::vector<std::vector<std::vector<unsigned char> > > pixels((size_t) C), mask_bytes((size_t) C);
  std::vector<std::vector<DepthImage> > captures((size_t) C);
  std::vector<std::vector<LabelImage> > masks((size_t) C);
  std::vector<int> n_objects((size_t) C);
  std::vector<std::int32_t> n_objects32((size_t) C);
  std::vector<agh_depth_image> recs;  // flat, in capture order
  std::vector<agh_label_image> mrecs;
  std::vector<std::int32_t> n_images_of((size_t) C);
  Matrix4d tf[2];
  for (long long c = 0; c < C; c++)
  {
    long long n_images = 0, objects = 0;
    if (std::fread(&objects, 8, 1, f) != 1 || objects < 1 || objects > 64 || std::fread(&n_images, 8, 1, f) != 1 || n_images < 1 ||
        n_images > 2)
      return 2;
    n_objects[(size_t) c] = (int) objects;
    n_objects32[(size_t) c] = (std::int32_t) objects;
    n_images_of[(size_t) c] = (std::int32_t) n_images;
    pixels[(size_t) c].resize((size_t) n_images);
    mask_bytes[(size_t) c].resize((size_t) n_images);
    for (long long k = 0; k < n_images; k++)
    {
      long long whs[3], stride = 0;
      double kp[16];
      if (std::fread(whs, 8, 3, f) != 3 || std::fread(kp, 8, 16, f) != 16)
        return 2;
      std::vector<unsigned char>& px = pixels[(size_t) c][(size_t) k];
      px.resize((size_t) (whs[1] * whs[2]));
      if (std::fread(px.data(), 1, px.size(), f) != px.size() || std::fread(&stride, 8, 1, f) != 1)
        return 2;
      std::vector<unsigned char>& mb = mask_bytes[(size_t) c][(size_t) k];
      mb.resize((size_t) (stride * whs[1]));
      if (std::fread(mb.data(), 1, mb.size(), f) != mb.size())
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
      masks[(size_t) c].push_back(stride > 0 ? LabelImage(mb.data(), stride) : LabelImage());
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
      recs.push_back(r);
      agh_label_image m;
      m.data = masks[(size_t) c].back().data;
      m.row_stride_bytes = masks[(size_t) c].back().row_stride_bytes;
      mrecs.push_back(m);
    }
  }
  std::fclose(f);
  VectorXd w(6);
  for (int i = 0; i < 6; i++)
    w(i) = ws[i];

  // the C call: the counts, handle records and eligible voxels the adapter's calls must reproduce; the deprojected points and
  // packed labels for the points form
  agh_params p;
  agh_default_params(&p);
  for (int k = 0; k < 2; k++)
    for (int r = 0; r < 3; r++)
      p.cam_origin[k][r] = tf[k](r, 3);
  agh_ctx* ctx = nullptr;
  if (agh_create(&p, &ctx) != AGH_OK || agh_load_svm_file(ctx, argv[2]) != AGH_OK)
    return 3;
  std::vector<PointCloud::Ptr> clouds;
  std::vector<int> sizes_left;
  std::vector<std::vector<std::uint8_t> > packed((size_t) C);
  for (size_t c = 0, i0 = 0; c < captures.size(); i0 += captures[c].size(), c++)
  {
    size_t total = 0;
    for (size_t k = 0; k < captures[c].size(); k++)
      total += (size_t) captures[c][k].width * (size_t) captures[c][k].height;
    std::vector<float> xyz(3 * total);
    if (agh_deproject(ctx, recs.data() + i0, (std::int32_t) captures[c].size(), xyz.data(), (std::int64_t) total) != (int) total)
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
    packed[c].assign(total, 0);
    size_t base = 0;
    for (size_t k = 0; k < captures[c].size(); k++)
    {
      const DepthImage& im = captures[c][k];
      const LabelImage& m = masks[c][k];
      for (int v = 0; v < im.height && m.data; v++)
        std::memcpy(packed[c].data() + base + (size_t) v * im.width, m.data + (size_t) v * m.row_stride_bytes, (size_t) im.width);
      base += (size_t) im.width * (size_t) im.height;
    }
  }
  std::vector<agh_localize_params> lp((size_t) C);
  for (size_t c = 0; c < lp.size(); c++)
  {
    std::memset(&lp[c], 0, sizeof(lp[c]));
    lp[c].classify = 1;
    for (int i = 0; i < 6; i++)
      lp[c].workspace[i] = ws[i];
    lp[c].cell_size = 0.003;
    lp[c].n_samples = n_samples;
    lp[c].sample_seed = (std::uint64_t) seed + (std::uint64_t) c;
    lp[c].min_inliers = 2;
    lp[c].min_length = 0.005;
  }
  size_t L = 0;
  for (size_t c = 0; c < n_objects.size(); c++)
    L += (size_t) n_objects[c];
  const std::int64_t cap = 8 * n_samples * (std::int64_t) L;
  std::vector<agh_handle> c_handles((size_t) cap);
  std::vector<std::int32_t> c_idx((size_t) cap), c_samples((size_t) n_samples * L);
  std::vector<agh_hypothesis> c_hands((size_t) cap);
  std::vector<agh_localize_batch_result> res(L);
  if (agh_localize_depth_batch_labeled(ctx, recs.data(), mrecs.data(), n_images_of.data(), n_objects32.data(), lp.data(), (std::int32_t) C,
        c_handles.data(), cap, c_idx.data(), cap, c_hands.data(), cap, c_samples.data(), res.data()) != AGH_OK)
  {
    std::printf("agh_localize_depth_batch_labeled: %s\n", agh_last_error(ctx));
    return 3;
  }
  std::vector<std::int64_t> m_c(L, -1);
  if (agh_get_batch_label_counts(ctx, m_c.data(), (std::int32_t) L) != AGH_OK)
    return 3;
  agh_destroy(ctx);
  for (size_t c = 0, l = 0; c < n_objects.size(); c++)
    for (int j = 0; j < n_objects[c]; j++, l++)
      std::printf("C %zu %d %lld %lld %lld\n", c, j, (long long) res[l].r.n_hands, (long long) res[l].r.n_handles, (long long) m_c[l]);

  // the adapter's depth form: the C call's counts, handle records and eligible voxels, per capture and object
  Localization loc(1, false, 0);
  set_up(loc, tf[0], tf[1], w, (int) n_samples, seed);
  KeptLists kept;
  HandleLists handles = loc.localizeHandlesDepthBatchLabeled(captures, masks, n_objects, argv[2], 2, 0.005, &kept);
  bool same_counts = handles.size() == (size_t) C && kept.size() == (size_t) C, same_handles = same_counts;
  for (size_t c = 0, l = 0; same_counts && c < handles.size(); c++)
  {
    same_counts = handles[c].size() == (size_t) n_objects[c] && kept[c].size() == (size_t) n_objects[c];
    for (size_t j = 0; same_counts && j < handles[c].size(); j++, l++)
    {
      same_counts = handles[c][j].size() == (size_t) res[l].r.n_handles && kept[c][j].size() == (size_t) res[l].r.n_hands;
      for (size_t i = 0; same_counts && same_handles && i < handles[c][j].size(); i++)
      {
        const agh_handle& h = c_handles[(size_t) res[l].first_handle + i];
        for (int r = 0; same_handles && r < 3; r++)
          same_handles = handles[c][j][i].getAxis()(r) == h.axis[r] && handles[c][j][i].getCenter()(r) == h.center[r] &&
                         handles[c][j][i].getWidth() == h.width && (int) handles[c][j][i].getInliers().size() == h.n_inliers;
      }
    }
  }
  const std::vector<int> list = loc.getLastSampleIndices();
  bool same_list = list.size() == c_samples.size();
  for (size_t i = 0; same_list && i < list.size(); i++)
    same_list = list[i] == c_samples[i];
  std::printf("DEPTH %d %d %d %d\n", same_counts ? 1 : 0, same_handles ? 1 : 0, same_list ? 1 : 0, loc.getBatchLabelCounts() == m_c ? 1 : 0);

  // the points form on the deprojected clouds with the label rows packed
  std::vector<PointCloud::Ptr> clouds2;
  for (size_t c = 0; c < clouds.size(); c++)  // (localizeHandlesBatchEnd filters NaNs out of the searched clouds in place)
    clouds2.push_back(PointCloud::Ptr(new PointCloud(*clouds[c])));
  KeptLists kept1;
  const HandleLists handles1 = loc.localizeHandlesBatchLabeled(clouds2, sizes_left, packed, n_objects, argv[2], 2, 0.005, &kept1);
  std::printf("POINTS %d %d\n", same_batch(kept1, handles1, kept, handles) ? 1 : 0, loc.getBatchLabelCounts() == m_c ? 1 : 0);

  // a labelled Begin while a chain is pending returns false and leaves that chain collectable
  if (!loc.localizeHandlesDepthBatchLabeledBegin(captures, masks, n_objects, argv[2], 2, 0.005))
    return 4;
  std::vector<PointCloud::Ptr> clouds3;
  for (size_t c = 0; c < clouds.size(); c++)
    clouds3.push_back(PointCloud::Ptr(new PointCloud(*clouds[c])));
  const bool refused_depth = !loc.localizeHandlesDepthBatchLabeledBegin(captures, masks, n_objects, argv[2], 2, 0.005);
  const bool refused_points = !loc.localizeHandlesBatchLabeledBegin(clouds3, sizes_left, packed, n_objects, argv[2], 2, 0.005);
  const size_t counts_pending = loc.getBatchLabelCounts().size();
  KeptLists kept2;
  const HandleLists handles2 = loc.localizeHandlesBatchLabeledEnd(&kept2);
  std::printf("PENDING %d %d %zu %d\n", refused_depth ? 1 : 0, refused_points ? 1 : 0, counts_pending,
    same_batch(kept2, handles2, kept, handles) ? 1 : 0);
  // ... and the points form's chain collected through localizeHandlesBatchEnd has one entry per list
  std::vector<PointCloud::Ptr> clouds4;
  for (size_t c = 0; c < clouds.size(); c++)
    clouds4.push_back(PointCloud::Ptr(new PointCloud(*clouds[c])));
  if (!loc.localizeHandlesBatchLabeledBegin(clouds4, sizes_left, packed, n_objects, argv[2], 2, 0.005))
    return 4;
  const std::vector<std::vector<Handle> > flat = loc.localizeHandlesBatchEnd();
  bool same_flat = flat.size() == L;
  for (size_t c = 0, l = 0; same_flat && c < handles.size(); c++)
    for (size_t j = 0; same_flat && j < handles[c].size(); j++, l++)
      same_flat = flat[l].size() == handles[c][j].size();
  std::printf("FLAT %d\n", same_flat ? 1 : 0);
  // a pending batch that is not labelled is not localizeHandlesBatchLabeledEnd's: refused, and still collectable
  if (!loc.localizeHandlesDepthBatchBegin(captures, std::vector<std::vector<int> >((size_t) C), argv[2], 2, 0.005))
    return 4;
  const bool refused_end = loc.localizeHandlesBatchLabeledEnd().empty();
  const std::vector<std::vector<Handle> > plain = loc.localizeHandlesBatchEnd();
  size_t plain_handles = 0;
  for (size_t c = 0; c < plain.size(); c++)
    plain_handles += plain[c].size();
  std::printf("OTHER %d %d %d\n", refused_end ? 1 : 0, plain.size() == (size_t) C ? 1 : 0, plain_handles > 0 ? 1 : 0);
  return 0;
}
