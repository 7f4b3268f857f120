// depth_fusion_adapter_test.cpp -- the adapter's depth-fusion methods (include/agile_grasp_amd/hand_search.h, localization.h):
// fuseDepth, depthFusionCounts and fusedDepth on Localization and on HandSearch, used the way a caller would; compiled in both
// type branches by tests/test_depth_fusion_adapter.py.
//   depth_fusion_adapter_test            usage (2): it leaves before it touches a device
//   depth_fusion_adapter_test run        fuses a constructed burst of three 5 x 2 uint16 frames and prints what the calls return
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_common.h"

int main(int argc, char** argv)
{
  if (argc != 2 || std::strcmp(argv[1], "run") != 0)
  {
    std::printf("usage: depth_fusion_adapter_test run\n");
    return 2;
  }
  const int W = 5, H = 2, T = 3;
  // per pixel the three readings: agreeing, one hole, the hole last, all holes, two sides and a hole, one reading only
  const std::uint16_t px[W * H][T] = { { 1000, 1001, 1002 }, { 0, 500, 501 }, { 700, 701, 0 }, { 0, 0, 0 }, { 400, 900, 0 },
                                       { 0, 0, 300 }, { 1, 1, 1 }, { 65535, 65535, 65535 }, { 1, 2, 0 }, { 2000, 2000, 2001 } };
  std::vector<std::vector<std::uint16_t> > bytes(T, std::vector<std::uint16_t>(W * H));
  std::vector<DepthImage> frames(T);
  for (int t = 0; t < T; t++)
  {
    for (int p = 0; p < W * H; p++)
      bytes[t][p] = px[p][t];
    frames[t].data = bytes[t].data();
    frames[t].width = W;
    frames[t].height = H;
    frames[t].row_stride_bytes = W * 2;
    frames[t].fx = frames[t].fy = 100.0;
    frames[t].cx = 2.0;
    frames[t].cy = 1.0;
  }
  agh_depth_fusion_params fp;
  agh_default_depth_fusion_params(&fp);

  Localization loc(1, false, 0);
  agh_depth_fusion_counts counts;
  std::vector<std::uint8_t> pixels;
  DepthImage fused;
  const bool none_before = !loc.depthFusionCounts(3, counts) && !loc.fusedDepth(3, pixels, fused);
  agh_depth_image rec;
  const bool ok = loc.fuseDepth(frames, fp, 3, 0, &rec);
  const bool has = loc.depthFusionCounts(3, counts) && loc.fusedDepth(3, pixels, fused);
  std::printf("LOCALIZATION %d %d %d %d %d\n", none_before ? 1 : 0, ok ? 1 : 0, has ? 1 : 0, rec.data != nullptr ? 1 : 0,
    (int) (fused.width == W && fused.height == H && !fused.is_float && fused.row_stride_bytes == W * 2 && fused.has_pose));
  std::printf("COUNTS %lld %lld %lld %lld %lld %lld\n", (long long) counts.n_pixels, (long long) counts.n_empty,
    (long long) counts.n_unsupported, (long long) counts.n_inconsistent, (long long) counts.n_fused, (long long) counts.n_filled);
  std::printf("PIXELS");
  for (int p = 0; has && p < W * H; p++)
    std::printf(" %u", (unsigned) reinterpret_cast<const std::uint16_t*>(pixels.data())[p]);
  std::printf("\n");
  fp.min_valid = T + 1;  // refused: the slot's image stays
  const bool refused = !loc.fuseDepth(frames, fp, 3);
  std::vector<std::uint8_t> again;
  const bool kept = loc.fusedDepth(3, again, fused) && again == pixels;

  HandSearch& search = loc.getHandSearch();
  fp.min_valid = 1;
  const bool s_ok = search.fuseDepth(frames, fp, 127, 1);
  const bool s_has = search.depthFusionCounts(127, counts) && search.fusedDepth(127, again, fused);
  std::printf("SEARCH %d %d %d %d %lld\n", refused ? 1 : 0, kept ? 1 : 0, s_ok ? 1 : 0, s_has ? 1 : 0, (long long) counts.n_fused);
  return 0;
}
