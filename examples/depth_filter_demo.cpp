/*
 * depth_filter_demo.cpp — a depth image cleaned before anything is built on it: prep::filterDepth (ppf_depth_filter: the
 * unsupported "flying" pixels removed, the others smoothed without crossing a depth step) -> Cloud::fromDepth with
 * ppf_depth_normal_params, once on the raw and once on the filtered image.  Prints the filter's counts and, per image and
 * cloud, the row count, the rows with a curvature above the threshold and a checksum of the bytes (the sum of the 32-bit
 * words, so NaNs count as their bits).
 *
 *   usage: depth_filter_demo depth.f32 rows cols fx fy ppx ppy [radius [range_abs [range_quad [support_abs [support_quad
 *          [min_support [curvature_threshold]]]]]]]
 *          (raw little-endian file: rows x cols float32 metres)
 *   build: g++ -std=c++11 -Iinclude examples/depth_filter_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ppf_cloud_stages.hpp"

using namespace std;
using namespace ppfhip;

static unsigned long long checksum(const vector<float>& a, unsigned long long sum = 0) {
  uint32_t w;
  for (size_t i = 0; i < a.size(); i++) { memcpy(&w, &a[i], sizeof(w)); sum += w; }
  return sum;
}

static void report(const char* name, const vector<float>& image, int rows, int cols, const double* intr, float threshold) {
  const prep::Cloud scene = prep::Cloud::fromDepth(&image[0], rows, cols, prep::Cloud::defaultDepthNormalParams(), intr[0], intr[1],
                                                   intr[2], intr[3], 0.f, 0.f, true);
  vector<float> r, curv;
  scene.download(r, curv);
  int over = 0;
  for (size_t i = 0; i < curv.size(); i++) over += curv[i] > threshold ? 1 : 0;
  printf("%s image checksum %llu cloud rows %d over %d checksum %llu\n", name, checksum(image), scene.size(), over,
         checksum(curv, checksum(r)));
}

int main(int argc, char** argv) {
  if (argc < 8) {
    cerr << "usage: " << argv[0]
         << " depth.f32 rows cols fx fy ppx ppy [radius [range_abs [range_quad [support_abs [support_quad [min_support "
            "[curvature_threshold]]]]]]]" << endl;
    return 1;
  }
  try {
    const int rows = atoi(argv[2]) > 0 ? atoi(argv[2]) : 0, cols = atoi(argv[3]) > 0 ? atoi(argv[3]) : 0;
    if (rows == 0 || cols == 0) throw ppf_match_3d::Error(PPF_ERR_INVALID, "rows and cols must be positive");
    vector<float> depth((size_t)rows * (size_t)cols + 1);
    ifstream f(argv[1], ios::binary);
    if (!f.read(reinterpret_cast<char*>(&depth[0]), (streamsize)((size_t)rows * (size_t)cols * sizeof(float))))
      throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + argv[1]);
    depth.resize((size_t)rows * (size_t)cols);
    const double intr[4] = {atof(argv[4]), atof(argv[5]), atof(argv[6]), atof(argv[7])};
    ppf_depth_filter_params fp = prep::defaultDepthFilterParams();
    if (argc > 8) fp.radius = atoi(argv[8]);
    if (argc > 9) fp.range_abs = (float)atof(argv[9]);
    if (argc > 10) fp.range_quad = (float)atof(argv[10]);
    if (argc > 11) fp.support_abs = (float)atof(argv[11]);
    if (argc > 12) fp.support_quad = (float)atof(argv[12]);
    if (argc > 13) fp.min_support = atoi(argv[13]);
    const float threshold = argc > 14 ? (float)atof(argv[14]) : 0.03f;

    ppf_depth_filter_stats st;
    const vector<float> filtered = prep::filterDepth(&depth[0], rows, cols, &fp, 0.f, 0.f, 0, &st);
    printf("kept %d unsupported %d written %d\n", st.n_kept, st.n_unsupported, st.n_written);
    report("raw", depth, rows, cols, intr, threshold);
    report("filtered", filtered, rows, cols, intr, threshold);
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
