/*
 * depth_normals_demo.cpp — a depth image to object clusters that carry normals and curvature, without a neighbour search:
 * Cloud::fromDepth with ppf_depth_normal_params (ppf_cloud_from_depth_normals: a plane fit over each pixel's image window)
 * -> Cloud::removePlanes -> Cloud::clusters -> Cloud::edges per cluster.  Prints the row counts and, per cloud, a checksum
 * of its bytes (the sum of the 32-bit words of its rows and curvatures, so NaNs count as their bits).
 *
 *   usage: depth_normals_demo depth.f32 rows cols fx fy ppx ppy [radius [max_depth_change [min_neighbours [drop [fp64
 *          [curvature_threshold]]]]]]
 *          (raw little-endian file: rows x cols float32 metres)
 *   build: g++ -std=c++11 -Iinclude examples/depth_normals_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
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

static unsigned long long checksum(const prep::Cloud& c) {
  vector<float> rows, curv;
  c.download(rows, curv);
  unsigned long long sum = 0;
  uint32_t w;
  for (size_t i = 0; i < rows.size(); i++) { memcpy(&w, &rows[i], sizeof(w)); sum += w; }
  for (size_t i = 0; i < curv.size(); i++) { memcpy(&w, &curv[i], sizeof(w)); sum += w; }
  return sum;
}

int main(int argc, char** argv) {
  if (argc < 8) {
    cerr << "usage: " << argv[0]
         << " depth.f32 rows cols fx fy ppx ppy [radius [max_depth_change [min_neighbours [drop [fp64 [curvature_threshold]]]]]]" << endl;
    return 1;
  }
  try {
    const int rows = atoi(argv[2]) > 0 ? atoi(argv[2]) : 0, cols = atoi(argv[3]) > 0 ? atoi(argv[3]) : 0;
    vector<float> depth((size_t)rows * (size_t)cols + 1);
    ifstream f(argv[1], ios::binary);
    if (!f.read(reinterpret_cast<char*>(&depth[0]), (streamsize)((size_t)rows * (size_t)cols * sizeof(float))))
      throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + argv[1]);
    const double fx = atof(argv[4]), fy = atof(argv[5]), ppx = atof(argv[6]), ppy = atof(argv[7]);
    ppf_depth_normal_params np = prep::Cloud::defaultDepthNormalParams();
    if (argc > 8) np.radius = atoi(argv[8]);
    if (argc > 9) np.max_depth_change = (float)atof(argv[9]);
    if (argc > 10) np.min_neighbours = atoi(argv[10]);
    if (argc > 11 && atoi(argv[11])) np.flags |= PPF_DEPTH_NORMALS_DROP;
    const bool fp64 = argc > 12 && atoi(argv[12]) != 0;
    const float threshold = argc > 13 ? (float)atof(argv[13]) : 0.03f;

    const prep::Cloud scene = prep::Cloud::fromDepth(&depth[0], rows, cols, np, fx, fy, ppx, ppy, 0.f, 0.f, fp64);
    printf("scene rows %d checksum %llu\n", scene.size(), checksum(scene));
    const vector<const prep::Cloud*> in(1, &scene);
    const prep::Cloud kept = prep::Cloud::removePlanes(in)[0];
    printf("plane-free rows %d checksum %llu\n", kept.size(), checksum(kept));
    const double intr[4] = {fx, fy, ppx, ppy};
    vector<ppf_cluster_info> info;
    const vector<prep::Cloud> found = kept.clusters(0, &info, intr, rows, cols);
    printf("clusters %d\n", (int)found.size());
    for (size_t r = 0; r < found.size(); r++) {
      const prep::Cloud edge = found[r].edges(threshold);
      printf("cluster %d: rows %d checksum %llu edge rows %d checksum %llu\n", (int)r, found[r].size(), checksum(found[r]), edge.size(),
             checksum(edge));
    }
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
