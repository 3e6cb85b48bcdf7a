/*
 * depth_motion_demo.cpp — the camera's motion between depth frames: prep::depthMotion (ppf_depth_motion: whole-image projective
 * point-to-plane ICP over a small pyramid) on every pair of consecutive frames of a stream, and prep::DepthOdometry, which
 * chains them into the camera's pose.  A pose (model -> camera) of frame t - 1 is T * pose in frame t: what
 * Cloud::refineFrame then starts from.  Prints, per pair, the status, the level rows and T, and at the end the accumulated pose;
 * every double with 17 significant digits, so the text identifies the bytes.
 *
 *   usage: depth_motion_demo frames.f32 n_frames rows cols fx fy ppx ppy [levels [iters0 [iters1 [iters2 [iters3 [dist_gate]]]]]]
 *          (raw little-endian file: n_frames images of rows x cols float32 metres, one after the other)
 *   build: g++ -std=c++11 -Iinclude examples/depth_motion_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ppf_cloud_stages.hpp"

using namespace std;
using namespace ppfhip;

static void print16(const char* what, const double* T) {
  printf("%s", what);
  for (int i = 0; i < 16; i++) printf(" %.17g", T[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 9) {
    cerr << "usage: " << argv[0] << " frames.f32 n_frames rows cols fx fy ppx ppy [levels [iters0 [iters1 [iters2 [iters3 [dist_gate]]]]]]" << endl;
    return 1;
  }
  try {
    const int frames = atoi(argv[2]) > 0 ? atoi(argv[2]) : 0;
    const int rows = atoi(argv[3]) > 0 ? atoi(argv[3]) : 0, cols = atoi(argv[4]) > 0 ? atoi(argv[4]) : 0;
    if (frames < 2 || rows == 0 || cols == 0) throw ppf_match_3d::Error(PPF_ERR_INVALID, "at least two frames; rows and cols must be positive");
    const size_t n = (size_t)rows * (size_t)cols;
    vector<float> depth(n * (size_t)frames + 1);
    ifstream f(argv[1], ios::binary);
    if (!f.read(reinterpret_cast<char*>(&depth[0]), (streamsize)(n * (size_t)frames * sizeof(float))))
      throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + argv[1]);
    const double intr[4] = {atof(argv[5]), atof(argv[6]), atof(argv[7]), atof(argv[8])};
    ppf_depth_motion_params mp = prep::defaultDepthMotionParams();
    if (argc > 9) mp.levels = atoi(argv[9]);
    for (int l = 0; l < 4; l++)
      if (argc > 10 + l) mp.iters[l] = atoi(argv[10 + l]);
    if (argc > 14) mp.dist_gate = (float)atof(argv[14]);

    prep::DepthOdometry odometry(rows, cols, intr, &mp);
    odometry.push(&depth[0]);
    for (int k = 1; k < frames; k++) {
      const prep::DepthMotion m = prep::depthMotion(&depth[(size_t)(k - 1) * n], &depth[(size_t)k * n], rows, cols, intr, &mp);
      printf("pair %d status %d evaluations %d of %d launches %d syncs %d\n", k, m.status, m.stats.n_evaluations, m.stats.n_enqueued,
             m.stats.n_launches, m.stats.n_host_syncs);
      for (int l = 0; l < mp.levels; l++) {
        const ppf_depth_motion_level& r = m.levels[l];
        printf("  level %d status %d iterations %d size %d x %d source %d pairs %d -> %d rmse %.9g -> %.9g\n", l, r.status, r.iterations, r.rows,
               r.cols, r.n_source, r.n_pairs_first, r.n_pairs_last, (double)r.rmse_first, (double)r.rmse_last);
      }
      print16("  T", m.T);
      const prep::DepthMotion o = odometry.push(&depth[(size_t)k * n]);
      if (!o.found()) printf("  the odometry keeps its pose\n");
    }
    print16("pose", odometry.pose());
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
