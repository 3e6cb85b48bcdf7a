/*
 * depth_frame_demo.cpp — the reference's driver from the depth image alone (src/YOLO_cropping_ppf_test.cpp:84-127 with
 * CloudProcessor::Deprojection filled in): Cloud::fromDepth back-projects the frame on the device, Cloud::prepareFrame
 * prepares every box, Cloud::matchFrame runs Matching_S2B and the ICP of all detections.  Every box is matched against
 * the one model given.  Prints the scene cloud's size, then per detection its refined best pose (the reference's
 * results[0]) and the call's counters.
 *
 *   usage: depth_frame_demo depth.f32 rows cols fx fy ppx ppy boxes.i32 n_boxes model_xyzn.f32 n_model [fp64]
 *          (raw little-endian files: depth rows x cols float32 metres, boxes n x 4 int32 {x y w h}, model n x 6 float32
 *           x y z nx ny nz; "fp64": the fp64 back-projection instead of Camera::back_projection's rounding)
 *   build: g++ -std=c++11 -Iinclude examples/depth_frame_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
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

template <class T>
static void read_raw(const char* path, vector<T>& v, size_t count) {
  ifstream f(path, ios::binary);
  if (!f.read(reinterpret_cast<char*>(&v[0]), (streamsize)(count * sizeof(T))))
    throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + path);
}

int main(int argc, char** argv) {
  if (argc < 12) {
    cerr << "usage: " << argv[0] << " depth.f32 rows cols fx fy ppx ppy boxes.i32 n_boxes model_xyzn.f32 n_model [fp64]" << endl;
    return 1;
  }
  try {
    const int rows = atoi(argv[2]), cols = atoi(argv[3]), nb = atoi(argv[9]), nm = atoi(argv[11]);
    const double fx = atof(argv[4]), fy = atof(argv[5]), ppx = atof(argv[6]), ppy = atof(argv[7]);
    const bool fp64 = argc > 12 && strcmp(argv[12], "fp64") == 0;
    vector<float> depth((size_t)rows * cols + 1), model((size_t)nm * 6 + 1);
    vector<int> boxes((size_t)nb * 4 + 1);
    read_raw(argv[1], depth, (size_t)rows * cols);
    if (nb) read_raw(argv[8], boxes, (size_t)nb * 4);
    read_raw(argv[10], model, (size_t)nm * 6);

    /* Deprojection(CameraIntr): the scene cloud, resident in HBM */
    const prep::Cloud scene = prep::Cloud::fromDepth(&depth[0], rows, cols, fx, fy, ppx, ppy, 0.f, 0.f, fp64);
    printf("scene_points %d\n", scene.size());
    const vector<pair<prep::Cloud, prep::Cloud> > dets = scene.prepareFrame(&boxes[0], nb, &depth[0], rows, cols, fx, fy, ppx, ppy);

    ppf_match_3d::PPF3DDetector detector(0.025, 0.05);           /* TrainDetector(0.025, 0.05), CloudProcessing.h:234 */
    detector.trainModel(&model[0], nm, 6);
    const prep::Cloud modelCloud = prep::Cloud::fromRows(&model[0], nm, 6, 6);
    const vector<const ppf_model*> models(dets.size(), detector.handle());
    const vector<const prep::Cloud*> modelClouds(dets.size(), &modelCloud);
    vector<vector<int> > iterations;
    const vector<vector<ppf_match_3d::Pose3D> > poses = prep::Cloud::matchFrame(models, modelClouds, dets, 0.05, 0.05, 5, &iterations);
    for (size_t i = 0; i < poses.size(); i++) {
      if (poses[i].empty()) {
        printf("det %d: none\n", (int)i);
        continue;
      }
      const ppf_match_3d::Pose3D& p = poses[i][0];
      printf("det %d: poses %d votes %d iterations %d residual %.17g pose", (int)i, (int)poses[i].size(), (int)p.numVotes, iterations[i][0],
             p.residual);
      for (int k = 0; k < 16; k++) printf(" %.17g", p.pose.val[k]);
      printf("\n");
    }
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
