/*
 * frame_select_demo.cpp — the post-detector half of the reference's driver for every detection of a frame, ending in one
 * consistent set of poses instead of the reference's `return *resultsSub[0];` per box: Cloud::prepareFrame,
 * Cloud::matchFrame (Matching_S2B + ICP of the top 8 poses of every detection), then Cloud::selectFrame, which suppresses
 * duplicates and the same object seen through overlapping boxes and keeps a second instance inside one box.  Every box is
 * matched against the one model given.  Prints one line per pose with its info row, then the selection in order; writes
 * the depth (float32 metres, 0 where empty) and label (int32 flat index detection * top + k, -1 where empty) images of the
 * selected poses.
 *
 *   usage: frame_select_demo scene_xyz.f32 n_points depth.f32 rows cols fx fy ppx ppy boxes.i32 n_boxes model_xyzn.f32 n_model
 *          out_depth.f32 out_label.i32 [min_score]
 *          (raw little-endian files: scene n x 3 float32, depth rows x cols float32 metres, boxes n x 4 int32 {x y w h},
 *           model n x 6 float32 x y z nx ny nz)
 *   build: g++ -std=c++11 -Iinclude examples/frame_select_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
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

template <class T>
static void read_raw(const char* path, vector<T>& v, size_t count) {
  ifstream f(path, ios::binary);
  if (!f.read(reinterpret_cast<char*>(&v[0]), (streamsize)(count * sizeof(T))))
    throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + path);
}

int main(int argc, char** argv) {
  if (argc < 16) {
    cerr << "usage: " << argv[0]
         << " scene_xyz.f32 n_points depth.f32 rows cols fx fy ppx ppy boxes.i32 n_boxes model_xyzn.f32 n_model out_depth.f32 out_label.i32"
         << endl;
    return 1;
  }
  try {
    const int n = atoi(argv[2]), rows = atoi(argv[4]), cols = atoi(argv[5]), nb = atoi(argv[11]), nm = atoi(argv[13]);
    vector<float> xyz((size_t)n * 3 + 1), depth((size_t)rows * cols), model((size_t)nm * 6 + 1);
    vector<int> boxes((size_t)nb * 4 + 1);
    read_raw(argv[1], xyz, (size_t)n * 3);
    read_raw(argv[3], depth, depth.size());
    if (nb) read_raw(argv[10], boxes, (size_t)nb * 4);
    read_raw(argv[12], model, (size_t)nm * 6);

    prep::Cloud scene = prep::Cloud::fromXYZ(&xyz[0], n);
    const vector<pair<prep::Cloud, prep::Cloud> > dets =
        scene.prepareFrame(&boxes[0], nb, &depth[0], rows, cols, atof(argv[6]), atof(argv[7]), atof(argv[8]), atof(argv[9]));

    ppf_match_3d::PPF3DDetector detector(0.05, 0.05);
    detector.trainModel(&model[0], nm, 6);
    const prep::Cloud modelCloud = prep::Cloud::fromRows(&model[0], nm, 6, 6);
    const vector<const ppf_model*> models(dets.size(), detector.handle());
    const vector<const prep::Cloud*> modelClouds(dets.size(), &modelCloud);
    const vector<vector<ppf_match_3d::Pose3D> > poses = prep::Cloud::matchFrame(models, modelClouds, dets, 0.05, 0.05, 8);
    const double fx = atof(argv[6]), fy = atof(argv[7]), ppx = atof(argv[8]), ppy = atof(argv[9]);
    ppf_select_params sp;
    ppf_default_select_params(&sp);
    if (argc > 16) sp.min_score = (float)atof(argv[16]);
    vector<vector<ppf_select_info> > info;
    vector<float> img;
    vector<int32_t> label;
    ppf_select_stats st;
    const vector<pair<int, int> > chosen =
        prep::Cloud::selectFrame(modelClouds, poses, &depth[0], rows, cols, fx, fy, ppx, ppy, &sp, 0, 0, &info, &img, &label, &st);
    for (size_t i = 0; i < info.size(); i++)
      for (size_t k = 0; k < info[i].size(); k++) {
        const ppf_select_info& r = info[i][k];
        printf("pose %d %d: status %d rank %d suppressed_by %d n_drawn %d n_supported %d n_overlap %d explained %.9g key %.9g\n", (int)i,
               (int)k, r.status, r.rank, r.suppressed_by, r.n_drawn, r.n_supported, r.n_overlap, (double)r.explained, (double)r.key);
      }
    for (size_t r = 0; r < chosen.size(); r++) printf("selected %d: det %d k %d\n", (int)r, chosen[r].first, chosen[r].second);
    printf("eligible %d selected %d\n", st.n_eligible, st.n_selected);
    ofstream(argv[14], ios::binary).write(reinterpret_cast<const char*>(&img[0]), (streamsize)(img.size() * sizeof(float)));
    ofstream(argv[15], ios::binary).write(reinterpret_cast<const char*>(&label[0]), (streamsize)(label.size() * sizeof(int32_t)));
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
